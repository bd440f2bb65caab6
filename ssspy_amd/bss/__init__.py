from . import (admmbss, base, cacgmm, convilrma, conviva, fdica, hva, ica, ilrma, ipsdta, iva, mnmf,
               overiva, pdsbss, proxbss)
from .admmbss import ADMMBSS, ADMMBSSBase, MaskingADMMBSS
from .base import IterativeMethodBase
from .cacgmm import CACGMM, CACGMMBase
from .convilrma import ConvGaussILRMA
from .conviva import ConvGaussIVA, ConvIVABase, ConvLaplaceIVA
from .fdica import (
    AuxFDICA,
    AuxLaplaceFDICA,
    FDICABase,
    GradFDICA,
    GradFDICABase,
    GradLaplaceFDICA,
    NaturalGradFDICA,
    NaturalGradLaplaceFDICA,
)
from .hva import HVA, MaskingADMMHVA, MaskingPDSHVA
from .ica import FastICA, GradICA, GradLaplaceICA, NaturalGradICA, NaturalGradLaplaceICA
from .ipsdta import TIPSDTA, BlockDecompositionIPSDTABase, GaussIPSDTA, IPSDTABase
from .overiva import OverGaussIVA, OverIVABase, OverLaplaceIVA
from .pdsbss import PDSBSS, MaskingPDSBSS, PDSBSSBase
from .proxbss import ProxBSSBase

__all__ = ["IterativeMethodBase", "CACGMM", "CACGMMBase", "IPSDTABase", "BlockDecompositionIPSDTABase",
           "GaussIPSDTA", "TIPSDTA", "FDICABase", "GradFDICABase", "GradFDICA", "NaturalGradFDICA",
           "AuxFDICA", "GradLaplaceFDICA", "NaturalGradLaplaceFDICA", "AuxLaplaceFDICA",
           "ProxBSSBase", "PDSBSSBase", "PDSBSS", "MaskingPDSBSS", "MaskingPDSHVA", "HVA", "ADMMBSSBase", "ADMMBSS",
           "MaskingADMMBSS", "MaskingADMMHVA", "GradICA", "NaturalGradICA", "FastICA", "GradLaplaceICA",
           "NaturalGradLaplaceICA", "OverIVABase", "OverLaplaceIVA", "OverGaussIVA", "ConvIVABase",
           "ConvLaplaceIVA", "ConvGaussIVA", "ConvGaussILRMA", "admmbss", "base", "cacgmm", "convilrma",
           "conviva", "fdica", "hva",
           "ica", "ilrma", "ipsdta", "iva", "mnmf", "overiva", "pdsbss", "proxbss"]
