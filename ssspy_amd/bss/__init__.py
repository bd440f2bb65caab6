from . import base, cacgmm, fdica, ilrma, ipsdta, iva, mnmf
from .base import IterativeMethodBase
from .cacgmm import CACGMM, CACGMMBase
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
from .ipsdta import TIPSDTA, BlockDecompositionIPSDTABase, GaussIPSDTA, IPSDTABase

__all__ = ["IterativeMethodBase", "CACGMM", "CACGMMBase", "IPSDTABase", "BlockDecompositionIPSDTABase",
           "GaussIPSDTA", "TIPSDTA", "FDICABase", "GradFDICABase", "GradFDICA", "NaturalGradFDICA",
           "AuxFDICA", "GradLaplaceFDICA", "NaturalGradLaplaceFDICA", "AuxLaplaceFDICA", "base",
           "cacgmm", "fdica", "ilrma", "ipsdta", "iva", "mnmf"]
