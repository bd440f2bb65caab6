from . import base, cacgmm, ilrma, ipsdta, iva, mnmf
from .base import IterativeMethodBase
from .cacgmm import CACGMM, CACGMMBase
from .ipsdta import TIPSDTA, BlockDecompositionIPSDTABase, GaussIPSDTA, IPSDTABase

__all__ = ["IterativeMethodBase", "CACGMM", "CACGMMBase", "IPSDTABase", "BlockDecompositionIPSDTABase",
           "GaussIPSDTA", "TIPSDTA", "base", "cacgmm", "ilrma", "ipsdta", "iva", "mnmf"]
