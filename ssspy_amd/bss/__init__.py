from . import base, cacgmm, ilrma, iva, mnmf
from .base import IterativeMethodBase
from .cacgmm import CACGMM, CACGMMBase

__all__ = ["IterativeMethodBase", "CACGMM", "CACGMMBase", "base", "cacgmm", "ilrma", "iva", "mnmf"]
