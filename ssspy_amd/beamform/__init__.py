"""Mask-based beamformers behind the mask estimators: MVDR, GEV, the multichannel Wiener filter and
the convolutional beamformer (WPD)."""

from .mask import GEV, MVDR, MWF, MaskBeamformerBase, masked_covariance
from .wpd import WPD

__all__ = ["MaskBeamformerBase", "MVDR", "GEV", "MWF", "WPD", "masked_covariance"]
