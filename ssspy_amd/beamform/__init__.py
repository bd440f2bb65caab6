"""Mask-based beamformers behind the mask estimators: MVDR, GEV and the multichannel Wiener filter."""

from .mask import GEV, MVDR, MWF, MaskBeamformerBase, masked_covariance

__all__ = ["MaskBeamformerBase", "MVDR", "GEV", "MWF", "masked_covariance"]
