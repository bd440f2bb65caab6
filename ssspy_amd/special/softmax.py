"""softmax and logsumexp: NumPy arrays on the host, torch device tensors on the device
(csrc/special.hip), the convention of ``ssspy_amd.algorithm.permutation_alignment``.

Counterparts of ``ssspy.special.softmax`` and ``ssspy.special.logsumexp``
(ssspy/special/softmax.py:4-36, logsumexp.py:4-40).
"""

import numpy as np

__all__ = ["softmax", "logsumexp"]


def _is_device_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def _device_axis(X, axis, what):
    """The reduced axis of a device tensor the kernels take, or NotImplementedError."""
    import torch

    if isinstance(axis, (tuple, list)):
        raise NotImplementedError(
            "{} of a device tensor reduces one axis, got axis={!r} (convert to NumPy for the host "
            "form)".format(what, axis))
    if axis is None:
        raise NotImplementedError(
            "{} of a device tensor needs an axis, got axis=None (convert to NumPy for the host "
            "form)".format(what))
    if not X.is_cuda or X.dtype != torch.float64 or X.ndim == 0:
        raise NotImplementedError(
            "{} on the device takes a float64 tensor on a HIP device, got {} on {} (convert to NumPy "
            "for the host form)".format(what, X.dtype, X.device))
    axis = int(axis)
    if not -X.ndim <= axis < X.ndim:
        raise ValueError("axis {} is out of bounds for a tensor of dimension {}".format(axis, X.ndim))
    if X.shape[axis] == 0:
        raise ValueError("{} over an axis of length 0".format(what))
    return axis % X.ndim


def softmax(X, axis=None):
    """exp(X - max) / sum exp(X - max) over ``axis`` (an int, a tuple of ints, or None for all axes).

    NumPy input is evaluated on the host and keeps its dtype.  A float64 torch tensor on the device
    is evaluated there over one axis, first, middle or last (walked by its stride, nothing is
    transposed), every sum in a fixed order, and a tensor comes back; ``axis=None``, a tuple axis or
    another dtype raise ``NotImplementedError`` for a device tensor.
    """
    if _is_device_tensor(X):
        from .. import _ops

        axis = _device_axis(X, axis, "softmax")
        return _ops.softmax_dev(X.contiguous(), axis)
    shifted = X - np.max(X, axis=axis, keepdims=True)
    weight = np.exp(shifted)
    return weight / np.sum(weight, axis=axis, keepdims=True)


def logsumexp(X, axis=None, keepdims=False):
    """log sum exp(X) over ``axis`` (an int, a tuple of ints, or None for all axes), the maximum
    taken out of the exponentials.

    NumPy input is evaluated on the host and keeps its dtype.  A float64 torch tensor on the device
    is evaluated there over one axis (see ``softmax``); ``axis=None``, a tuple axis or another dtype
    raise ``NotImplementedError`` for a device tensor.
    """
    if _is_device_tensor(X):
        from .. import _ops

        axis = _device_axis(X, axis, "logsumexp")
        out = _ops.logsumexp_dev(X.contiguous(), axis)
        return out.unsqueeze(axis) if keepdims else out
    top = np.max(X, axis=axis, keepdims=True)
    total = np.sum(np.exp(X - top), axis=axis, keepdims=True)
    out = np.log(total) + top
    return out if keepdims else np.squeeze(out, axis=axis)
