"""Proximal operators (NumPy in, NumPy out), the reference's ``ssspy.linalg.prox`` (ssspy/linalg/prox.py).

``l1``, ``l21`` and ``neg_log`` are elementwise or group-wise shrinkages and run on the host as in the
reference; passed to :class:`ssspy_amd.bss.pdsbss.PDSBSS` *as these functions* (or as a
``functools.partial`` of them that fixes no ``step_size``) they are recognised by identity and the
separator applies them inside its own kernels.  ``neg_logdet`` needs a singular value decomposition
per matrix and runs on the device (``ssspy_prox_neg_logdet``, csrc/prox_svd.hpp: a one-sided complex
Jacobi on the matrix itself).
"""

import numpy as np

from .. import _device as dv
from .. import _lib
from .._device import ptr

__all__ = ["l1", "l21", "neg_log", "neg_logdet"]


def l1(x, step_size: float = 1) -> np.ndarray:
    """Proximal operator of the L1 norm (ref: ssspy/linalg/prox.py:6-12)."""
    norm = np.abs(x)
    # (the reference's guard against a division by zero: a norm below step_size shrinks to 0 anyway)
    norm = np.where(norm < step_size, step_size, norm)
    return np.maximum(1 - step_size / norm, 0) * x


def l21(x: np.ndarray, step_size: float = 1, axis1: int = -2, axis2: int = -1):
    """Proximal operator of the L21 norm: the group norm is taken over ``axis2`` only, ``axis1`` is
    accepted and unused, as in the reference (ref: ssspy/linalg/prox.py:15-33)."""
    norm = np.linalg.norm(x, axis=axis2, keepdims=True)
    norm = np.where(norm < step_size, step_size, norm)
    return np.maximum(1 - step_size / norm, 0) * x


def neg_log(x: np.ndarray, step_size: float = 1):
    """Proximal operator of -log: ``(x + sqrt(x^2 + 4 step_size)) / 2`` for ``x >= 0``
    (ref: ssspy/linalg/prox.py:36-59)."""
    assert np.all(x >= 0)
    return (x + np.sqrt(x**2 + 4 * step_size)) / 2


def neg_logdet(X: np.ndarray, step_size=1):
    """Proximal operator of the negative log-determinant, ``U diag(neg_log(sigma)) V^H`` of
    ``X = U diag(sigma) V^H`` (ref: ssspy/linalg/prox.py:62-91), for batches of N x N matrices,
    N <= 16; leading axes are batch axes.  The result is a function of the matrix: it does not depend
    on the phases or the order of the singular vectors.  Where a singular value is exactly zero it is
    not determined (the reference returns what LAPACK picks); the result is then finite and has the
    singular values ``neg_log(sigma)``."""
    X = np.asarray(X)
    if X.ndim < 2 or X.shape[-1] != X.shape[-2]:
        raise ValueError("neg_logdet takes square matrices, got shape {}.".format(X.shape))
    lead, N = X.shape[:-2], X.shape[-1]
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if n == 0:
        return np.zeros(X.shape, dtype=np.complex128 if np.iscomplexobj(X) else np.float64)
    dX = dv.to_device(np.ascontiguousarray(X.reshape(n, N, N), dtype=np.complex128))
    out = dv.empty((n, N, N), dv.c128, dX.device)
    _lib.check(_lib.load().ssspy_prox_neg_logdet(ptr(dX), ptr(out), n, N, float(step_size),
                                                 dv.stream_handle()), "neg_logdet")
    res = dv.to_host(out).reshape(lead + (N, N))
    return res if np.iscomplexobj(X) else np.ascontiguousarray(res.real)
