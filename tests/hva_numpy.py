"""NumPy restatement of the mask of harmonic vector analysis and of MaskingPDSHVA / HVA on top of
tests/pdsbss_numpy.py, written for this project: the oracle of the GPU tests on shapes no fixture
has.  tests/test_golden_hva.py pins it against the fixtures generated from the reference.

The transform along the bins is written as the DCT-I it is,
``D(c)_k = c_0 + (-1)^k c_{F-1} + 2 sum_{0<j<F-1} c_j cos(pi j k / (F - 1))``, as a matrix product, in
any floating type: ``varrho(..., dtype=np.longdouble)`` is the extended evaluation the kernel is
checked against element by element.
"""

import functools
import math

import numpy as np

import pdsbss_numpy as pn

EPS = 1e-10


def identity(x):
    return x


def max_flooring(x, eps=EPS):
    return np.maximum(x, eps)


def add_flooring(x, eps=EPS):
    return x + eps


@functools.lru_cache(maxsize=None)
def dct1_matrix(F, dtype=np.float64):
    """(F, F): row k holds the weights of c_0 .. c_{F-1} in D(c)_k.  The table of 2 (F - 1) cosines is
    indexed by (j k) mod 2 (F - 1) in integers."""
    n2 = 2 * (F - 1)
    pi = 4 * np.arctan(dtype(1))
    table = np.cos(pi * np.arange(n2).astype(dtype) / dtype(F - 1))
    k = np.arange(F)
    weight = np.full(F, 2, dtype=dtype)
    weight[0] = weight[-1] = 1
    return table[np.outer(k, k) % n2] * weight


def dct1(c):
    """D along axis -2 of (..., F, T)."""
    return np.einsum("kj,...jt->...kt", dct1_matrix(c.shape[-2], c.dtype.type), c)


def cepstrum_chain(Z, flooring_fn=None, mask_iter=1, dtype=np.float64):
    """(varrho, rho, sigma nu) of Z (..., F, T) in ``dtype``; pi is the double the reference
    multiplies by."""
    ctype = np.clongdouble if dtype is np.longdouble else np.complex128
    a = np.abs(np.asarray(Z).astype(ctype))
    if flooring_fn is not None:
        a = flooring_fn(a)
    F = a.shape[-2]
    if F < 2:
        raise ValueError("Invalid number of FFT data points (0) specified.")
    with np.errstate(divide="ignore", invalid="ignore"):
        zeta = np.log(a)
        mean = zeta.mean(axis=-2, keepdims=True)
        rho = zeta - mean
        nu = dct1(rho) / dtype(2 * (F - 1))
        sigma = np.minimum(1, nu)
        for _ in range(mask_iter):
            sigma = (1 - np.cos(dtype(math.pi) * sigma)) / 2
        product = sigma * nu
        return dct1(product) + mean, rho, product


def varrho(Z, flooring_fn=None, mask_iter=1, dtype=np.float64):
    return cepstrum_chain(Z, flooring_fn, mask_iter, dtype)[0]


def mask_of(varrho, attenuation):
    """The reference's expression: (v / sum_n v) ** attenuation, v = exp(2 varrho); sources on
    axis -3."""
    v = np.exp(2 * varrho)
    return (v / v.sum(axis=-3, keepdims=True)) ** attenuation


def stable_mask_of(varrho, attenuation):
    """The same with the maximum over sources subtracted: no overflow."""
    d = varrho - varrho.max(axis=-3, keepdims=True)
    return np.exp(2 * attenuation * d) / np.exp(2 * d).sum(axis=-3, keepdims=True) ** attenuation


class MaskingPDSHVA(pn.MaskingPDSBSS):
    _repr_name = "MaskingPDSHVA"

    def __init__(self, mu1=1, mu2=1, alpha=None, relaxation=1, attenuation=None, mask_iter=1,
                 flooring_fn=functools.partial(max_flooring, eps=EPS), callbacks=None,
                 scale_restoration=True, record_loss=None, reference_id=0):
        super().__init__(mu1=mu1, mu2=mu2, alpha=alpha, relaxation=relaxation, penalty_fn=None,
                         mask_fn=self._mask, callbacks=callbacks,
                         scale_restoration=scale_restoration, record_loss=record_loss,
                         reference_id=reference_id)
        self.attenuation, self.mask_iter = attenuation, mask_iter
        self.flooring_fn = identity if flooring_fn is None else flooring_fn

    def _mask(self, y):
        if self.attenuation is None:
            self.attenuation = 1 / y.shape[0]
        return mask_of(varrho(y, self.flooring_fn, self.mask_iter), self.attenuation)

    def __repr__(self):
        s = "{}(mu1={}, mu2={}, relaxation={}".format(self._repr_name, self.mu1, self.mu2,
                                                     self.relaxation)
        if self.attenuation is not None:
            s += ", attenuation={}".format(self.attenuation)
        s += ", mask_iter={}, scale_restoration={}, record_loss={}".format(
            self.mask_iter, self.scale_restoration, self.record_loss)
        if self.scale_restoration:
            s += ", reference_id={}".format(self.reference_id)
        return s + ")"


class HVA(MaskingPDSHVA):
    _repr_name = "HVA"


CLASSES = {"MaskingPDSHVA": MaskingPDSHVA, "HVA": HVA}
