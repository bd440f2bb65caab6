"""NumPy restatement of ``whiten`` / ``pca`` and of the fixed-point IVA classes of the reference
(ssspy/transform/whiten.py, ssspy/transform/pca.py, ssspy/bss/iva.py:409-550, :991-1400), written
from their equations: whitening z = Lambda^-1/2 V^H x, the FastIVA update with its two means, the
FasterIVA principal eigenvectors, the polar factor u v^H.

A test helper: the product never imports it.  Single mixtures only, (n_channels, n_bins, n_frames).

Gauge.  The eigenvectors of ``numpy.linalg.eigh`` carry LAPACK's phase; another choice multiplies
the whitened mixture by a diagonal unitary D per bin (Z -> D Z, W -> Phi W D^H, Y -> Phi Y).
``gauge_like`` (a whitened mixture of the same input from elsewhere) makes a run take that mixture's
phases, so that a run can be compared with one made under another decomposition.
"""

import functools

import numpy as np

from oracle import spatial as sp

EPS = 1e-10


def max_flooring(x, eps=EPS):
    return np.maximum(x, eps)


def add_flooring(x, eps=EPS):
    return x + eps


def identity(x):
    return x


def covariance(X):
    """mean_j x x^H per bin, (n_bins, n_channels, n_channels)."""
    return np.einsum("mft,nft->fmn", X, X.conj()) / X.shape[-1]


def whitening_filter(X):
    lam, V = np.linalg.eigh(covariance(X))
    return (1 / np.sqrt(lam))[:, :, np.newaxis] * V.transpose(0, 2, 1).conj()


def gauge_between(Z, Z_like):
    """D (n_bins, n_channels) of unit modulus with D Z ~ Z_like row by row."""
    inner = np.sum(Z_like * Z.conj(), axis=-1).T
    return inner / np.abs(inner)


def whiten(X, gauge_like=None):
    """Complex (n_channels, n_bins, n_frames), or real (n_channels, n_samples)."""
    if not np.iscomplexobj(X):
        lam, V = np.linalg.eigh(X @ X.T / X.shape[-1])
        return ((1 / np.sqrt(lam))[:, np.newaxis] * V.T) @ X
    Z = sp.separate(X, whitening_filter(X))
    if gauge_like is not None:
        Z = gauge_between(Z, gauge_like).T[:, :, np.newaxis] * Z
    return Z


def pca(X, ascend=True):
    if not np.iscomplexobj(X):
        _, V = np.linalg.eigh(X @ X.T / X.shape[-1])
        return (V[:, ::-1] if ascend else V).T @ X
    _, V = np.linalg.eigh(covariance(X))
    if ascend:
        V = V[..., ::-1]
    return sp.separate(X, V.transpose(0, 2, 1).conj())


def polar_unitary(W):
    """u v^H of W = u s v^H: (W W^H)^-1/2 W."""
    u, _, vh = np.linalg.svd(W)
    return u @ vh


class FastIVABase:
    name = "FastIVA"

    def __init__(self, contrast_fn=None, d_contrast_fn=None,
                 flooring_fn=functools.partial(max_flooring, eps=EPS), callbacks=None,
                 scale_restoration=True, record_loss=True, reference_id=0, gauge_like=None):
        if contrast_fn is None:
            raise ValueError("Specify contrast function.")
        if d_contrast_fn is None:
            raise ValueError("Specify derivative of contrast function.")
        self.contrast_fn, self.d_contrast_fn = contrast_fn, d_contrast_fn
        self.flooring_fn = identity if flooring_fn is None else flooring_fn
        self.callbacks = [callbacks] if callable(callbacks) else callbacks
        self.scale_restoration, self.record_loss = scale_restoration, record_loss
        self.reference_id = reference_id
        self.gauge_like = gauge_like
        self.loss = [] if record_loss else None

    def _reset(self, **kwargs):
        for key, value in kwargs.items():
            setattr(self, key, value)
        N, F, T = self.input.shape
        self.n_sources, self.n_channels, self.n_bins, self.n_frames = N, N, F, T
        if not hasattr(self, "demix_filter"):
            self.demix_filter = np.tile(np.eye(N, dtype=np.complex128), (F, 1, 1))
        else:
            self.demix_filter = self.demix_filter.copy()
        self.whitened_input = whiten(self.input, self.gauge_like)
        self.output = sp.separate(self.whitened_input, self.demix_filter)

    def _after_step(self):
        if self.record_loss:
            self.loss.append(self.compute_loss())
        for hook in self.callbacks or ():
            hook(self)

    def __call__(self, input, n_iter=100, initial_call=True, **kwargs):
        self.input = input.copy()
        self._reset(**kwargs)
        if initial_call:
            self._after_step()
        for _ in range(n_iter):
            self.update_once()
            self._after_step()
        if self.scale_restoration:
            self.restore_scale()
        self.output = sp.separate(self.whitened_input, self.demix_filter)
        return self.output

    def _weights(self):
        Y = sp.separate(self.whitened_input, self.demix_filter)
        r = np.sqrt(np.sum(np.abs(Y) ** 2, axis=1))  # (n_sources, n_frames)
        return Y, r, self.d_contrast_fn(r) / self.flooring_fn(2 * r)

    def compute_loss(self):
        Y = sp.separate(self.whitened_input, self.demix_filter)
        return np.sum(np.mean(self.contrast_fn(Y), axis=1), axis=0).item()

    def restore_scale(self):
        kind = self.scale_restoration
        if type(kind) is bool:
            kind = "projection_back"
        X, Z, W = self.input, self.whitened_input, self.demix_filter
        if kind == "projection_back":
            # scaled against the unwhitened input, refitted on the whitened one (:533-550)
            Y = sp.projection_back_output(sp.separate(Z, W), X, reference_id=self.reference_id)
            self.output, self.demix_filter = Y, sp.demix_from_output(Y, Z)
        elif kind == "minimal_distortion_principle":
            # the reference inherits IVABase's method here (:269-281), whose ``separate`` call whitens:
            # the estimate W z is scaled against x, but the filters are refitted on the UNWHITENED
            # input and then applied to the whitened one (:1132-1134)
            Y = sp.minimal_distortion_output(sp.separate(Z, W), X, reference_id=self.reference_id)
            self.output, self.demix_filter = Y, sp.demix_from_output(Y, X)
        else:
            raise ValueError("{} is not supported for scale restoration.".format(kind))


class FastIVA(FastIVABase):
    def __init__(self, contrast_fn=None, d_contrast_fn=None, dd_contrast_fn=None, **kwargs):
        super().__init__(contrast_fn=contrast_fn, d_contrast_fn=d_contrast_fn, **kwargs)
        if dd_contrast_fn is None:
            raise ValueError("Specify second order derivative of contrast function.")
        self.dd_contrast_fn = dd_contrast_fn

    def update_once(self):
        Z, W = self.whitened_input, self.demix_filter
        Y, r, phi = self._weights()
        psi = (2 * phi - self.dd_contrast_fn(r)) / self.flooring_fn(2 * r)
        T = self.n_frames
        a = np.sum(phi, axis=-1) / T                                  # (n,)
        b = np.einsum("nt,nft->fn", psi, np.abs(Y) ** 2) / T           # (f, n)
        c = np.einsum("nt,nft,mft->fnm", phi, Y.conj(), Z) / T         # (f, n, m)
        # w_in of the equations is the conjugate of row n of W_i
        W = (a[np.newaxis, :, np.newaxis] - b[:, :, np.newaxis]) * W - c.conj()
        self.demix_filter = polar_unitary(W)


class FasterIVA(FastIVABase):
    name = "FasterIVA"

    def update_once(self):
        Z = self.whitened_input
        _, _, phi = self._weights()
        U = np.einsum("nt,aft,bft->fnab", phi, Z, Z.conj()) / self.n_frames
        _, V = np.linalg.eigh(U)
        self.demix_filter = polar_unitary(V[..., -1].conj())

    def eigen_gaps(self):
        """(lam_max - lam_2) / lam_max of every U_in of the current state, (n_bins, n_sources)."""
        Z = self.whitened_input
        _, _, phi = self._weights()
        U = np.einsum("nt,aft,bft->fnab", phi, Z, Z.conj()) / self.n_frames
        lam = np.linalg.eigvalsh(U)
        return (lam[..., -1] - lam[..., -2]) / lam[..., -1]


CLASSES = {"FastIVA": FastIVA, "FasterIVA": FasterIVA}
