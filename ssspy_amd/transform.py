"""STFT / ISTFT on the device, with the conventions of ``scipy.signal.stft`` / ``istft`` that the
reference's workflow uses either side of a separator (``window="hann"``, ``boundary="zeros"``,
``padded=True``, one-sided, ``scaling="spectrum"``; tests/package/bss/test_ilrma.py et al.).

    Z = stft(x, n_fft=2048, hop_length=512)          # (n_channels, n_fft // 2 + 1, n_frames)
    Y = GaussILRMA(n_basis=16)(Z)
    y = istft(Y, n_fft=2048, hop_length=512)[..., : x.shape[-1]]

Both take NumPy arrays or device tensors; with ``device_output=True`` the result stays in HBM, so
a separator can consume the spectrogram (``_bind_input`` accepts device tensors) and hand its
output to ``istft`` without the spectrogram crossing PCIe.  ``n_fft``: a power of two <= 65536 or any
length in [2, 32768] (Bluestein; up to 8192 points in LDS, longer transforms on a workspace in HBM);
``window``: an array, or what ``scipy.signal.get_window`` takes for
its periodic windows (a name, or a ``(name, parameter)`` tuple).

``whiten`` and ``pca`` (ssspy/transform/whiten.py, ssspy/transform/pca.py) are here as well: complex
spectrograms go through the covariance pass, the per-bin whitening / PCA filter and ``separate`` on
the device; the real time-domain forms are one small matrix per signal and stay NumPy on the host.
"""

import warnings
from typing import Optional, Union

import numpy as np
import torch

from . import _device as dv
from . import _lib


def _L():
    return _lib.load()


def _cosine_sum(a, n):
    k = 2.0 * np.pi * np.arange(n) / n  # periodic (fftbins=True): the (n + 1)-point symmetric window cut
    w = np.zeros(n)
    for i, c in enumerate(a):
        w += ((-1) ** i) * c * np.cos(i * k)
    return w


def get_window(window, n_fft: int) -> np.ndarray:
    """The periodic (``fftbins=True``) windows of ``scipy.signal.get_window`` that ``scipy.signal.stft``
    accepts by name: the (n_fft,) samples are a host-side table the kernels multiply by.
    ref: the reference's workflow passes ``window="hann"`` (tests/package/bss/test_ilrma.py:95-110)."""
    n = int(n_fft)
    args = ()
    if isinstance(window, tuple):
        window, args = window[0], tuple(window[1:])
    name = str(window).lower()
    m = n + 1  # the symmetric window of n + 1 points, last one dropped
    t = np.arange(n)
    if name in ("hann", "hanning", "han"):
        return _cosine_sum([0.5, 0.5], n)
    if name in ("hamming", "hamm", "ham"):
        return _cosine_sum([0.54, 0.46], n)
    if name in ("blackman", "black", "blk"):
        return _cosine_sum([0.42, 0.50, 0.08], n)
    if name in ("blackmanharris", "blackharr", "bkh"):
        return _cosine_sum([0.35875, 0.48829, 0.14128, 0.01168], n)
    if name in ("nuttall", "nutl", "nut"):
        return _cosine_sum([0.3635819, 0.4891775, 0.1365995, 0.0106411], n)
    if name in ("flattop", "flat", "flt"):
        return _cosine_sum([0.21557895, 0.41663158, 0.277263158, 0.083578947, 0.006947368], n)
    if name in ("general_hamming",):
        (alpha,) = args
        return _cosine_sum([alpha, 1.0 - alpha], n)
    if name in ("general_cosine",):
        (coeffs,) = args
        return _cosine_sum(list(coeffs), n)
    if name in ("boxcar", "box", "ones", "rect", "rectangular"):
        return np.ones(n)
    if name in ("bartlett", "bart", "brt"):
        return 1.0 - np.abs(2.0 * t / (m - 1) - 1.0)
    if name in ("triang", "triangle", "tri"):
        k = np.arange(1, (m + 1) // 2 + 1)
        if m % 2 == 0:
            half = (2 * k - 1.0) / m
            w = np.concatenate([half, half[::-1]])
        else:
            half = 2 * k / (m + 1.0)
            w = np.concatenate([half, half[-2::-1]])
        return w[:n]
    if name in ("cosine", "halfcosine"):
        return np.sin(np.pi / m * (t + 0.5))
    if name in ("bohman", "bman", "bmn"):
        x = np.abs(np.linspace(-1, 1, m)[1:-1])
        w = (1 - x) * np.cos(np.pi * x) + 1.0 / np.pi * np.sin(np.pi * x)
        return np.concatenate([[0.0], w, [0.0]])[:n]
    if name in ("parzen", "parz", "par"):
        k = np.arange(-(m - 1) / 2.0, (m - 1) / 2.0 + 0.5, 1.0)
        na = k[np.abs(k) <= (m - 1) / 4.0]
        nb = k[np.abs(k) > (m - 1) / 4.0]
        wa = 1 - 6 * (np.abs(na) / (m / 2.0)) ** 2 + 6 * (np.abs(na) / (m / 2.0)) ** 3
        wb = 2 * (1 - np.abs(nb) / (m / 2.0)) ** 3
        half = len(nb) // 2
        return np.concatenate([wb[:half], wa, wb[half:]])[:n]
    if name in ("kaiser", "ksr"):
        (beta,) = args
        k = np.arange(m)
        alpha = (m - 1) / 2.0
        return (np.i0(beta * np.sqrt(np.maximum(1 - ((k - alpha) / alpha) ** 2.0, 0.0)))
                / np.i0(beta))[:n]
    if name in ("gaussian", "gauss", "gss"):
        (std,) = args
        k = np.arange(m) - (m - 1.0) / 2.0
        return np.exp(-(k ** 2) / (2.0 * std * std))[:n]
    if name in ("tukey", "tuk"):
        alpha = args[0] if args else 0.5
        if alpha <= 0:
            return np.ones(n)
        if alpha >= 1.0:
            return _cosine_sum([0.5, 0.5], n)
        k = np.arange(m)
        width = int(np.floor(alpha * (m - 1) / 2.0))
        n1, n2, n3 = k[: width + 1], k[width + 1: m - width - 1], k[m - width - 1:]
        w1 = 0.5 * (1 + np.cos(np.pi * (-1 + 2.0 * n1 / alpha / (m - 1))))
        w3 = 0.5 * (1 + np.cos(np.pi * (-2.0 / alpha + 1 + 2.0 * n3 / alpha / (m - 1))))
        return np.concatenate([w1, np.ones(n2.shape), w3])[:n]
    if name in _SCIPY_ONLY_WINDOWS:
        raise NotImplementedError(
            "window {!r} is a scipy.signal window that is not built here; pass "
            "scipy.signal.get_window({!r}, n_fft) as an array instead.".format(name, window))
    raise ValueError("Unknown window type {!r}.".format(window))


# valid scipy.signal.get_window names that have no closed form here (see get_window)
_SCIPY_ONLY_WINDOWS = frozenset([
    "barthann", "brthan", "bth", "lanczos", "sinc", "taylor", "taylorwin", "exponential", "poisson",
    "chebwin", "cheb", "dpss", "general_gaussian", "general gaussian", "general gauss",
    "general_gauss", "ggs", "general_cosine", "general cosine", "general_hamming",
    "general hamming", "kaiser_bessel_derived", "kbd",
])


def _window(window, n_fft: int) -> np.ndarray:
    if isinstance(window, (str, tuple)):
        return np.ascontiguousarray(get_window(window, n_fft), dtype=np.float64)
    w = np.asarray(window, dtype=np.float64)
    if w.shape != (n_fft,):
        raise ValueError("window must have n_fft = {} samples".format(n_fft))
    return w


def _workspace(n_fft, dev):
    nbytes = int(_L().ssspy_stft_workspace_bytes(int(n_fft)))
    return dv.empty((max(nbytes, 16) // 16,), dv.c128, dev) if nbytes else None


def _stream():
    return dv.stream_handle()


# a launch grid is (n_frames, C, 1): HIP takes at most 65535 workgroups along y
_MAX_GRID_Y = 65535


def _on_device(a, dtype, torch_dtype, what, core, real_only):
    """The kernels read `dtype` through a raw pointer: anything else is converted first (a tensor on
    the device, where the cast is plumbing), and a tensor the device cannot read is refused as
    ``_bind_input`` refuses it.  The checks come before the upload or the cast: what is refused has
    touched no device.  `core`: the trailing axes of one signal; the others index the launch grid."""
    is_tensor = isinstance(a, torch.Tensor)
    if is_tensor:
        if not a.is_cuda:
            raise ValueError("a tensor input must be on the HIP device")
        is_complex = a.is_complex()
    else:
        a = np.asarray(a)
        is_complex = np.iscomplexobj(a)
    if real_only and is_complex:
        raise ValueError("{} takes a real signal, got {}".format(what, a.dtype))
    if a.ndim < core:
        raise ValueError("{} takes at least {} axes, got shape {}".format(what, core, tuple(a.shape)))
    C = int(np.prod(a.shape[: a.ndim - core], dtype=np.int64))
    if C > _MAX_GRID_Y:
        raise ValueError("{}: the leading axes hold {} signals, a launch takes at most {}".format(
            what, C, _MAX_GRID_Y))
    if is_tensor:
        return a if a.dtype == torch_dtype else a.to(torch_dtype)
    return dv.to_device(a, dtype=dtype)


def stft(x, n_fft: int, hop_length: Optional[int] = None, window="hann", device_output=False):
    """x (..., n_samples) real -> (..., n_fft // 2 + 1, n_frames) complex128.  ``x``: an array (or
    what ``np.asarray`` takes) or a tensor on the HIP device, of any real dtype."""
    hop = n_fft // 2 if hop_length is None else int(hop_length)
    xd = _on_device(x, np.float64, dv.f64, "stft", 1, real_only=True)
    lead, L = tuple(xd.shape[:-1]), int(xd.shape[-1])
    if n_fft > L:
        # a signal shorter than one window: scipy.signal.stft shrinks nperseg to the signal (with this
        # warning) and keeps noverlap, so the transform has L // 2 + 1 bins
        # (scipy/signal/_spectral_py.py, _triage_segments)
        warnings.warn("nperseg = {0:d} is greater than input length  = {1:d}, using nperseg = {1:d}"
                      .format(n_fft, L))
        noverlap = n_fft - hop
        if noverlap >= L:
            raise ValueError("noverlap must be less than nperseg.")
        n_fft, hop = L, L - noverlap
    w = _window(window, n_fft)
    flat = xd.reshape(1, -1, L).contiguous()
    C = flat.shape[1]
    n_frames = int(_L().ssspy_stft_frames(L, n_fft, hop))
    Z = dv.empty((1, C, n_fft // 2 + 1, n_frames), dv.c128, flat.device)
    wd = dv.to_device(w, dtype=np.float64)
    ws = _workspace(n_fft, flat.device)
    _lib.check(
        _L().ssspy_stft(dv.ptr(flat), dv.ptr(Z), dv.ptr(wd), float(w.sum()), 1, C, L, n_fft,
                        hop, dv.ptr(ws), _stream()),
        "stft",
    )
    Z = Z.reshape(lead + (n_fft // 2 + 1, n_frames))
    return Z if device_output else dv.to_host(Z)


def istft(Z, n_fft: int, hop_length: Optional[int] = None, window="hann", device_output=False):
    """Z (..., n_fft // 2 + 1, n_frames) complex -> (..., n_samples) real (trim to the original
    length yourself, as with SciPy: the forward transform pads to a whole number of hops).  ``Z``: an
    array or a tensor on the HIP device, of any real or complex dtype."""
    hop = n_fft // 2 if hop_length is None else int(hop_length)
    w = _window(window, n_fft)
    Zd = _on_device(Z, np.complex128, dv.c128, "istft", 2, real_only=False)
    lead, F, n_frames = tuple(Zd.shape[:-2]), int(Zd.shape[-2]), int(Zd.shape[-1])
    if F != n_fft // 2 + 1:
        raise ValueError("expected {} bins for n_fft = {}, got {}".format(n_fft // 2 + 1, n_fft, F))
    flat = Zd.reshape(1, -1, F, n_frames).contiguous()
    C = flat.shape[1]
    L = int(_L().ssspy_istft_samples(n_frames, n_fft, hop))
    x = dv.empty((1, C, L), dv.f64, flat.device)
    seg = dv.empty((C * n_frames * n_fft,), dv.f64, flat.device)
    wd = dv.to_device(w, dtype=np.float64)
    ws = _workspace(n_fft, flat.device)
    _lib.check(
        _L().ssspy_istft(dv.ptr(flat), dv.ptr(x), dv.ptr(wd), float(w.sum()), dv.ptr(seg), 1, C,
                         n_frames, n_fft, hop, dv.ptr(ws), _stream()),
        "istft",
    )
    x = x.reshape(lead + (L,))
    return x if device_output else dv.to_host(x)


def _device_rotation(input: np.ndarray, mode: int, what: str) -> np.ndarray:
    """P x per bin with P from the eigen-decomposition of mean_j x x^H; complex (M, F, T) or
    (B, M, F, T).  A covariance the filter kernel cannot decompose raises LinAlgError, where the
    reference returns inf / nan."""
    from . import _ops

    batched = input.ndim == 4
    n_channels = input.shape[1 if batched else 0]
    if not 2 <= n_channels <= _lib.RT_MAX_SOURCES:
        raise NotImplementedError(
            "{} takes 2 to {} channels, got {}.".format(what, _lib.RT_MAX_SOURCES, n_channels))
    X = dv.to_device(input if batched else input[None], dtype=np.complex128)
    B, M, F, T = X.shape
    info = dv.zeros((1,), dv.i32, X.device)
    if mode == _lib.WHITEN:
        out = dv.to_host(_ops.whitened(X, info))
    else:
        C = _ops.weighted_covariance(X).reshape(B, F, M, M)
        out = dv.to_host(_ops.separate(X, _ops.whitening_filter(C, mode, info)))
    _lib.raise_if_singular(int(info.item()), what)
    return out if batched else out[0]


def whiten(input: np.ndarray) -> np.ndarray:
    """Whitening (sphering): z = Lambda^-1/2 V^H x with mean_j x x^H = V Lambda V^H
    (ref: ssspy/transform/whiten.py:4-94).

    Complex (n_channels, n_bins, n_frames) and (batch_size, n_channels, n_bins, n_frames) inputs run
    on the device; real (n_channels, n_samples) and (batch_size, n_channels, n_samples) inputs are
    one n_channels x n_channels problem per signal and stay NumPy on the host.  The eigenvectors
    carry the decomposition's phase (with LAPACK as here, arbitrary): the rows of the complex result
    are defined up to a unit factor per (channel, bin).
    """
    if input.ndim == 2:
        if np.iscomplexobj(input):
            raise ValueError("Real tensor is expected, but given complex tensor.")
        return _host_rotation(input[np.newaxis], scale=True, reverse=False)[0]
    elif input.ndim == 3:
        if np.iscomplexobj(input):
            return _device_rotation(input, _lib.WHITEN, "whiten")
        return _host_rotation(input, scale=True, reverse=False)
    elif input.ndim == 4:
        if np.iscomplexobj(input):
            return _device_rotation(input, _lib.WHITEN, "whiten")
        raise ValueError("Complex tensor is expected, but given real tensor.")
    raise ValueError(
        "The dimension of input is expected 2, 3, or 4, but given {}.".format(input.ndim)
    )


def pca(input: np.ndarray, ascend: bool = True) -> np.ndarray:
    """Principal component analysis: y = V^H x, the first channel the first principal component when
    ``ascend`` (ref: ssspy/transform/pca.py:4-96).  Where it runs: as for ``whiten``."""
    if input.ndim == 2:
        if np.iscomplexobj(input):
            raise ValueError("Real tensor is expected, but given complex tensor.")
        return _host_rotation(input[np.newaxis], scale=False, reverse=bool(ascend))[0]
    elif input.ndim == 3:
        if np.iscomplexobj(input):
            return _device_rotation(input, _lib.PCA_FIRST_COMPONENT_FIRST if ascend else _lib.PCA_FIRST_COMPONENT_LAST,
                                    "pca")
        return _host_rotation(input, scale=False, reverse=bool(ascend))
    elif input.ndim == 4:
        if np.iscomplexobj(input):
            return _device_rotation(input, _lib.PCA_FIRST_COMPONENT_FIRST if ascend else _lib.PCA_FIRST_COMPONENT_LAST,
                                    "pca")
        raise ValueError("Complex tensor is expected, but given real tensor.")
    raise ValueError(
        "The dimension of input is expected 3 or 4, but given {}.".format(input.ndim)
    )


def _host_rotation(x: np.ndarray, scale: bool, reverse: bool) -> np.ndarray:
    """Real time-domain signals (batch_size, n_channels, n_samples) on the host."""
    covariance = np.einsum("bmt,bnt->bmn", x, x) / x.shape[-1]
    lam, V = np.linalg.eigh(covariance)
    if reverse:
        V = V[..., ::-1]
    P = V.transpose(0, 2, 1)
    if scale:
        P = (1 / np.sqrt(lam))[:, :, np.newaxis] * P
    return P @ x
