"""The extended-precision STFT / ISTFT reference (tests/stft_reference.py) checked without a GPU:
it is the operation ``scipy.signal`` computes, its bars are attainable by plain float64 NumPy (the
same formulas in float64, and ``np.fft`` plus a NumPy overlap-add), and they are not vacuous: the
float64 NumPy analogue of a subtly wrong kernel lands outside them.

Largest observed error / bar, over the shapes of SHAPES (measured with this file, x86-64, NumPy's
pocketfft):

    route        float64 formulas   np.fft      scipy.signal
    direct       0.095              0.053       0.053
    Bluestein    0.0067             0.0065      0.0065
    inverse      0.046              0.046       0.046

(np.fft has no chirp-z route: its row for the lengths that the kernels send through Bluestein shows
that the bar of that route is attainable; `bluestein_f64` below, the float64 NumPy analogue of the
kernels' chirp-z route, gives 0.0018 at n = 8191, and 4.8 once the chirp drops its integer reduction.)

On the MI355X (gfx950), over every case of tests/test_gpu_stft_elementwise.py, the kernels gave:
direct 0.11 (n = 2), Bluestein in LDS 0.014 (n = 3), global workspace 0.0010, inverse 0.076 (n = 2),
round trip 0.0026.
"""

import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stft_reference as sr  # noqa: E402

LD = sr.LD

# (n_fft, hop, L, window): direct and Bluestein lengths, a hop that does not divide n, hop == 1-like
# many frames, padding 0 and hop - 1, a length beyond 1024 (64 bins / samples)
SHAPES = [
    (2, 1, 9, "boxcar"),
    (5, 2, 23, "boxcar"),
    (64, 16, 300, "hann"),
    (100, 33, 401, ("kaiser", 8.6)),
    (255, 64, 700, "hann"),
    (1024, 512, 3072, "hann"),
    (4097, 1024, 9000, "hann"),
]


def ratio(err, bar):
    """max err / bar; an error where the bar is exactly zero counts as infinite."""
    err = np.asarray(err, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def _window(window, n):
    import scipy.signal as ss

    return ss.get_window(window, n)


def overlap_add_f64(seg, w, n, hop, k_lo_shift=0):
    """NumPy float64 overlap-add of seg (..., J, n) as the kernel states it: sample s sums the frames
    k_lo .. k_hi that cover p = s + n // 2, divided by the same frames' window^2 (where > 1e-10).
    k_lo_shift = 1 is the kernel with a k_lo that is one too high."""
    J = seg.shape[-2]
    L_out = sr.istft_samples(J, n, hop)
    p = np.arange(L_out) + n // 2
    k_lo = np.maximum(0, -(-(p - n + 1) // hop)) + k_lo_shift  # smallest k with k hop + n > p
    acc = np.zeros(seg.shape[:-2] + (L_out,))
    norm = np.zeros(L_out)
    for j in range(J):
        t = p - j * hop
        sel = np.nonzero((t >= 0) & (t < n) & (j >= k_lo))[0]
        acc[..., sel] += seg[..., j, t[sel]]
        norm[sel] += w[t[sel]] ** 2
    return acc / np.where(norm > sr.NORM_THRESHOLD, norm, 1.0)


def bluestein_f64(v, n, sign, reduce=True):
    """The kernels' chirp-z route in float64 NumPy: v (..., n) -> its DFT with exponent sign `sign`.
    reduce=False drops the integer reduction of t^2 mod 2n in the chirp."""
    m = sr.bluestein_len(n)
    t = np.arange(n)
    r = ((t * t) % (2 * n) if reduce else t * t).astype(np.float64)
    c = np.exp(sign * 1j * np.pi * (r / n))
    b = np.zeros(m, np.complex128)
    b[:n] = np.conj(c)
    b[m - n + 1:] = np.conj(c[1:][::-1])
    a = np.zeros(v.shape[:-1] + (m,), np.complex128)
    a[..., :n] = v * c
    return np.fft.ifft(np.fft.fft(a, axis=-1) * np.fft.fft(b), axis=-1)[..., :n] * c


@pytest.mark.parametrize("n,hop,L,window", SHAPES)
def test_reference_is_scipys_operation_and_float64_meets_the_bars(n, hop, L, window):
    import scipy.signal as ss

    w = _window(window, n)
    x = sr.signal(n + hop, 4, L, n, hop)
    bins = sr.check_bins(n)
    starts, J = sr.frames(L, n, hop)
    Z, bar = sr.stft(x, w, n, hop, bins)
    assert Z.dtype == np.clongdouble and bar.dtype == np.float64 and Z.shape == (4, len(bins), J)
    assert (bar[1] == 0).all() and (Z[1] == 0).all()  # the zero channel

    _, _, Zs = ss.stft(x, window=w, nperseg=n, noverlap=n - hop)
    assert Zs.shape == (4, n // 2 + 1, J)
    Z64, _ = sr.stft(x, w, n, hop, bins, dtype=np.float64)
    Zf = np.swapaxes(np.fft.rfft(sr.segments(x, n, hop) * w, axis=-1), -1, -2)[:, bins] / w.sum()
    r = {"scipy": ratio(np.abs(Zs[:, bins] - Z), bar), "float64": ratio(np.abs(Z64 - Z), bar),
         "np.fft": ratio(np.abs(Zf - Z), bar)}
    print("forward n={} {}".format(n, r))
    assert max(r.values()) <= 1.0

    Zi = sr.spectrogram(n, 3, n, J)
    samples = sr.check_samples(sr.istft_samples(J, n, hop), n)
    xr, xbar, norm = sr.istft(Zi, w, n, hop, samples)
    sr.assert_norm_clear_of_threshold(norm)
    assert (xbar[1] == 0).all() and (xr[1] == 0).all()
    _, xs = ss.istft(Zi, window=w, nperseg=n, noverlap=n - hop)
    assert xs.shape[-1] == sr.istft_samples(J, n, hop)
    x64, _, _ = sr.istft(Zi, w, n, hop, samples, dtype=np.float64)
    seg = np.fft.irfft(np.swapaxes(Zi, -1, -2), n=n, axis=-1) * (w * w.sum())
    xf = overlap_add_f64(seg, w, n, hop)[:, samples]
    r = {"scipy": ratio(np.abs(xs[:, samples] - xr), xbar), "float64": ratio(np.abs(x64 - xr), xbar),
         "np.fft": ratio(np.abs(xf - xr), xbar)}
    print("inverse n={} {}".format(n, r))
    assert max(r.values()) <= 1.0


def test_frames_follow_scipy_at_the_padding_edges():
    import scipy.signal as ss

    for n, hop in [(2, 1), (5, 2), (64, 16), (64, 64), (100, 33), (127, 32)]:
        for L in range(n, n + 2 * hop + 2):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                _, _, Zs = ss.stft(np.ones(L), window="boxcar", nperseg=n, noverlap=n - hop)
            starts, J = sr.frames(L, n, hop)
            assert J == Zs.shape[-1], (n, hop, L)
            assert starts[0] == -(n // 2) and starts[-1] + n >= L + n // 2


def test_both_sides_of_the_norm_threshold_are_taken_with_hann_and_hop_equal_to_n():
    for n in (64, 4096):
        w = _window("hann", n)
        Zi = sr.spectrogram(n, 2, n, 3)
        samples = np.arange(sr.istft_samples(3, n, n)) if n == 64 else np.concatenate(
            [np.arange(n // 2 - 8, n // 2 + 9), np.arange(3 * n // 2 - 8, 3 * n // 2 + 9)])
        xr, xbar, norm = sr.istft(Zi, w, n, n, samples)
        sr.assert_norm_clear_of_threshold(norm)
        small = np.asarray(norm <= sr.NORM_THRESHOLD)
        assert small.any() and not small.all()
        x64, _, _ = sr.istft(Zi, w, n, n, samples, dtype=np.float64)
        assert ratio(np.abs(x64 - xr), xbar) <= 1.0


def test_bars_are_not_vacuous():
    """A kernel that is subtly wrong lands outside: the float64 NumPy analogue of (1) a chirp that
    drops the integer reduction of t^2, (2) an overlap-add whose k_lo is one too high."""
    n, hop = 8191, 8191
    F = n // 2 + 1
    t = np.arange(n)
    x = np.cos(2 * np.pi * (((F - 2) * t) % n) / n)[None] + 1e-3 * np.random.default_rng(0) \
        .standard_normal((1, n))
    w = np.ones(n)
    bins = sr.check_bins(n)
    Z, bar = sr.stft(x, w, n, hop, bins)
    seg = (sr.segments(x, n, hop) * w).astype(np.complex128)
    good = np.swapaxes(bluestein_f64(seg, n, -1.0), -1, -2)[:, bins] / w.sum()
    bad = np.swapaxes(bluestein_f64(seg, n, -1.0, reduce=False), -1, -2)[:, bins] / w.sum()
    r_good, r_bad = ratio(np.abs(good - Z), bar), ratio(np.abs(bad - Z), bar)
    print("chirp: analogue {} without the reduction {}".format(r_good, r_bad))
    assert r_good <= 1.0 < r_bad

    n, hop = 64, 16
    w = _window("hann", n)
    Zi = sr.spectrogram(5, 3, n, 9)
    xr, xbar, _ = sr.istft(Zi, w, n, hop)
    seg = np.fft.irfft(np.swapaxes(Zi, -1, -2), n=n, axis=-1) * (w * w.sum())
    r_good = ratio(np.abs(overlap_add_f64(seg, w, n, hop) - xr), xbar)
    r_bad = ratio(np.abs(overlap_add_f64(seg, w, n, hop, k_lo_shift=1) - xr), xbar)
    print("overlap-add: analogue {} with k_lo + 1 {}".format(r_good, r_bad))
    assert r_good <= 1.0 < r_bad


def test_pi_as_a_python_float_would_spoil_the_reference():
    """The table's far end is 2 pi (n - 1) / n: a float64 pi there is off by several u of phase."""
    assert abs(LD(np.pi) - sr._pi(LD)) * 2 > 2 * sr.U
    assert sr._pi(np.float64) == np.pi


def test_inputs_that_no_kernel_may_see_raise_before_any_launch():
    """These end before the library is loaded or a device is touched: they pass without a GPU."""
    import torch

    from ssspy_amd.transform import istft, stft

    with pytest.raises(ValueError):
        stft(np.zeros((2, 100), np.complex64), n_fft=16)
    with pytest.raises(ValueError, match="HIP device"):
        stft(torch.zeros(2, 100, dtype=torch.float64), n_fft=16)
    with pytest.raises(ValueError, match="HIP device"):
        istft(torch.zeros(2, 9, 5, dtype=torch.complex128), n_fft=16)
    with pytest.raises(ValueError):
        stft(np.zeros((65536, 8)), n_fft=4)
    with pytest.raises(ValueError):
        istft(np.zeros((65536, 3, 2), np.complex128), n_fft=4)
