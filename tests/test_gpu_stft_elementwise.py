"""STFT / ISTFT (ssspy_amd/csrc/stft_kernels.hip, ssspy_amd/transform.py) per frame, bin and sample
against the extended-precision restatement of tests/stft_reference.py: every comparison is
``|got - ref| <= bar`` elementwise with the per-segment bars derived there, on a signal whose
neighbouring frames differ by up to 12 decades, at the kernels' route and block boundaries.

Largest observed error / bar on the MI355X (gfx950), per route, over every case of this module:

    direct radix-2 in LDS (n = 2 .. 8192)        0.11  (n = 2)
    Bluestein in LDS (n = 3 .. 4095)             0.014 (n = 3)
    global workspace (n = 4097, 16384)           0.0010
    inverse, per sample (all routes)             0.076 (n = 2)
    round trip                                   0.0026

Each check prints its figure (``RATIO <route> ...``) before it asserts.
"""

import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stft_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu

DIRECT = [2, 4, 64, 512, 1024, 8192]
BLUESTEIN = [3, 5, 6, 100, 127, 129, 255, 257, 2047, 2049, 4095]
GLOBAL = [4097, 16384]
ALL_N = DIRECT + BLUESTEIN + GLOBAL
ARRAY = "array"  # a window given as samples, with negative and zero ones


def route(n):
    return "global" if n in GLOBAL else "direct" if n in DIRECT else "bluestein"


def window_samples(window, n):
    """The float64 samples the kernels multiply by: an input of the comparison, not under test here
    (tests/test_host_logic.py holds the named windows against scipy.signal.get_window)."""
    from ssspy_amd.transform import get_window

    if isinstance(window, str) and window == ARRAY:
        w = np.random.default_rng(n).standard_normal(n) + 0.5
        w[:: max(2, n // 7)] = 0.0
        if n > 2:
            w[1] = -abs(w[1]) - 0.1
        w[-1] = 1.0 + abs(w[-1])  # (keeps sum(w) away from zero at n = 2)
        return w
    return np.asarray(get_window(window, n), dtype=np.float64)


def ratio(err, bar):
    err = np.asarray(err, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def lengths(n, hop):
    """(L0, L1): the smallest signal of at least two windows that needs no padding to a whole number
    of hops, and the one a sample longer, which needs hop - 1."""
    L0 = 2 * n
    while (L0 + 2 * (n // 2) - n) % hop:
        L0 += 1
    return L0, L0 + 1


def check_forward(x, n, hop, window, hop_arg="same", tag=""):
    from ssspy_amd.transform import stft

    w = window_samples(window, n)
    arg = w if isinstance(window, str) and window == ARRAY else window
    Z = stft(x, n_fft=n, hop_length=hop if hop_arg == "same" else hop_arg, window=arg)
    bins = sr.check_bins(n, seed=n)
    Zr, bar = sr.stft(x, w, n, hop, bins)
    assert Z.dtype == np.complex128
    assert Z.shape == x.shape[:-1] + (n // 2 + 1, sr.frames(x.shape[-1], n, hop)[1])
    err = np.abs(Z[..., bins, :] - Zr)
    print("RATIO {} forward n={} hop={} L={} {}{}: {:.4f}".format(
        route(n), n, hop, x.shape[-1], window, tag, ratio(err, bar)))
    assert np.isfinite(Z).all()
    assert (err <= bar).all()
    return Z


def check_inverse(Z, n, hop, window, extra_samples=(), tag=""):
    from ssspy_amd.transform import istft

    w = window_samples(window, n)
    arg = w if isinstance(window, str) and window == ARRAY else window
    x = istft(Z, n_fft=n, hop_length=hop, window=arg)
    L_out = sr.istft_samples(Z.shape[-1], n, hop)
    assert x.dtype == np.float64 and x.shape == Z.shape[:-2] + (L_out,)
    samples = np.union1d(sr.check_samples(L_out, n, seed=n), np.asarray(extra_samples, dtype=np.int64))
    xr, bar, norm = sr.istft(Z, w, n, hop, samples)
    sr.assert_norm_clear_of_threshold(norm)
    err = np.abs(x[..., samples] - xr)
    print("RATIO inverse({}) n={} hop={} J={} {}{}: {:.4f}".format(
        route(n), n, hop, Z.shape[-1], window, tag, ratio(err, bar)))
    assert np.isfinite(x).all()
    assert (err <= bar).all()
    return x, norm


# ------------------------------------------------------------------------------ (a) forward
def _forward_cases():
    cases = []
    for n in ALL_N:
        half, quarter = max(1, n // 2), max(1, n // 4)
        cases.append((n, half, lengths(n, half)[0], "hann", None))  # hop_length=None, no padding
        cases.append((n, quarter, lengths(n, quarter)[1], ("kaiser", 8.6), "same"))  # pads hop - 1
        cases.append((n, n, n, "boxcar", "same"))  # L == n, hop == n
    cases.append((64, 1, 150, "hann", "same"))  # many frames
    cases.append((100, 33, lengths(100, 33)[0], "hann", "same"))  # a hop that does not divide n
    cases.append((100, 33, lengths(100, 33)[1], ("kaiser", 8.6), "same"))
    for n in (2, 64, 100, 1024, 4097):
        cases.append((n, max(1, n // 2), lengths(n, max(1, n // 2))[1], ARRAY, "same"))
    return cases


@pytest.mark.parametrize("n,hop,L,window,hop_arg", _forward_cases())
def test_forward_per_element(n, hop, L, window, hop_arg):
    x = sr.signal(n + hop + L, 4, L, n, hop)
    Z = check_forward(x, n, hop, window, hop_arg)
    assert (Z[1] == 0).all()  # the zero channel next to the loud one


# ------------------------------------------------------- (b) more segments than resident workgroups
def test_global_route_walks_more_segments_than_workgroups():
    """n = 4097 leaves LDS; 65 channels x 4 frames = 260 segments on 256 workgroups, so channel 64
    is computed in the scratch slices channel 0 used.  Every channel has its own decade, channel 0 the
    loudest (1e32) and channel 64 the quietest (1e-32): any residue of the earlier segment shows.  A
    NaN in channel 0 must stay there."""
    from ssspy_amd.transform import istft, stft

    n = hop = 4097
    C, L = 65, 3 * 4097
    assert sr.frames(L, n, hop)[1] == 4
    rng = np.random.default_rng(4097)
    decade = 10.0 ** (32 - np.arange(C))
    x = rng.standard_normal((C, L)) * decade[:, None]
    x[1] = 0.0
    Z = check_forward(x, n, hop, "hann", tag=" 260 segments")
    assert (Z[1] == 0).all()
    xn = x.copy()
    xn[0, L // 2] = np.nan
    Zn = stft(xn, n_fft=n, hop_length=hop)
    assert np.array_equal(Zn[1:], Z[1:]) and np.isnan(Zn[0]).any()

    Zi = (rng.standard_normal((C, n // 2 + 1, 4)) + 1j * rng.standard_normal((C, n // 2 + 1, 4))) \
        * decade[:, None, None]
    Zi[1] = 0.0
    xi, _ = check_inverse(Zi, n, hop, "boxcar", tag=" 260 segments")
    assert (xi[1] == 0).all()
    Zi[0, 7, 2] = np.nan
    assert np.array_equal(istft(Zi, n_fft=n, hop_length=hop, window="boxcar")[1:], xi[1:])


# ------------------------------------------------------------------------------ (c) inverse
INVERSE = [
    # output lengths 256, 255, 257, 255 around the overlap-add's 256-sample blocks
    (64, 32, 9, "hann"), (64, 17, 16, "hann"), (127, 32, 9, "hann"), (127, 127, 3, "boxcar"),
    (2, 1, 5, "boxcar"), (4, 2, 5, "hann"), (3, 1, 6, "boxcar"), (5, 2, 6, "hann"), (6, 3, 5, "hann"),
    (100, 33, 7, ("kaiser", 8.6)), (129, 64, 5, "hann"), (255, 64, 6, "hann"), (257, 128, 5, "hann"),
    (512, 128, 6, "hann"), (1024, 512, 5, "hann"), (2047, 512, 5, "hann"), (2049, 1024, 4, "hann"),
    (4095, 2048, 4, "hann"), (8192, 4096, 3, ("kaiser", 8.6)), (4097, 1024, 6, "hann"),
    (16384, 8192, 3, "hann"), (100, 50, 5, ARRAY),
]


@pytest.mark.parametrize("n,hop,J,window", INVERSE)
def test_inverse_per_sample(n, hop, J, window):
    Z = sr.spectrogram(n + hop + J, 3, n, J)
    assert (Z.imag[0, 0] != 0).any() and (Z.imag[0, -1] != 0).any()
    x, _ = check_inverse(Z, n, hop, window)
    assert (x[1] == 0).all()


def test_inverse_output_lengths_straddle_the_block():
    assert [sr.istft_samples(J, n, hop) for n, hop, J, _ in INVERSE[:4]] == [256, 255, 257, 255]


@pytest.mark.parametrize("n", [64, 4096])
def test_inverse_takes_both_sides_of_the_norm_threshold(n):
    """hann with hop == n: the squared window alone is the divisor, exactly 0 at t = 0 and (n = 4096)
    below 1e-10 up to t = 4; there the sum is divided by 1."""
    Z = sr.spectrogram(n, 3, n, 3)
    near = np.concatenate([np.arange(n // 2 - 8, n // 2 + 9), np.arange(3 * n // 2 - 8, 3 * n // 2 + 9)])
    x, norm = check_inverse(Z, n, n, "hann", extra_samples=near, tag=" hop == n")
    small = np.asarray(norm <= sr.NORM_THRESHOLD)
    assert small.any() and not small.all()
    assert (np.asarray(norm)[small] == 0).any()
    if n == 4096:
        assert (np.asarray(norm)[small] > 0).any()


# ------------------------------------------------------------------------------ (d) round trip
@pytest.mark.parametrize("n,hop", [(64, 16), (100, 25), (257, 64), (1024, 256)])
def test_round_trip_within_the_composed_bars(n, hop):
    """istft(stft(x))[..., :L] against x where NOLA holds: the ISTFT's own bar at the spectrogram it
    was given, plus the forward bar carried through the exact inverse (stft_reference.propagate)."""
    from ssspy_amd.transform import istft, stft

    L = lengths(n, hop)[1]
    x = sr.signal(n + hop, 4, L, n, hop)
    w = window_samples("hann", n)
    Z = stft(x, n_fft=n, hop_length=hop)
    Zr, bar_Z = sr.stft(x, w, n, hop)
    assert (np.abs(Z - Zr) <= bar_Z).all()
    y = istft(Z, n_fft=n, hop_length=hop)
    _, bar_y, norm = sr.istft(Z, w, n, hop)
    assert (np.asarray(norm) > sr.NORM_THRESHOLD).all()  # NOLA
    bar = (bar_y + sr.propagate(bar_Z, w, n, hop))[..., :L]
    err = np.abs(y[..., :L] - x)
    print("RATIO roundtrip n={} hop={}: {:.4f}".format(n, hop, ratio(err, bar)))
    assert (err <= bar).all()
    assert (y[1] == 0).all()


# ------------------------------------------------------------------------------ (e) the C ABI, B > 1
def _abi_stft(x3, w, n, hop):
    from ssspy_amd import _device as dv
    from ssspy_amd import _lib
    from ssspy_amd.transform import _workspace

    lib = _lib.load()
    B, C, L = x3.shape
    xd = dv.to_device(x3, dtype=np.float64)
    J = int(lib.ssspy_stft_frames(L, n, hop))
    Z = dv.empty((B, C, n // 2 + 1, J), dv.c128, xd.device)
    wd = dv.to_device(w, dtype=np.float64)
    ws = _workspace(n, xd.device)
    _lib.check(lib.ssspy_stft(dv.ptr(xd), dv.ptr(Z), dv.ptr(wd), float(w.sum()), B, C, L, n, hop,
                              dv.ptr(ws), dv.stream_handle()), "stft")
    return dv.to_host(Z)


def _abi_istft(Z4, w, n, hop):
    from ssspy_amd import _device as dv
    from ssspy_amd import _lib
    from ssspy_amd.transform import _workspace

    lib = _lib.load()
    B, C, F, J = Z4.shape
    Zd = dv.to_device(Z4, dtype=np.complex128)
    L = int(lib.ssspy_istft_samples(J, n, hop))
    x = dv.empty((B, C, L), dv.f64, Zd.device)
    seg = dv.empty((B * C * J * n,), dv.f64, Zd.device)
    wd = dv.to_device(w, dtype=np.float64)
    ws = _workspace(n, Zd.device)
    _lib.check(lib.ssspy_istft(dv.ptr(Zd), dv.ptr(x), dv.ptr(wd), float(w.sum()), dv.ptr(seg), B, C,
                               J, n, hop, dv.ptr(ws), dv.stream_handle()), "istft")
    return dv.to_host(x)


@pytest.mark.parametrize("B,C", [(2, 3), (3, 1)])
@pytest.mark.parametrize("n,hop", [(64, 16), (100, 33), (4097, 2048)])
def test_c_abi_with_a_batch_axis(n, hop, B, C):
    """ssspy_stft / ssspy_istft with B > 1 (Python always passes B = 1): bit-equal to the same data as
    (1, B C), and inside the bars."""
    w = window_samples("hann", n)
    L = lengths(n, hop)[1]
    x = sr.signal(n + B, B * C, L, n, hop)
    Z = _abi_stft(x.reshape(B, C, L), w, n, hop)
    assert np.array_equal(Z.reshape((B * C,) + Z.shape[2:]), _abi_stft(x[None], w, n, hop)[0])
    bins = sr.check_bins(n, seed=n)
    Zr, bar = sr.stft(x, w, n, hop, bins)
    err = np.abs(Z.reshape((B * C,) + Z.shape[2:])[:, bins] - Zr)
    print("RATIO {} forward ABI B={} C={} n={}: {:.4f}".format(route(n), B, C, n, ratio(err, bar)))
    assert (err <= bar).all()

    Zi = sr.spectrogram(n + C, B * C, n, 5)
    y = _abi_istft(Zi.reshape((B, C) + Zi.shape[1:]), w, n, hop)
    assert np.array_equal(y.reshape(B * C, -1), _abi_istft(Zi[None], w, n, hop)[0])
    samples = sr.check_samples(y.shape[-1], n, seed=n)
    yr, ybar, norm = sr.istft(Zi, w, n, hop, samples)
    sr.assert_norm_clear_of_threshold(norm)
    err = np.abs(y.reshape(B * C, -1)[:, samples] - yr)
    print("RATIO inverse({}) ABI B={} C={} n={}: {:.4f}".format(route(n), B, C, n, ratio(err, ybar)))
    assert (err <= ybar).all()


# ------------------------------------------------------------------------------ (f) shapes, layouts
@pytest.mark.parametrize("lead", [(), (1,), (2, 3)])
def test_leading_axes(lead):
    n, hop = 100, 25
    L = lengths(n, hop)[1]
    C = int(np.prod(lead, dtype=np.int64))
    x = sr.signal(len(lead), max(C, 1), L, n, hop).reshape(lead + (L,))
    Z = check_forward(x, n, hop, "hann", tag=" lead={}".format(lead))
    Zi = sr.spectrogram(len(lead), max(C, 1), n, 6).reshape(lead + (n // 2 + 1, 6))
    check_inverse(Zi, n, hop, "hann", tag=" lead={}".format(lead))
    assert Z.shape[:-2] == lead


def test_layouts_and_repeat_runs_are_bit_equal():
    from ssspy_amd import _device as dv
    from ssspy_amd.transform import istft, stft

    n, hop = 100, 25
    L = lengths(n, hop)[1]
    x = sr.signal(11, 4, L, n, hop)
    Z = stft(x, n_fft=n, hop_length=hop)
    assert np.array_equal(Z, stft(x, n_fft=n, hop_length=hop))  # two runs
    Zd = stft(x, n_fft=n, hop_length=hop, device_output=True)
    assert Zd.is_cuda and np.array_equal(dv.to_host(Zd), Z)
    xt = dv.to_device(np.ascontiguousarray(x.T), dtype=np.float64).T  # a transposed view
    assert not xt.is_contiguous()
    assert np.array_equal(stft(xt, n_fft=n, hop_length=hop), Z)
    x2 = dv.to_device(np.repeat(x, 2, axis=0), dtype=np.float64)[::2]  # a strided slice
    assert not x2.is_contiguous()
    assert np.array_equal(stft(x2, n_fft=n, hop_length=hop), Z)

    Zi = sr.spectrogram(12, 4, n, 6)
    y = istft(Zi, n_fft=n, hop_length=hop)
    assert np.array_equal(y, istft(Zi, n_fft=n, hop_length=hop))
    yd = istft(Zi, n_fft=n, hop_length=hop, device_output=True)
    assert yd.is_cuda and np.array_equal(dv.to_host(yd), y)
    Zt = dv.to_device(np.ascontiguousarray(Zi.transpose(0, 2, 1)), dtype=np.complex128).transpose(1, 2)
    assert not Zt.is_contiguous()
    assert np.array_equal(istft(Zt, n_fft=n, hop_length=hop), y)
    assert np.array_equal(istft(dv.to_device(Zi, dtype=np.complex128), n_fft=n, hop_length=hop), y)


# ------------------------------------------------------------------------------ (g) non-finite
@pytest.mark.parametrize("n,hop", [(64, 16), (100, 33), (4097, 2048)])
def test_a_nan_stays_in_the_frames_that_hold_it(n, hop):
    from ssspy_amd.transform import istft, stft

    L = lengths(n, hop)[1] + 2 * n
    x = sr.signal(n, 3, L, n, hop)
    Z = stft(x, n_fft=n, hop_length=hop)
    at = L // 2 + 1
    xn = x.copy()
    xn[2, at] = np.nan
    Zn = stft(xn, n_fft=n, hop_length=hop)
    starts, J = sr.frames(L, n, hop)
    holds = (starts <= at) & (at < starts + n)
    assert holds.any() and not holds.all()
    assert np.array_equal(Zn[:2], Z[:2])
    assert np.array_equal(Zn[2][:, ~holds], Z[2][:, ~holds])
    assert np.isnan(Zn[2][:, holds]).all()

    Zi = sr.spectrogram(n, 3, n, J)
    y = istft(Zi, n_fft=n, hop_length=hop)
    Zin = Zi.copy()
    j = J // 2
    Zin[0, 1, j] = np.nan
    yn = istft(Zin, n_fft=n, hop_length=hop)
    p = np.arange(y.shape[-1]) + n // 2
    touched = (p >= j * hop) & (p < j * hop + n)
    assert np.array_equal(yn[1:], y[1:])
    assert np.array_equal(yn[0][~touched], y[0][~touched])


# ------------------------------------------------------------------------------ (h) input contract
def test_any_real_dtype_is_converted_to_float64():
    import torch

    from ssspy_amd import _device as dv
    from ssspy_amd.transform import istft, stft

    n, hop = 100, 25
    L = lengths(n, hop)[1]
    x = sr.signal(3, 3, L, n, hop)
    for dtype in (np.float32, np.float16, np.int16):
        with np.errstate(over="ignore"):
            xs = np.clip(x, -3e4, 3e4).astype(dtype)
        want = stft(xs.astype(np.float64), n_fft=n, hop_length=hop)
        assert np.array_equal(stft(xs, n_fft=n, hop_length=hop), want), dtype
    x32 = x.astype(np.float32)
    want = stft(x32.astype(np.float64), n_fft=n, hop_length=hop)
    assert np.array_equal(stft(torch.from_numpy(x32).to(dv.device()), n_fft=n, hop_length=hop), want)
    assert np.array_equal(stft(x32.tolist(), n_fft=n, hop_length=hop), want)  # a list

    Zi = sr.spectrogram(3, 3, n, 6).astype(np.complex64)
    want = istft(Zi.astype(np.complex128), n_fft=n, hop_length=hop)
    assert np.array_equal(istft(torch.from_numpy(Zi).to(dv.device()), n_fft=n, hop_length=hop), want)
    assert np.array_equal(istft(Zi, n_fft=n, hop_length=hop), want)
    Zreal = Zi.real.astype(np.float32)
    want = istft(Zreal.astype(np.complex128), n_fft=n, hop_length=hop)
    assert np.array_equal(istft(Zreal, n_fft=n, hop_length=hop), want)
    assert np.array_equal(istft(torch.from_numpy(Zreal).to(dv.device()), n_fft=n, hop_length=hop), want)
    assert np.array_equal(istft(Zreal.tolist(), n_fft=n, hop_length=hop), want)


def test_inputs_that_no_kernel_may_see_raise():
    """None of these reaches a launch: the checks come before the upload (they pass without a device
    too, tests/test_stft_reference_cpu.py)."""
    import torch

    from ssspy_amd import _device as dv
    from ssspy_amd.transform import istft, stft

    with pytest.raises(ValueError):
        stft(np.zeros((2, 100), np.complex64), n_fft=16)
    with pytest.raises(ValueError):
        stft(torch.zeros(2, 100, dtype=torch.complex128, device=dv.device()), n_fft=16)
    with pytest.raises(ValueError, match="HIP device"):
        stft(torch.zeros(2, 100, dtype=torch.float64), n_fft=16)
    with pytest.raises(ValueError, match="HIP device"):
        istft(torch.zeros(2, 9, 5, dtype=torch.complex128), n_fft=16)
    with pytest.raises(ValueError):
        stft(np.zeros((65536, 8)), n_fft=4)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (and no complex-to-real cast on the way)
        with pytest.raises(ValueError):
            stft(np.zeros((2, 100), np.complex128), n_fft=16)
