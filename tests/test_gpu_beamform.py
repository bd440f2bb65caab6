"""The mask-based beamformers on the device against the NumPy restatement (tests/beamform_numpy.py):
end to end within bars taken from the restatement's own sensitivity
(profiles/beamform_sensitivity.txt), one entry point at a time against extended precision within bars
derived from the operation counts, the routes against each other, batches, containers, the failure
paths and the composition with WPE and CACGMM."""

import functools

import numpy as np
import pytest

import beamform_cases
import beamform_numpy

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NAMES = tuple(b[0] for b in beamform_cases.BEAMFORMERS)
SPEC = {b[0]: b[1:] for b in beamform_cases.BEAMFORMERS}

# profiles/beamform_sensitivity.txt (benchmarks/tools/beamform_sensitivity.py): 1000 x how far the
# restatement itself moves under a 1e-15 relative perturbation of the input, per shape and beamformer
# (mvdr, gev-reference, gev-ban, mwf): (output, demix_filter)
BARS = {
    (1, 1, 1, 5, 1): ((1.7e-12, 1.0e-12), (1.7e-12, 1.0e-12), (1.7e-12, 1.0e-12), (1.7e-12, 1.0e-12)),
    (2, 1, 1, 7, 1): ((7.7e-12, 1.0e-12), (5.9e-12, 1.0e-12), (5.0e-12, 1.0e-12), (7.2e-12, 4.1e-11)),
    (3, 2, 3, 97, 2): ((7.3e-11, 3.7e-11), (2.9e-11, 7.4e-11), (3.1e-11, 7.8e-11), (2.4e-11, 6.1e-11)),
    (4, 3, 3, 257, 1): ((8.8e-11, 4.6e-11), (2.2e-11, 7.7e-11), (2.0e-11, 5.6e-11), (9.9e-12, 3.4e-11)),
    (5, 1, 2, 64, 1): ((6.1e-12, 1.6e-12), (4.1e-12, 1.5e-12), (3.4e-12, 1.2e-12), (1.4e-11, 4.0e-11)),
    (8, 16, 2, 300, 1): ((5.8e-12, 1.0e-12), (2.2e-11, 1.9e-12), (2.0e-11, 1.8e-12), (1.9e-11, 1.0e-12)),
    (2, 2, 2, 1700, 1): ((9.9e-12, 4.2e-12), (1.1e-11, 2.9e-12), (9.4e-12, 2.4e-12), (9.1e-12, 6.9e-12)),
}
# the same file, row "composition": MVDR behind WPE(taps=3, delay=1), 3 iterations, with the masks held
# fixed, on (3 channels, 2 sources, 9 bins, 64 frames)
COMPOSITION_CASE = (3, 2, 9, 64, 1)
COMPOSITION_BAR = 1.3e-09


def _beamformer(name, **kwargs):
    from ssspy_amd import beamform

    _, _, cls, cls_kwargs = SPEC[name]
    return getattr(beamform, cls)(**dict(cls_kwargs, **kwargs))


@functools.lru_cache(maxsize=None)
def _data(case):
    arrays = beamform_cases.make_case(case)
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _reference(case, name, dtype=np.float64):
    kind, kwargs = SPEC[name][:2]
    return beamform_numpy.run(*_data(case), kind=kind, dtype=dtype, **kwargs)


@functools.lru_cache(maxsize=None)
def _device_run(case, name):
    m = _beamformer(name)
    X, mask, noise_mask = _data(case)
    Y = m(X, mask, noise_mask=noise_mask)
    return Y, np.array(m.demix_filter), m


# ---- parity with the restatement
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", beamform_cases.CASES, ids=beamform_cases.case_id)
def test_parity_with_restatement(case, name):
    ref = _reference(case, name)
    Y, W, m = _device_run(case, name)
    out_bar, filter_bar = BARS[case][NAMES.index(name)]
    M, N, F, T, B = case
    lead = (B,) if B > 1 else ()
    assert Y.shape == lead + (N, F, T) and Y.dtype == np.complex128
    assert W.shape == lead + (F, N, M)
    assert (m.n_channels, m.n_sources, m.n_bins, m.n_frames) == (M, N, F, T)
    figures = (np.abs(Y - ref["output"]).max(), np.abs(W - ref["demix_filter"]).max())
    print("beamform parity {} {}: output {:.2e} (bar {:.1e}), filter {:.2e} (bar {:.1e})".format(
        case, name, figures[0], out_bar, figures[1], filter_bar))
    assert figures[0] <= out_bar
    assert figures[1] <= filter_bar


def test_route_of_every_shape():
    """Only the 1700-frame shape re-reads the slab; every shape within 160 KiB."""
    from ssspy_amd import _lib, _ops

    for case in beamform_cases.CASES:
        M, N, F, T, B = case
        route, lds = _ops.beamform_route(B, M, N, F, T)
        expected = (_lib.BEAMFORM_ROUTE_STREAMING if case == beamform_cases.STREAMING_CASE
                    else _lib.BEAMFORM_ROUTE_RESIDENT)
        assert route == expected, case
        assert 0 < lds <= 160 * 1024
    assert _ops.beamform_route(1, 8, 16, 1, 384)[0] == _lib.BEAMFORM_ROUTE_RESIDENT  # 48 KiB exactly
    assert _ops.beamform_route(1, 8, 16, 1, 385)[0] == _lib.BEAMFORM_ROUTE_STREAMING
    assert _ops.beamform_route(1, 8, 16, 1, 384)[1] <= 160 * 1024


# ---- one entry point at a time, against extended precision
def _four(a, batched):
    return a if batched else a[None]


@pytest.mark.parametrize("case", beamform_cases.ELEMENTWISE, ids=beamform_cases.case_id)
def test_covariance_sums_elementwise(case):
    """S_n, N_n, a_n, b_n of ssspy_beamform_covariances, every entry: pins the tile edge at 257 frames,
    the noise weight 1 - m and the ownership map of up to 1152 sums.
    Per entry the kernel adds T terms (w x_i) conj(x_j): one rounding for w x_i (and one for 1 - m in
    N_n), then two fused multiply-adds per real component and term, each one rounding on a partial
    sum below sum_t |w_t| |x_it| |x_jt|: (2 T + 2) eps per component, sqrt(2) of it on the modulus,
    below c (T + 2) eps sum_t |w_t| |x_it| |x_jt| with c = 4.  a_n, b_n: T - 1 additions (and the
    rounding of 1 - m): (T + 1) eps of the sum."""
    from ssspy_amd import _device as dv
    from ssspy_amd import _ops

    M, N, F, T, B = case
    X, mask, noise_mask = _data(case)
    ext = _reference(case, "mvdr", np.longdouble)
    X4, m4 = _four(np.asarray(X), B > 1), _four(np.asarray(mask), B > 1)
    u4 = 1.0 - m4 if noise_mask is None else np.broadcast_to(
        _four(np.asarray(noise_mask), B > 1)[:, None], m4.shape)
    S, Nv, a, b = (dv.to_host(t) for t in _ops.beamform_covariances(
        dv.to_device(X4, dtype=np.complex128), dv.to_device(m4, dtype=np.float64),
        None if noise_mask is None else dv.to_device(_four(np.asarray(noise_mask), B > 1),
                                                     dtype=np.float64)))
    absX = np.abs(X4)
    for name, got, weight in (("S", S, m4), ("Nv", Nv, u4)):
        bar = 4 * (T + 2) * EPS * np.einsum("bnft,bift,bjft->bfnij", np.abs(weight), absX, absX)
        err = np.abs(got - _four(ext[name], B > 1))
        print("beamform sums {} {}: max error / bar {:.3f}".format(
            case, name, float((err / bar).max())))
        assert np.all(err <= bar), name
        assert np.array_equal(got, np.conj(np.swapaxes(got, -1, -2))), name  # exactly Hermitian
    for name, got in (("a", a), ("b", b)):
        want = _four(ext[name], B > 1)
        err = np.abs(got - want)
        assert np.all(err <= (T + 1) * EPS * np.abs(want).astype(np.float64)), name


def _amplification(s, v, kind, mu):
    """cond of the factorised matrix and, for GEV, lambda_1 / (lambda_1 - lambda_2) of
    L^-1 Phi_s L^-H (tests/test_beamform_cpu.py states the bar these make)."""
    amp = float(np.linalg.cond(s + mu * v if kind == "mwf" else v))
    if kind == "gev" and s.shape[0] > 1:
        L = np.linalg.cholesky(v)
        Z = np.linalg.solve(L, s)
        lam = np.linalg.eigvalsh(np.linalg.solve(L, np.conj(Z.T)))
        amp *= float(lam[-1] / (lam[-1] - lam[-2]))
    return amp


def _covariance_sets():
    """(label, Phi_s, Phi_v) as (B, F, N, M, M) doubles: two test shapes, and one whose masks sum to
    one in every frame, the situation behind CACGMM."""
    sets = []
    for case in (beamform_cases.CASES[2], beamform_cases.CASES[5]):
        ref = _reference(case, "mvdr")
        sets.append((beamform_cases.case_id(case),
                     _four(ref["signal_covariance"], case[4] > 1),
                     _four(ref["noise_covariance"], case[4] > 1)))
    case = beamform_cases.CASES[3]
    X, mask, _ = _data(case)
    posterior = mask + 1e-3  # (no frame without a weight: the masks are zero where nothing is active)
    posterior = posterior / posterior.sum(axis=0, keepdims=True)
    ref = beamform_numpy.run(X, posterior, None, kind="mvdr", loading=1e-6)
    sets.append(("masks-sum-to-one", ref["signal_covariance"][None], ref["noise_covariance"][None]))
    return sets


@pytest.mark.parametrize("name", NAMES)
def test_filter_elementwise(name):
    """ssspy_beamform_filter from given covariances against the restatement in longdouble on the same
    doubles, every entry of every filter within 100 M eps times the amplification of its own
    (bin, source): the backward error of a factorisation and two solves (and a Jacobi iteration to
    ~M eps) with room for the products around them."""
    from ssspy_amd import _device as dv
    from ssspy_amd import _lib, _ops

    kind, kwargs = SPEC[name][:2]
    code = {"mvdr": _lib.BEAMFORM_MVDR, "gev-reference": _lib.BEAMFORM_GEV_REFERENCE,
            "gev-ban": _lib.BEAMFORM_GEV_BAN, "mwf": _lib.BEAMFORM_MWF}[name]
    mu = kwargs.get("mu", 1.0)
    for label, Ps, Pv in _covariance_sets():
        B, F, N, M = Ps.shape[:4]
        ref_id = M - 1
        info = dv.zeros((2,), dv.i32)
        W = dv.to_host(_ops.beamform_filter(dv.to_device(Ps, dtype=np.complex128),
                                            dv.to_device(Pv, dtype=np.complex128), code, ref_id,
                                            mu=mu, info=info))
        assert info.tolist() == [0, 0]
        worst = 0.0
        for b in range(B):
            for f in range(F):
                for n in range(N):
                    s, v = Ps[b, f, n], Pv[b, f, n]
                    w, failed = beamform_numpy.filter_from_covariances(
                        s.astype(np.clongdouble), v.astype(np.clongdouble), kind, ref=ref_id, mu=mu,
                        normalization=kwargs.get("normalization", "reference"))
                    assert not failed
                    bar = 100 * M * EPS * _amplification(s, v, kind, mu) * max(
                        1.0, float(np.abs(w).max()))
                    err = float(np.abs(W[b, f, n] - np.conj(w)).max())
                    worst = max(worst, err / bar)
                    assert err <= bar, (label, b, f, n, err, bar)
        print("beamform filter {} {}: max error / bar {:.3f}".format(name, label, worst))


# ---- routes and reproducibility
@pytest.mark.parametrize("name", NAMES)
def test_slab_in_lds_against_reread_bit_for_bit(name):
    from ssspy_amd import _routes

    case = beamform_cases.CASES[3]
    X, mask, noise_mask = _data(case)
    Y, W, _ = _device_run(case, name)
    with _routes.override(beamform_resident=False):
        m = _beamformer(name)
        Ys = m(X, mask, noise_mask=noise_mask)
        Ws = np.array(m.demix_filter)
    assert np.array_equal(Ys, Y) and np.array_equal(Ws, W)


def test_runs_repeat_bit_for_bit():
    for case in (beamform_cases.CASES[5], beamform_cases.STREAMING_CASE):
        X, mask, noise_mask = _data(case)
        Y, W, _ = _device_run(case, "gev-reference")
        m = _beamformer("gev-reference")
        assert np.array_equal(m(X, mask, noise_mask=noise_mask), Y)
        assert np.array_equal(np.array(m.demix_filter), W)


# ---- batches and containers
def test_batch_equals_single_runs():
    case = beamform_cases.CASES[2]
    X, mask, _ = _data(case)
    for name in NAMES:
        Y, W, _ = _device_run(case, name)
        for b in range(case[4]):
            m = _beamformer(name)
            assert np.array_equal(m(X[b], mask[b]), Y[b]), name
            assert np.array_equal(np.array(m.demix_filter), W[b]), name


def test_device_tensors_in_device_tensor_out():
    import torch

    case = beamform_cases.SHARED_NOISE_CASE
    X, mask, noise_mask = (torch.from_numpy(np.array(a)).to("cuda") for a in _data(case))
    m = _beamformer("mvdr")
    Yd = m(X, mask, noise_mask=noise_mask)
    assert isinstance(Yd, torch.Tensor) and Yd.is_cuda and Yd.dtype == torch.complex128
    assert tuple(Yd.shape) == _device_run(case, "mvdr")[0].shape
    assert m._state()["output"]["host"] is None  # (nothing was downloaded)
    assert np.array_equal(Yd.cpu().numpy(), _device_run(case, "mvdr")[0])
    applied = m.apply(X)
    assert isinstance(applied, torch.Tensor) and torch.equal(applied, Yd)
    from ssspy_amd.beamform import masked_covariance

    S = masked_covariance(X, mask)
    assert isinstance(S, torch.Tensor) and S.is_cuda
    assert np.array_equal(S.cpu().numpy(), np.array(m.signal_covariance))


def test_numpy_in_numpy_out_and_any_real_mask_dtype():
    case = beamform_cases.CASES[2]
    X, mask, _ = _data(case)
    Y, _, _ = _device_run(case, "mwf")
    assert isinstance(Y, np.ndarray)
    m = _beamformer("mwf")
    m(X, mask.astype(np.float32))
    ref = beamform_numpy.run(X, mask.astype(np.float32), None, kind="mwf")
    assert np.abs(np.array(m.output) - ref["output"]).max() <= BARS[case][3][0]


def test_apply_reproduces_output_and_covariances_agree():
    from ssspy_amd.beamform import masked_covariance

    for case in (beamform_cases.CASES[2], beamform_cases.STREAMING_CASE):
        X, mask, noise_mask = _data(case)
        Y, _, m = _device_run(case, "mvdr")
        assert np.array_equal(m.apply(X), Y)
        ref = _reference(case, "mvdr")
        Ps, Pv = np.array(m.signal_covariance), np.array(m.noise_covariance)
        assert Ps.shape == ref["signal_covariance"].shape == Pv.shape
        assert np.array_equal(masked_covariance(X, mask), Ps)
        # the sums within 4 (T + 2) eps sum |w| |x_i| |x_j| (test_covariance_sums_elementwise), which
        # is at most the largest diagonal entry (Cauchy-Schwarz); the weight sum and the division add
        # (T + 2) eps, the restatement's own double sums up to 2 (T + 2) eps: 8 (T + 2) eps in all
        T = case[3]
        for got, key in ((Ps, "signal_covariance"), (Pv, "noise_covariance")):
            scale = float(np.abs(ref[key]).max())
            assert np.abs(got - ref[key]).max() <= 8 * (T + 2) * EPS * scale, key
        raw = masked_covariance(X, mask, normalize=False)
        assert np.abs(raw - ref["S"]).max() <= 8 * (T + 2) * EPS * float(np.abs(ref["S"]).max())


# ---- failure paths: ordinary error returns
@pytest.mark.parametrize("name", NAMES)
def test_all_zero_mask_gives_zero_output_and_no_error(name):
    case = beamform_cases.CASES[2]
    X, mask, _ = _data(case)
    mask = np.array(mask)
    mask[:, 1] = 0
    m = _beamformer(name)
    Y = m(X, mask)
    assert np.all(Y[:, 1] == 0) and np.all(np.array(m.demix_filter)[:, :, 1] == 0)
    assert np.all(np.isfinite(Y)) and np.any(Y[:, 0] != 0)


def _exactly_singular():
    """Two channels, one frame, three bins of small Gaussian integers and masks of one half: every
    product, sum and quotient on the way to Phi_v = x x^H is exact, its first pivot a power of four
    and its second pivot exactly zero."""
    X = np.array([[[2.0], [4.0], [1.0]], [[1 + 1j], [2 - 2j], [1j]]], dtype=np.complex128)
    return X, np.full((2, 3, 1), 0.5)


@pytest.mark.parametrize("name", ("mvdr", "gev-reference", "gev-ban"))
def test_too_few_frames_without_loading_is_singular(name):
    """(MWF factorises Phi_s + mu Phi_v = 2 x x^H here, whose first pivot 8 has no exact root: the
    sign of its second pivot is rounding, so it is left out.)"""
    X, mask = _exactly_singular()
    m = _beamformer(name, diagonal_loading=0.0)
    with pytest.raises(np.linalg.LinAlgError, match=r"6 \(mixture, bin, source\)"):
        m(X, mask)
    assert np.all(np.isfinite(np.asarray(m.output))) and np.all(np.asarray(m.output) == 0)
    assert beamform_numpy.run(X, mask, None, kind=SPEC[name][0])["failed"] == 6
    Y = _beamformer(name)(X, mask)  # the default loading
    assert np.all(np.isfinite(Y)) and np.any(Y != 0)


def test_limits_and_mismatches_raise_as_specified():
    X, mask, _ = _data(beamform_cases.CASES[2])
    with pytest.raises(NotImplementedError, match="channels"):
        _beamformer("mvdr")(np.zeros((9, 2, 30), dtype=np.complex128), np.zeros((1, 2, 30)))
    with pytest.raises(NotImplementedError, match="masks"):
        _beamformer("gev-ban")(np.zeros((2, 2, 30), dtype=np.complex128), np.zeros((17, 2, 30)))
    with pytest.raises(ValueError):
        _beamformer("mwf")(X, mask[0])
    with pytest.raises(ValueError, match="reference_id"):
        _beamformer("mvdr", reference_id=3)(X, mask)
    m = _beamformer("mvdr", reference_id=-1)
    m(X, mask)
    assert np.array_equal(np.array(m.demix_filter),
                          np.array(_run_with_reference(X, mask, X.shape[-3] - 1)))
    with pytest.raises(ValueError):
        m.apply(X[:, :, :2])


def _run_with_reference(X, mask, reference_id):
    m = _beamformer("mvdr", reference_id=reference_id)
    m(X, mask)
    return m.demix_filter


# ---- composition: WPE -> CACGMM -> MVDR
def test_mvdr_behind_wpe_and_cacgmm():
    from ssspy_amd.bss.cacgmm import CACGMM
    from ssspy_amd.dereverb import WPE

    X, _, _ = _data(COMPOSITION_CASE)
    dereverberated = WPE(taps=3, delay=1)(X, n_iter=3)
    cacgmm = CACGMM(n_sources=2, rng=np.random.default_rng(0))
    cacgmm(dereverberated, n_iter=5)
    posterior = np.array(cacgmm.posterior)
    assert posterior.shape == (2,) + X.shape[1:]
    Y = _beamformer("mvdr")(dereverberated, posterior)
    ref = beamform_numpy.run(dereverberated, posterior, None, kind="mvdr", loading=1e-6)
    worst = np.abs(Y - ref["output"]).max()
    print("wpe + cacgmm + mvdr {}: {:.2e} (bar {:.1e})".format(COMPOSITION_CASE, worst,
                                                                COMPOSITION_BAR))
    assert worst <= COMPOSITION_BAR
