"""The mask-based beamformers without a device: the NumPy restatement against itself in extended
precision, the properties that define each beamformer on an exactly rank-1 source covariance, the
all-zero-mask rule, and the constructor / argument / limit paths of the classes."""

import functools

import numpy as np
import pytest

import beamform_cases
import beamform_numpy
from ssspy_amd.beamform import GEV, MVDR, MWF, MaskBeamformerBase, masked_covariance

EPS = np.finfo(np.float64).eps
KEYS = ("output", "demix_filter", "signal_covariance", "noise_covariance")


@functools.lru_cache(maxsize=None)
def _pair(case, name):
    kind, kwargs = {b[0]: b[1:3] for b in beamform_cases.BEAMFORMERS}[name]
    X, mask, noise_mask = beamform_cases.make_case(case)
    return tuple(beamform_numpy.run(X, mask, noise_mask, kind=kind, dtype=dtype, **kwargs)
                 for dtype in (np.float64, np.longdouble))


def _amplification(run, kind, mu):
    """cond of the matrix the beamformer factorises, times, for GEV, lambda_1 / (lambda_1 - lambda_2)
    of L^-1 Phi_s L^-H: what a relative rounding error is amplified by, at the worst (bin, source)."""
    Ps = run["signal_covariance"].reshape(-1, *run["signal_covariance"].shape[-2:])
    Pv = run["noise_covariance"].reshape(-1, *run["noise_covariance"].shape[-2:])
    worst = 1.0
    for s, v in zip(Ps, Pv):
        A = s + mu * v if kind == "mwf" else v
        amp = float(np.linalg.cond(A))
        if kind == "gev" and s.shape[0] > 1:
            L = np.linalg.cholesky(v)
            Z = np.linalg.solve(L, s)
            lam = np.linalg.eigvalsh(np.linalg.solve(L, np.conj(Z.T)))
            amp *= float(lam[-1] / (lam[-1] - lam[-2]))
        worst = max(worst, amp)
    return worst


@pytest.mark.parametrize("name", [b[0] for b in beamform_cases.BEAMFORMERS])
@pytest.mark.parametrize("case", beamform_cases.CASES, ids=beamform_cases.case_id)
def test_restatement_double_agrees_with_longdouble(case, name):
    """The double run is the longdouble run up to rounding: T eps on the sums, and on the filter the
    backward error of a factorisation and two solves, ~M eps each (Higham, Accuracy and Stability,
    th. 10.4), amplified by the condition number of the factorised matrix and, for GEV, by the
    reciprocal relative eigen-gap.  100 M eps times that leaves room for the products around them."""
    double, extended = _pair(case, name)
    kind, kwargs = {b[0]: b[1:3] for b in beamform_cases.BEAMFORMERS}[name]
    M, _, _, T, _ = case
    assert double["failed"] == 0 and extended["failed"] == 0
    for key in ("signal_covariance", "noise_covariance"):
        scale = max(1.0, float(np.abs(extended[key]).max()))
        assert np.abs(double[key] - extended[key]).max() <= 4 * (T + 2) * EPS * scale, key
    bar = 100 * M * EPS * _amplification(double, kind, kwargs.get("mu", 1.0))
    for key in ("output", "demix_filter"):
        scale = max(1.0, float(np.abs(extended[key]).max()))
        worst = float(np.abs(double[key] - extended[key]).max())
        print("beamform {} {} {}: {:.2e} (bar {:.1e})".format(case, name, key, worst, bar * scale))
        assert worst <= bar * scale, key


def _rank_one(M, seed, dtype=np.complex128):
    rng = np.random.default_rng(seed)
    h = (rng.standard_normal(M) + 1j * rng.standard_normal(M)).astype(dtype)
    G = (rng.standard_normal((M, 2 * M)) + 1j * rng.standard_normal((M, 2 * M))).astype(dtype)
    return h, np.outer(h, np.conj(h)), G @ np.conj(G.T) / (2 * M)


@pytest.mark.parametrize("M", (2, 3, 8))
@pytest.mark.parametrize("ref", (0, 1))
def test_mvdr_and_gev_reference_are_distortionless(M, ref):
    """On Phi_s = h h^H exactly, w^H h = h_ref for MVDR (w = Phi_v^-1 h conj(h_ref) / h^H Phi_v^-1 h)
    and for GEV with the reference normalisation (a = Phi_v w0 is h up to a factor)."""
    h, Phi_s, Phi_v = _rank_one(M, seed=M)
    for kind in ("mvdr", "gev"):
        w, failed = beamform_numpy.filter_from_covariances(Phi_s, Phi_v, kind, ref=ref)
        assert not failed
        assert abs(np.conj(w) @ h - h[ref]) <= 1e-10 * np.abs(h).max(), kind


@pytest.mark.parametrize("normalization", ("reference", "ban"))
@pytest.mark.parametrize("dtype", (np.complex128, np.clongdouble))
def test_gev_does_not_depend_on_the_phase_of_the_eigenvector(normalization, dtype):
    rng = np.random.default_rng(3)
    _, Phi_s, Phi_v = _rank_one(4, seed=11, dtype=dtype)
    Phi_s = Phi_s + 0.05 * _rank_one(4, seed=12, dtype=dtype)[2]  # (full rank: a generic problem)
    base, _ = beamform_numpy.filter_from_covariances(Phi_s, Phi_v, "gev", ref=1,
                                                     normalization=normalization)
    for _ in range(3):
        phase = np.exp(2j * np.pi * rng.random())
        w, _ = beamform_numpy.filter_from_covariances(Phi_s, Phi_v, "gev", ref=1,
                                                      normalization=normalization, phase=phase)
        assert np.abs(w - base).max() <= 1e-13 * np.abs(base).max()


def test_ban_gain_is_real_positive_towards_the_reference():
    """The pinned phase: w^H a = conj(p) ||a|| / sqrt(M) for the steering vector a the filter itself
    estimates, so w^H a / a_ref = ||a|| / (sqrt(M) |a_ref|) is real and positive."""
    h, Phi_s, Phi_v = _rank_one(3, seed=5)
    w, _ = beamform_numpy.filter_from_covariances(Phi_s, Phi_v, "gev", ref=2, normalization="ban")
    response = np.conj(w) @ h / h[2]  # a is h up to a factor, so this is |.| > 0 with zero phase
    assert abs(response.imag) <= 1e-12 * abs(response) and response.real > 0


@pytest.mark.parametrize("M", (2, 5))
def test_filters_are_parallel_on_a_rank_one_source(M):
    """MVDR, MWF and GEV all point along Phi_v^-1 h when Phi_s = h h^H."""
    h, Phi_s, Phi_v = _rank_one(M, seed=20 + M)
    direction = np.linalg.solve(Phi_v, h)
    for kind, kwargs in (("mvdr", {}), ("mwf", {"mu": 0.3}), ("mwf", {"mu": 4.0}),
                         ("gev", {"normalization": "reference"}), ("gev", {"normalization": "ban"})):
        w, _ = beamform_numpy.filter_from_covariances(Phi_s, Phi_v, kind, **kwargs)
        cosine = abs(np.vdot(direction, w)) / (np.linalg.norm(direction) * np.linalg.norm(w))
        assert abs(cosine - 1) <= 1e-10, (kind, kwargs)


@pytest.mark.parametrize("name", [b[0] for b in beamform_cases.BEAMFORMERS])
def test_all_zero_mask_gives_a_zero_filter(name):
    kind, kwargs = {b[0]: b[1:3] for b in beamform_cases.BEAMFORMERS}[name]
    X, mask, _ = beamform_cases.make_case(beamform_cases.CASES[2])
    mask = mask.copy()
    mask[:, 1] = 0
    run = beamform_numpy.run(X, mask, None, kind=kind, **kwargs)
    assert run["failed"] == 0
    assert np.all(run["demix_filter"][:, :, 1] == 0) and np.all(run["output"][:, 1] == 0)
    assert np.all(np.isfinite(run["output"])) and np.any(run["output"][:, 0] != 0)


def test_noise_weight_is_one_minus_mask_not_total_minus_signal():
    """With a mask within 2^-30 of one the noise covariance still has full relative accuracy: the
    weight 2^-30 cancels between N_n and b_n (7 * 2^-30 > eps).  Total minus signal would leave
    eps / 2^-30 = 2e-7 of it."""
    X, _, _ = beamform_cases.make_case(beamform_cases.CASES[1])
    mask = np.full((1,) + X.shape[1:], 1 - 2.0 ** -30)
    run = beamform_numpy.run(X, mask, None, kind="mvdr")
    exact = np.einsum("it,jt->ij", X[:, 0], np.conj(X[:, 0])) / X.shape[-1]
    assert np.abs(run["noise_covariance"][0, 0] - exact).max() <= 1e-12 * np.abs(exact).max()
    assert np.all(run["b"] > 0)


# ---- the classes, as far as they go without a device
def test_constructors_and_repr():
    m = MVDR()
    assert (m.reference_id, m.diagonal_loading) == (0, 1e-6)
    assert repr(m) == "MVDR(reference_id=0, diagonal_loading=1e-06)"
    g = GEV(reference_id=2, normalization="ban")
    assert (g.reference_id, g.diagonal_loading, g.normalization) == (2, 1e-6, "ban")
    assert repr(g) == "GEV(reference_id=2, diagonal_loading=1e-06, normalization=ban)"
    w = MWF(mu=2)
    assert (w.reference_id, w.diagonal_loading, w.mu) == (0, 0.0, 2.0)
    assert repr(w) == "MWF(reference_id=0, diagonal_loading=0.0, mu=2.0)"
    assert all(isinstance(x, MaskBeamformerBase) for x in (m, g, w))
    assert MVDR(reference_id=-1).reference_id == -1


@pytest.mark.parametrize("cls, kwargs", [
    (MVDR, {"diagonal_loading": -1e-3}), (MVDR, {"diagonal_loading": float("nan")}),
    (MVDR, {"reference_id": 0.5}), (GEV, {"normalization": "none"}),
    (GEV, {"diagonal_loading": float("inf")}), (MWF, {"mu": 0.0}), (MWF, {"mu": -1.0}),
    (MWF, {"mu": float("nan")}),
])
def test_bad_constructor_values_are_value_errors(cls, kwargs):
    with pytest.raises(ValueError):
        cls(**kwargs)


def _zeros(input_shape, mask_shape):
    return np.zeros(input_shape, dtype=np.complex128), np.zeros(mask_shape)


@pytest.mark.parametrize("input_shape, mask_shape, noise_shape", [
    ((3, 20), (2, 3, 20), None),                # rank of input
    ((2, 3, 20), (3, 20), None),                # rank of mask
    ((2, 2, 3, 20), (2, 3, 20), None),          # a batch with a single mixture's mask
    ((2, 3, 20), (2, 4, 20), None),             # bins
    ((2, 3, 20), (2, 3, 21), None),             # frames
    ((2, 2, 3, 20), (3, 2, 3, 20), None),       # mixtures
    ((2, 3, 20), (2, 3, 20), (3, 3, 20)),       # noise mask: sources
    ((2, 3, 20), (2, 3, 20), (20,)),            # noise mask: rank
    ((2, 2, 3, 20), (2, 2, 3, 20), (3, 20)),    # noise mask of a batch without its mixture axis
    ((2, 0, 20), (2, 0, 20), None),             # an empty axis
])
def test_shape_mismatches_are_value_errors(input_shape, mask_shape, noise_shape):
    X, mask = _zeros(input_shape, mask_shape)
    noise = None if noise_shape is None else np.zeros(noise_shape)
    for m in (MVDR(), GEV(), MWF()):
        with pytest.raises(ValueError):
            m(X, mask, noise_mask=noise)
    if noise is None:
        with pytest.raises(ValueError):
            masked_covariance(X, mask)


def test_mixed_containers_are_value_errors():
    import torch

    X, mask = _zeros((2, 3, 20), (2, 3, 20))
    with pytest.raises(ValueError, match="NumPy"):
        MVDR()(X, torch.zeros(2, 3, 20, dtype=torch.float64))
    with pytest.raises(ValueError, match="NumPy"):
        MVDR()(torch.zeros(2, 3, 20, dtype=torch.complex128), mask)
    with pytest.raises(ValueError, match="NumPy"):
        GEV()(X, mask, noise_mask=torch.zeros(3, 20, dtype=torch.float64))
    with pytest.raises(ValueError, match="NumPy"):
        masked_covariance(X, torch.zeros(2, 3, 20, dtype=torch.float64))


def test_bad_masks_are_value_errors_before_anything_is_uploaded():
    X, mask = _zeros((2, 3, 20), (2, 3, 20))
    for bad in (-1e-3, np.nan, np.inf):
        wrong = mask.copy()
        wrong[1, 2, 3] = bad
        with pytest.raises(ValueError, match="finite"):
            MVDR()(X, wrong)
        with pytest.raises(ValueError, match="finite"):
            MVDR()(X, mask, noise_mask=wrong)
        with pytest.raises(ValueError, match="finite"):
            masked_covariance(X, wrong)
    with pytest.raises(ValueError, match="real"):
        MVDR()(X, mask.astype(np.complex128))


@pytest.mark.parametrize("reference_id", (2, -3, 7))
def test_reference_id_is_checked_against_the_channels(reference_id):
    X, mask = _zeros((2, 3, 20), (2, 3, 20))
    for cls in (MVDR, GEV, MWF):
        with pytest.raises(ValueError, match="reference_id"):
            cls(reference_id=reference_id)(X, mask)


@pytest.mark.parametrize("input_shape, mask_shape, match", [
    ((9, 3, 20), (2, 3, 20), "channels"),
    ((2, 3, 20), (17, 3, 20), "masks"),
    ((2, 9, 3, 20), (2, 1, 3, 20), "channels"),
])
def test_limits_raise_before_anything_is_uploaded(input_shape, mask_shape, match):
    X, mask = _zeros(input_shape, mask_shape)
    for m in (MVDR(), GEV(), MWF()):
        with pytest.raises(NotImplementedError, match=match):
            m(X, mask)
    with pytest.raises(NotImplementedError, match=match):
        masked_covariance(X, mask)


def test_apply_needs_a_call():
    with pytest.raises(ValueError):
        MVDR().apply(np.zeros((2, 3, 20), dtype=np.complex128))
