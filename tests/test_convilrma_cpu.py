"""ConvILRMA without a device: the descent of the NumPy restatement (tests/convilrma_numpy.py), the
restatement against itself in extended precision, taps = 0 against the GaussILRMA-IP1 oracle (which
is pinned to the reference's goldens), and the constructor / limit paths of the class."""

import functools

import numpy as np
import pytest

import convilrma_cases
import convilrma_numpy
from oracle import spatial as sp
from oracle.ilrma import GaussILRMAOracle
from ssspy_amd.bss import ConvGaussILRMA, ConvIVABase
from ssspy_amd.special.flooring import add_flooring, identity, max_flooring

EPS = np.finfo(np.float64).eps
N_ITER = convilrma_cases.N_ITER


@functools.lru_cache(maxsize=None)
def _mixture(case):
    return convilrma_cases.make_mixture(case)


def _run(case, **kwargs):
    basis, activation = convilrma_cases.make_factors(case)
    kwargs.setdefault("domain", case[7])
    return convilrma_numpy.run(_mixture(case), case[1], case[2], n_iter=N_ITER, basis=basis,
                               activation=activation, **kwargs)


# ---- the restatement
@pytest.mark.parametrize("normalization", (True, False))
@pytest.mark.parametrize("case", convilrma_cases.CASES, ids=convilrma_cases.case_id)
def test_restatement_loss_is_non_increasing(case, normalization):
    """The MM updates of the factors lower the data term for the current Y, step 2 minimises the
    majoriser over G_n for any q_n, step 3 is IP1 on what is left, and the normalisation moves
    (2 / p) log TV and log|det Q| by the same amount: no step may raise the loss by more than its own
    rounding (loading 0; the floor of 1e-10 does not bind on these shapes)."""
    out = _run(case, normalization=normalization)
    loss = np.asarray(out["loss"])
    assert out["failed"] == 0 and np.all(np.isfinite(loss))
    assert np.all(loss[1:] <= loss[:-1] + 1e-12 * np.abs(loss[:-1]))
    assert np.all(loss[-1] < loss[0])


def test_restatement_normalisation_leaves_the_loss_and_sets_unit_power():
    case = convilrma_cases.CASES[1]
    plain = _run(case, normalization=False, scale_restoration=False)
    normed = _run(case, normalization=True, scale_restoration=False)
    rel = np.abs(np.asarray(normed["loss"]) / np.asarray(plain["loss"]) - 1).max()
    assert rel <= 1e-12
    power = np.mean(np.abs(normed["output"]) ** 2, axis=(-2, -1))
    assert np.abs(power - 1).max() <= 1e-12


@pytest.mark.parametrize("case", convilrma_cases.SMALL, ids=convilrma_cases.case_id)
def test_restatement_double_agrees_with_longdouble(case):
    """As test_conviva_cpu.py: per iteration one solve off by at most ~L eps cond(R) relative and one
    sweep, on filters and spectrograms of order one; the NMF updates are ratios of sums of positive
    terms (relative error of a few (T + Kb) eps, below Lb cond(R) here): 100 Lb eps cond(R)."""
    double, extended = (_run(case, dtype=dtype) for dtype in (np.float64, np.longdouble))
    Lb = case[0] * (case[1] + 1)
    bar = 100 * Lb * EPS * max(double["max_cond"], 1.0)
    assert double["failed"] == 0 and extended["failed"] == 0
    for key in ("output", "convolutional_filter", "prediction_filter", "basis", "activation"):
        scale = max(1.0, float(np.abs(extended[key]).max()))
        assert np.abs(double[key] - extended[key]).max() <= bar * scale, key
    rel = np.abs(np.asarray(double["loss"]) / np.asarray(extended["loss"], dtype=np.float64) - 1)
    assert rel.max() <= bar


@pytest.mark.parametrize("normalization", (True, False))
@pytest.mark.parametrize("domain", (2, 1))
def test_taps_zero_is_the_gauss_ilrma_ip1_oracle(domain, normalization):
    """taps = 0: Sigma_n is the weighted covariance with varphi = 1 / (TV)^(2/p) and the sweep is
    update_by_ip1, so the run is GaussILRMA with IP1 from the same factors.  The two restatements
    differ in the order of the T-term sums of the covariances (8 T eps relative with 8 real operations
    per complex multiply-add), of the M-term products of the sweep (8 M^3 eps) and of the T-, F- and
    Kb-term sums of positive numbers in the NMF updates and TV ((T + F + Kb) eps relative, which the
    weights pass on to the covariances one to one); the solve of every row passes that on amplified by
    cond(Q Sigma_n).  The bar takes the largest such condition number of the oracle's last state, once
    per iteration, on filters of order max |W|; the factors are compared relative to their largest
    entry."""
    case = convilrma_cases.CASES[5]
    M, K, D, F, T, _, Kb, _ = case
    assert K == 0
    X = _mixture(case)
    basis, activation = convilrma_cases.make_factors(case)
    out = _run(case, domain=domain, normalization=normalization)
    oracle = GaussILRMAOracle(Kb, spatial_algorithm="IP1", domain=domain,
                              normalization=normalization)
    Y = oracle.run(X, n_iter=N_ITER, basis=basis, activation=activation)
    W = oracle.demix_filter
    U = sp.weighted_covariance(X, oracle._spatial_weight(Y))
    kappa = max(np.linalg.cond(W[f] @ U[f, n]) for f in range(F) for n in range(M))
    bar = N_ITER * 8 * (2 * T + F + Kb + M ** 3) * EPS * kappa * max(1.0, np.abs(W).max())
    figures = (np.abs(out["output"] - Y).max(), np.abs(out["demix_filter"] - W).max(),
               np.abs(out["basis"] - oracle.basis).max() / np.abs(oracle.basis).max(),
               np.abs(out["activation"] - oracle.activation).max() / np.abs(oracle.activation).max(),
               np.abs(np.asarray(out["loss"]) / np.asarray(oracle.loss) - 1).max())
    print("convilrma taps = 0 against the oracle p={} normalization={}: output {:.2e}, filter {:.2e}, "
          "basis {:.2e}, activation {:.2e}, loss {:.2e} (bar {:.1e})".format(
              domain, normalization, *figures, bar))
    assert np.array_equal(out["convolutional_filter"][:, :, 0, :], out["demix_filter"])
    assert out["prediction_filter"].shape == (F, M, 0, M, M)
    assert max(figures) <= bar


def test_restatement_counts_failed_pivots():
    """T = 3 < L = 6 with an all-zero last block: every (bin, source) fails, every row keeps its
    direction (the normalisation scales it)."""
    M, K, D, F, T = 2, 3, 1, 3, 3
    case = (M, K, D, F, T, 1, 2, 2)
    X = convilrma_cases.make_mixture(case)
    basis, activation = convilrma_cases.make_factors(case)
    out = convilrma_numpy.run(X, K, D, n_iter=2, basis=basis, activation=activation,
                              normalization=False, scale_restoration=False)
    assert out["failed"] == F * M
    assert np.array_equal(out["output"], X)
    loaded = convilrma_numpy.run(X, K, D, n_iter=2, basis=basis, activation=activation, loading=1e-6)
    assert loaded["failed"] == 0 and np.all(np.isfinite(loaded["output"]))


# ---- the class: errors raised before anything is uploaded
def test_constructor_errors():
    for kwargs in (dict(n_basis=0), dict(n_basis=1.5), dict(n_basis=True), dict(taps=-1),
                   dict(delay=0), dict(domain=0), dict(domain=2.5), dict(domain=-1),
                   dict(diagonal_loading=-1.0), dict(diagonal_loading=float("nan")),
                   dict(normalization="nothing"), dict(scale_restoration="nothing"),
                   dict(reference_id=None), dict(reference_id=0.5)):
        kwargs.setdefault("n_basis", 2)
        with pytest.raises(ValueError):
            ConvGaussILRMA(**kwargs)
    with pytest.raises(NotImplementedError):
        ConvGaussILRMA(33)
    with pytest.raises(NotImplementedError):
        ConvGaussILRMA(2, normalization="projection_back")
    with pytest.raises(NotImplementedError):
        ConvGaussILRMA(2, scale_restoration="minimal_distortion_principle")
    with pytest.raises(NotImplementedError):
        ConvGaussILRMA(2, flooring_fn=lambda x: np.maximum(x, 1e-3))
    for flooring_fn in (None, identity, max_flooring, add_flooring,
                        functools.partial(add_flooring, eps=1e-8)):
        ConvGaussILRMA(2, flooring_fn=flooring_fn)
    for n_basis in (1, 32):
        ConvGaussILRMA(n_basis, normalization="power")
    assert issubclass(ConvGaussILRMA, ConvIVABase)
    ConvGaussILRMA(2, reference_id=None, scale_restoration=False)


def test_shape_errors_come_before_any_upload():
    zeros = functools.partial(np.zeros, dtype=np.complex128)
    with pytest.raises(ValueError):
        ConvGaussILRMA(2)(zeros((4, 8)))
    with pytest.raises(ValueError):
        ConvGaussILRMA(2)(zeros((2, 0, 8)))
    with pytest.raises(ValueError):
        ConvGaussILRMA(2, reference_id=2)(zeros((2, 3, 8)))
    with pytest.raises(NotImplementedError):
        ConvGaussILRMA(2)(zeros((1, 3, 8)))
    with pytest.raises(NotImplementedError):
        ConvGaussILRMA(2)(zeros((9, 3, 8)))
    with pytest.raises(NotImplementedError):
        ConvGaussILRMA(2, taps=8)(zeros((8, 3, 100)))  # (taps + 1) M = 72
    with pytest.raises(ValueError):
        ConvGaussILRMA(2)(zeros((2, 3, 8)), basis=np.ones((2, 3, 3)))
    with pytest.raises(ValueError):
        ConvGaussILRMA(2)(zeros((2, 3, 8)), activation=np.ones((2, 2, 7)))
    with pytest.raises(ValueError):
        ConvGaussILRMA(2)(zeros((2, 3, 8)), basis=None)
    method = ConvGaussILRMA(2)
    method.n_basis = 40
    with pytest.raises(NotImplementedError):
        method(zeros((2, 3, 8)))
    with pytest.raises(NotImplementedError):
        ConvGaussILRMA(2).apply_minimal_distortion_principle()
    with pytest.raises(NotImplementedError):
        ConvGaussILRMA(2).separate(zeros((2, 3, 8)), zeros((3, 2, 2)))
    with pytest.raises(ValueError):
        ConvGaussILRMA(2).apply(zeros((2, 3, 8)))  # (no call yet)


def test_repr():
    assert repr(ConvGaussILRMA(4)) == (
        "ConvGaussILRMA(n_basis=4, taps=5, delay=3, domain=2, diagonal_loading=0.0, "
        "normalization=True, scale_restoration=True, record_loss=True, reference_id=0)")
    assert repr(ConvGaussILRMA(2, taps=2, delay=1, domain=1, diagonal_loading=1e-6,
                               normalization=False, scale_restoration=False,
                               record_loss=False)) == (
        "ConvGaussILRMA(n_basis=2, taps=2, delay=1, domain=1, diagonal_loading=1e-06, "
        "normalization=False, scale_restoration=False, record_loss=False)")


def test_limits_mirror_the_header():
    import os
    import re

    from conftest import ROOT
    from ssspy_amd import _lib

    text = open(os.path.join(ROOT, "include", "ssspy_amd.h")).read()
    value = int(re.search(r"SSSPY_CONVIVA_MAX_BASIS = (\d+)", text).group(1))
    assert _lib.CONVIVA_MAX_BASIS == value == 32
