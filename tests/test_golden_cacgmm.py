"""The NumPy restatement of CACGMM and the host permutation solvers against the reference's
fixtures (tests/golden/cacgmm_*.npz, written by tests/golden/make_golden_cacgmm.py).  CPU only.

Parameters and outputs to 1e-9 (collapsed covariances to 5e-7, the reference's own movement),
losses to rtol 1e-8, permutations exactly."""

import numpy as np
import pytest

import cacgmm_numpy as cn
from conftest import load_golden
from ssspy_amd.algorithm.permutation_alignment import (
    correlation_based_permutation_solver,
    score_based_permutation_solver,
)


def golden_options(g):
    kind = str(g["meta_floor_kind"])
    pa = str(g["meta_permutation_alignment"])
    return dict(
        n_sources=int(g["meta_n_sources"]),
        flooring=None if kind == "none" else (kind, float(g["meta_floor_eps"])),
        normalization=bool(g["meta_normalization"]),
        permutation_alignment={"True": True, "False": False}.get(pa, pa),
        reference_id=int(g["meta_reference_id"]),
        global_iter=int(g["meta_global_iter"]),
        local_iter=int(g["meta_local_iter"]),
    )


def host_score(seq, *args, **kw):
    out = score_based_permutation_solver(seq, *args, overwrite=False, **kw)
    return out[0], list(out[1])


def host_correlation(seq, *args, **kw):
    out = correlation_based_permutation_solver(seq, *args, overwrite=False, **kw)
    return out[0], list(out[1])


@pytest.fixture(scope="module", params=sorted(cn.GOLDEN))
def replay(request):
    g = load_golden(request.param)
    opts = golden_options(g)
    return g, opts, cn.run(g["input"], np.random.default_rng(0), **opts)


def test_restatement_matches_reference(replay):
    g, opts, r = replay
    assert np.abs(r["mixing"] - g["mixing"]).max() <= 1e-9
    assert np.abs(r["final_mixing"] - g["final_mixing"]).max() <= 1e-9
    # Covariances that collapsed onto single frames (condition number above 1e6 at some iteration)
    # move by 1e-8..5e-7 under a 1e-15 perturbation of the input in the reference itself (measured
    # with the reference on these mixtures), so 1e-9 holds where the reference stayed well
    # conditioned and the collapsed pairs are held to the upper end of the reference's own
    # movement, 5e-7 (seen: 5.6e-9 on cacgmm_acorr_m5_n3), and to their structure.
    cond = np.linalg.cond(g["covariance"])
    keep = (cond < 1e6).all(axis=0)
    assert keep.mean() >= 0.75
    diff = np.abs(r["covariance"] - g["covariance"]).max(axis=(-2, -1))
    assert diff[:, keep].max() <= 1e-9
    if not keep.all():
        assert diff[:, ~keep].max() <= 5e-7
        cov = r["covariance"][-1][~keep]
        assert np.abs(cov - cov.swapaxes(-2, -1).conj()).max() <= 1e-15
        if opts["normalization"]:
            assert np.abs(np.trace(cov, axis1=-2, axis2=-1).real - 1).max() <= 1e-12
        assert np.linalg.eigvalsh(cov).min() > 0
    np.testing.assert_allclose(r["loss"], g["loss"], rtol=1e-8)
    assert len(g["loss"]) == cn.N_ITER + 1
    assert np.abs(r["posterior"] - g["posterior"]).max() <= 1e-9
    assert np.abs(r["output"] - g["output"]).max() <= 1e-9


def test_host_solvers_choose_the_same_permutations(replay):
    g, opts, r = replay
    if not opts["permutation_alignment"]:
        return  # (a fixture without permutation alignment)
    X = g["input"]
    fn = cn.flooring_of(opts["flooring"])
    Z = cn.unit_input(X, fn)
    gamma = cn.e_step(Z, r["mixing"][-1], r["covariance"][-1], fn)
    alpha, B, post, perm = cn.align(X, r["mixing"][-1], r["covariance"][-1], gamma,
                                    opts["permutation_alignment"], opts["reference_id"],
                                    opts["global_iter"], opts["local_iter"], fn,
                                    score=host_score, correlation=host_correlation)
    assert np.array_equal(perm, r["permutation"])
    assert np.abs(post - g["posterior"]).max() <= 1e-9
    assert np.abs(alpha - g["final_mixing"]).max() <= 1e-9
    keep = (np.linalg.cond(g["final_covariance"]) < 1e6)
    diff = np.abs(B - g["final_covariance"]).max(axis=(-2, -1))
    assert diff[keep].max() <= 1e-9
    assert diff.max() <= 5e-7  # (the collapsed pairs: see test_restatement_matches_reference)
