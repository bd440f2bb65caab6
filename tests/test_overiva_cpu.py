"""OverIVA without a device: the NumPy restatement (tests/overiva_numpy.py) against the reference's
AuxIVA-IP1 fixtures at n_sources == n_channels, its orthogonality constraint below that, and the
host-side contract of the classes (constructor errors, repr, limits).

Bars.  The determined replay is held to what tests/test_oracle_golden.py asks of the oracle on the
same fixtures: 1e-11 relative (Frobenius) on every snapshot and on the restored filter / output,
1e-10 relative on the loss list.
"""

import functools

import numpy as np
import pytest

import overiva_numpy as on
from conftest import load_golden, rel_err
from conftest import option as _option

TOL = 1e-11
FIXTURES = ["auxlap_ip1_n2", "auxlap_ip1_n4", "auxlap_ip1_n9", "auxgauss_ip1_n3"]


@pytest.mark.parametrize("case", FIXTURES)
def test_determined_case_replays_reference_fixture(case):
    g = load_golden(case)
    assert str(g["meta_algo"]) in ("IP", "IP1")
    n_iter = int(g["meta_n_iter"])
    snaps = {k: {} for k in (1, 2, 10) if k <= n_iter}
    out = on.run(g["X"], n_iter=n_iter, contrast=str(g["meta_contrast"]),
                 flooring=(str(g["meta_floor_kind"]), float(g["meta_floor_eps"])),
                 scale_restoration=_option(g["meta_scale_restoration"]), snapshots=snaps)
    checked = 0
    for k, snap in snaps.items():
        for name in ("demix_filter", "variance"):
            key = "it{}_{}".format(k, name)
            if key in g:
                assert rel_err(snap[name], g[key]) < TOL, key
                checked += 1
    assert checked > 0
    np.testing.assert_allclose(out["loss"], g["loss"], rtol=1e-10)
    assert rel_err(out["demix_filter"], g["final_demix_filter"]) < TOL
    assert rel_err(out["output"], g["final_output"]) < TOL
    assert out["background_filter"].shape == (g["X"].shape[1], 0, g["X"].shape[0])


@pytest.mark.parametrize("case", on.CASES)
@pytest.mark.parametrize("contrast,flooring", [("laplace", ("max", 1e-10)), ("gauss", ("add", 1e-3))])
def test_orthogonality_and_loss(case, contrast, flooring):
    """[J, -I] C W_t^H = 0 after every iteration to 64 M eps ||C|| ||W_t|| per bin.

    The loss of the restatement is NOT non-increasing on the case list, so that is not asserted:
    (8, 2, 65, 70) rises over iterations 2 and 3 with both contrasts (Laplace / max floor: 1136.0,
    213.8, 320.3, 343.4, 329.3, 296.8); the other five cases fall at every iteration.  The N row
    updates each minimise the auxiliary function over their row, but re-forming J afterwards moves
    the trace and the log-determinant terms outside that minimisation.  The loss stays finite."""
    M, N, F, T = case
    X = on.make_mixture(*case)
    out = on.run(X, n_sources=N, n_iter=5, contrast=contrast, flooring=flooring)
    for resid, bound in out["ortho"]:
        assert (resid <= bound).all()
    assert out["demix_filter"].shape == (F, N, M)
    assert out["background_filter"].shape == (F, M - N, N)
    assert out["output"].shape == (N, F, T)
    loss = out["loss"]
    assert np.isfinite(loss).all() and loss.shape == (6,)


def test_step_bins_are_well_conditioned_on_the_elementwise_seeds():
    """The elementwise GPU test of the step kernel runs on bins with cond(W V_n) <= 1e6; its seeds
    are chosen so that the restatement excludes none."""
    for case in on.CASES:
        W, V, C, N = step_operands(case)
        cond = np.linalg.cond(W[:, None] @ V)
        assert cond.max() <= 1e6, (case, cond.max())


def step_operands(case, seed=7):
    """Operands of one step in mid-run: the full filter after two iterations, the next weighted
    covariances, the static covariance.  Shared with tests/test_gpu_overiva.py."""
    M, N, F, T = case
    X = on.make_mixture(M, N, F, T, seed=seed)
    W = on.run(X, n_sources=N, n_iter=2, scale_restoration=False)["full"]
    _, r2 = on.frame_power(X, W[:, :N, :])
    phi, _ = on.weights(r2, F, "laplace", on.DEFAULT_FLOOR)
    return W, on.covariance(X, phi), on.covariance(X), N


# ---------------------------------------------------------------- the classes, host side
def test_exports_and_repr():
    import ssspy_amd.bss as bss
    from ssspy_amd.bss.overiva import OverGaussIVA, OverIVABase, OverLaplaceIVA

    assert bss.OverLaplaceIVA is OverLaplaceIVA and bss.OverGaussIVA is OverGaussIVA
    assert issubclass(OverLaplaceIVA, OverIVABase) and issubclass(OverGaussIVA, OverIVABase)
    assert repr(OverLaplaceIVA(n_sources=2)) == (
        "OverLaplaceIVA(n_sources=2, spatial_algorithm=IP, scale_restoration=True, record_loss=True, "
        "reference_id=0)")
    assert repr(OverGaussIVA(spatial_algorithm="IP1", scale_restoration=False, record_loss=False)) == (
        "OverGaussIVA(n_sources=None, spatial_algorithm=IP1, scale_restoration=False, "
        "record_loss=False)")
    assert OverLaplaceIVA(scale_restoration="projection_back").scale_restoration == "projection_back"


def test_constructor_errors():
    from ssspy_amd.bss.overiva import OverGaussIVA, OverLaplaceIVA
    from ssspy_amd.special.flooring import add_flooring

    for algo in ("IP2", "ISS", "IPA", "nonsense"):
        with pytest.raises(ValueError):
            OverLaplaceIVA(spatial_algorithm=algo)
    with pytest.raises(ValueError):
        OverLaplaceIVA(n_sources=0)
    with pytest.raises(ValueError):
        OverGaussIVA(reference_id=None)
    with pytest.raises(ValueError):
        OverGaussIVA(scale_restoration="nonsense")
    with pytest.raises(NotImplementedError):
        OverLaplaceIVA(scale_restoration="minimal_distortion_principle")
    with pytest.raises(NotImplementedError):
        OverLaplaceIVA(flooring_fn=lambda x: np.maximum(x, 1e-3))
    OverLaplaceIVA(flooring_fn=functools.partial(add_flooring, eps=1e-3))
    OverLaplaceIVA(flooring_fn=None)


def test_limits_are_checked_before_the_device_is_touched():
    from ssspy_amd.bss.overiva import OverLaplaceIVA

    with pytest.raises(NotImplementedError):
        OverLaplaceIVA()(np.zeros((17, 3, 4), dtype=complex), n_iter=1)
    with pytest.raises(NotImplementedError):
        OverLaplaceIVA(n_sources=4)(np.zeros((3, 3, 4), dtype=complex), n_iter=1)
    with pytest.raises(NotImplementedError):
        OverLaplaceIVA(n_sources=1)(np.zeros((1, 3, 4), dtype=complex), n_iter=1)
    with pytest.raises(ValueError):
        OverLaplaceIVA()(np.zeros((3, 4), dtype=complex), n_iter=1)
