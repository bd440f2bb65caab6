"""Pin the NumPy restatement of the gradient IVA classes (tests/grad_iva_numpy.py) against the golden
vectors generated from the reference (tests/golden/make_golden_grad_iva.py).

The restatement follows the reference's expression structure, so the filters after 1 / 2 / 10
iterations, the loss list and the output agree to ~1e-12 relative (Frobenius); the bar is the one of
tests/test_oracle_golden.py.
"""

import numpy as np
import pytest

import grad_iva_numpy as gn
from conftest import load_golden
from grad_iva_cases import CASES, Snapshots, check_against_golden, golden_init, golden_kwargs

TOL = 1e-11


@pytest.mark.parametrize("name", CASES)
def test_restatement_replays_golden(name):
    g = load_golden(name)
    snap = Snapshots()
    m = gn.CLASSES[str(g["meta_cls"])](callbacks=snap, **golden_kwargs(g, gn))
    init = golden_init(g)
    Y = m(g["X"], n_iter=int(g["meta_n_iter"]), **init)
    check_against_golden(g, m, Y, snap, TOL, TOL)
    if init:  # injected filters are copied, never mutated
        assert np.array_equal(init["demix_filter"], g["demix_filter0"])


def test_fixtures_hold_what_their_names_promise():
    gs = {name: load_golden(name) for name in CASES}
    for name, g in gs.items():
        N, F, T = (int(v) for v in g["meta_shape"])
        n_iter = int(g["meta_n_iter"])
        assert g["X"].shape == (N, F, T) and g["final_output"].shape == (N, F, T)
        assert g["final_demix_filter"].shape == (F, N, N)
        assert g["loss"].shape == (n_iter + 1,) and np.isfinite(g["loss"]).all()
        for it in (1, 2, 10):
            assert ("it{}_demix_filter".format(it) in g) == (it <= n_iter), (name, it)
            if it <= n_iter:
                assert g["it{}_demix_filter".format(it)].shape == (F, N, N)
                assert ("it{}_variance".format(it) in g) == ("Gauss" in str(g["meta_cls"]))
        assert "n{}".format(N) in name.split("_")
        assert ("nonhol" in name) == (not bool(g["meta_is_holonomic"]))
        assert ("init" in name or "generic" in name) == ("demix_filter0" in g)
        tag = {"GradLaplaceIVA": "glap", "GradGaussIVA": "ggauss", "NaturalGradLaplaceIVA": "nglap",
               "NaturalGradGaussIVA": "ngauss", "NaturalGradIVA": "generic"}[str(g["meta_cls"])]
        assert tag in name.split("_")
    # between them: the four named classes and a generic one, both update types, the source counts,
    # the floors, a non-default step, the three scale restorations with a non-zero reference
    assert {str(g["meta_cls"]) for g in gs.values()} == {
        "GradLaplaceIVA", "GradGaussIVA", "NaturalGradLaplaceIVA", "NaturalGradGaussIVA",
        "NaturalGradIVA"}
    for cls in ("GradLaplaceIVA", "GradGaussIVA", "NaturalGradLaplaceIVA", "NaturalGradGaussIVA"):
        assert {bool(g["meta_is_holonomic"]) for g in gs.values() if str(g["meta_cls"]) == cls} == {
            True, False}, cls
    sizes = {int(g["meta_shape"][0]) for g in gs.values()}
    assert {2, 3, 4, 6, 8} <= sizes and any(9 <= n <= 16 for n in sizes)
    assert {str(g["meta_floor_kind"]) for g in gs.values()} >= {"max", "add", "custom"}
    assert any(float(g["meta_step_size"]) != 0.1 for g in gs.values())
    restorations = {str(g["meta_scale_restoration"]) for g in gs.values()}
    assert restorations >= {"False", "True", "projection_back", "minimal_distortion_principle"}
    assert any(int(g["meta_reference_id"]) != 0 for g in gs.values())
    # the max floor of gradiva_glap_n3_nonhol_maxfloor acts: norms on both sides of it
    g = gs["gradiva_glap_n3_nonhol_maxfloor"]
    r = np.linalg.norm(g["X"], axis=1)
    eps = float(g["meta_floor_eps"])
    assert 0.05 < np.mean(r < eps) < 0.95
