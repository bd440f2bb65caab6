"""Pin the NumPy restatement of the FDICA classes (tests/fdica_numpy.py) against the golden vectors
generated from the reference (tests/golden/make_golden_fdica.py).

Bars: 1e-8 relative Frobenius on filters and outputs, rtol 1e-9 on loss lists.
The generator checked every fixture to be conditioned 100x better than that (see its docstring).
"""

import numpy as np
import pytest

import fdica_numpy as fn
from conftest import load_golden
from fdica_cases import CASES, Snapshots, check_against_golden, golden_init, golden_kwargs

TOL = 1e-8
LOSS_RTOL = 1e-9


@pytest.mark.parametrize("name", CASES)
def test_restatement_replays_golden(name):
    g = load_golden(name)
    snap = Snapshots()
    m = fn.CLASSES[str(g["meta_cls"])](callbacks=snap, **golden_kwargs(g, fn))
    init = golden_init(g)
    Y = m(g["X"], n_iter=int(g["meta_n_iter"]), **init)
    check_against_golden(g, m, Y, snap, TOL, LOSS_RTOL)
    if init:  # injected filters are copied, never mutated
        assert np.array_equal(init["demix_filter"], g["demix_filter0"])


def test_fixtures_hold_what_their_names_promise():
    gs = {name: load_golden(name) for name in CASES}
    for name, g in gs.items():
        N, F, T = (int(v) for v in g["meta_shape"])
        n_iter = int(g["meta_n_iter"])
        assert N <= 12 and F <= 33 and T <= 300
        assert g["X"].shape == (N, F, T) and g["final_output"].shape == (N, F, T)
        assert g["final_demix_filter"].shape == (F, N, N)
        assert g["loss"].shape == (n_iter + 1,) and np.isfinite(g["loss"]).all()
        for it in (1, 2, n_iter):
            assert g["it{}_demix_filter".format(it)].shape == (F, N, N)
        assert "n{}".format(N) in name.split("_")
        aux = "Aux" in str(g["meta_cls"])
        ip2 = aux and str(g["meta_spatial_algorithm"]) == "IP2"
        assert n_iter == (5 if ip2 else 10)
        assert ("ip2" in name.split("_")) == ip2
        if not aux and "generic" not in name:
            assert ("hol" in name.split("_")) == bool(g["meta_is_holonomic"])
        assert ("init" in name or "generic_grad" in name) == ("demix_filter0" in g)
        assert ("noperm" in name) == (not bool(g["meta_permutation_alignment"]))
    assert {str(g["meta_cls"]) for g in gs.values()} == {
        "GradLaplaceFDICA", "NaturalGradLaplaceFDICA", "AuxLaplaceFDICA", "GradFDICA", "AuxFDICA"}
    for cls in ("GradLaplaceFDICA", "NaturalGradLaplaceFDICA"):
        assert {bool(g["meta_is_holonomic"]) for g in gs.values() if str(g["meta_cls"]) == cls} == {
            True, False}, cls
    sizes = {int(g["meta_shape"][0]) for g in gs.values()}
    assert {2, 3, 4, 8} <= sizes and any(9 <= n <= 12 for n in sizes)
    assert {str(g["meta_floor_kind"]) for g in gs.values()} >= {"max", "add", "none", "custom"}
    assert {str(g["meta_pair_selector"]) for g in gs.values()} == {"sequential", "combination"}
    restorations = {str(g["meta_scale_restoration"]) for g in gs.values()}
    assert restorations >= {"False", "True", "projection_back", "minimal_distortion_principle"}
    assert any(int(g["meta_reference_id"]) != 0 for g in gs.values())
    # the max floor of fdica_nglap_n3_hol_maxfloor acts: magnitudes on both sides of it
    g = gs["fdica_nglap_n3_hol_maxfloor"]
    assert 0.05 < np.mean(np.abs(g["X"]) < float(g["meta_floor_eps"])) < 0.95
