"""Pin the NumPy restatement of the time-domain ICA classes (tests/ica_numpy.py) against the golden
vectors generated from the reference (tests/golden/make_golden_ica.py).

The restatement is written from the formulas, so it replays the reference to rounding only: 1e-10
relative Frobenius on filters, snapshots and outputs and on the loss lists (the generator checked
every fixture to move by less than 1e-10 under a 1e-15 perturbation of its input; the measured
distances are 1e-15 .. 1e-12).
"""

import numpy as np
import pytest

import ica_numpy as inp
from conftest import load_golden, rel_err
from ica_cases import CASES, Snapshots, check_against_golden, golden_init, golden_kwargs

TOL = 1e-10


@pytest.mark.parametrize("name", CASES)
def test_restatement_replays_golden(name):
    g = load_golden(name)
    n_iter = int(g["meta_n_iter"])
    snap = Snapshots(n_iter)
    m = inp.CLASSES[str(g["meta_cls"])](callbacks=snap, **golden_kwargs(g))
    init = golden_init(g)
    Y = m(g["X"], n_iter=n_iter, **init)
    check_against_golden(g, m, Y, snap, TOL, TOL, report=name)
    if "whitened_input" in g:
        assert rel_err(m.whitened_input, g["whitened_input"]) < TOL
    if init:  # injected filters are copied, never mutated
        assert np.array_equal(init["demix_filter"], g["demix_filter0"])


def test_fixtures_hold_what_the_issue_lists():
    gs = {name: load_golden(name) for name in CASES}
    for name, g in gs.items():
        N, T = (int(v) for v in g["meta_shape"])
        n_iter = int(g["meta_n_iter"])
        assert str(g["meta_kind"]) == "ica" and n_iter == 10
        assert g["X"].shape == (N, T) and g["final_output"].shape == (N, T)
        assert g["final_demix_filter"].shape == (N, N)
        assert g["loss"].shape == (n_iter + 1,) and np.isfinite(g["loss"]).all()
        for key in ("it1_demix_filter", "it2_demix_filter", "itlast_demix_filter"):
            assert g[key].shape == (N, N)
        assert np.array_equal(g["itlast_demix_filter"], g["final_demix_filter"])
        assert "n{}".format(N) in name.split("_")
        if str(g["meta_cls"]) != "FastICA":
            assert ("hol" in name.split("_")) == bool(g["meta_is_holonomic"])
        assert ("fast" in name.split("_")) == ("whitened_input" in g)
    assert {str(g["meta_cls"]) for g in gs.values()} == {
        "GradICA", "NaturalGradICA", "FastICA", "GradLaplaceICA", "NaturalGradLaplaceICA"}
    for cls in ("GradLaplaceICA", "NaturalGradLaplaceICA", "GradICA", "NaturalGradICA"):
        assert {bool(g["meta_is_holonomic"]) for g in gs.values() if str(g["meta_cls"]) == cls} == {
            True, False}, cls
    assert {int(g["meta_shape"][0]) for g in gs.values()} == {2, 3, 4, 8, 16}
    by_cls = {}
    for g in gs.values():
        by_cls.setdefault(str(g["meta_cls"]), set()).add(str(g["meta_nonlinearity"]))
    assert by_cls["FastICA"] == {"logistic", "logcosh", "closure"}
    assert "closure" in by_cls["GradICA"] and "closure" in by_cls["NaturalGradICA"]
    assert {"logistic", "logcosh"} <= by_cls["GradICA"] | by_cls["NaturalGradICA"]
    # an injected filter that is not the identity
    injected = [g for g in gs.values() if "demix_filter0" in g]
    assert injected and all(
        not np.allclose(g["demix_filter0"], np.eye(len(g["demix_filter0"]))) for g in injected)
    # a run of exactly zero samples: sign(0) = 0 enters the sums
    g = gs["ica_glap_n4_zeros"]
    a, b = (int(v) for v in g["meta_zero_run"])
    assert b - a >= 8 and not g["X"][:, a:b].any() and not g["final_output"][:, a:b].any()
