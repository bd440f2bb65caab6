"""FastIVA / FasterIVA and whiten / pca on the CPU: the NumPy restatement (tests/fast_iva_numpy.py)
replays every reference fixture at 1e-11 -- the bar of test_golden_grad_iva.py -- in the phase gauge
the fixture records (its ``whitened_input``), and the fixtures hold what their names promise."""

import numpy as np
import pytest

import fast_iva_cases as fc
import fast_iva_numpy as fn
from conftest import load_golden, option

TOL = 1e-11


def replay(name, module=fn, gauge_like="fixture", regauge=None):
    """The restatement on the fixture's input; returns (method, snapshots, output, fixture)."""
    g = load_golden(name)
    cfg = fc.settings(name)
    snap = fc.ActionSnapshots()
    like = g["whitened_input"] if isinstance(gauge_like, str) else gauge_like
    m = module.CLASSES[cfg["cls"]](flooring_fn=fc.flooring_for(cfg["flooring"], module),
                                   callbacks=snap, scale_restoration=cfg["scale_restoration"],
                                   reference_id=cfg["reference_id"], gauge_like=like,
                                   **fc.closures_for(cfg["cls"], cfg["contrast"]))
    init = {}
    if cfg["init_filter"]:
        W0 = g["demix_filter0"]
        init["demix_filter"] = W0 if regauge is None else fc.regauge_filter(W0, regauge)
    Y = m(g["X"], n_iter=int(g["meta_n_iter"]), **init)
    return m, snap, Y, g


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_restatement_replays_fixture(name):
    m, snap, Y, g = replay(name)
    assert fc.err(m.whitened_input, g["whitened_input"]) <= TOL
    np.testing.assert_allclose(m.loss, g["loss"], rtol=TOL)
    for key in ("it1_action", "it2_action"):
        assert fc.err_up_to_row_phase(snap.store[key], g[key]) <= TOL, key
    if fc.settings(name)["scale_restoration"]:
        assert fc.err(fc.filter_action(m), g["final_action"]) <= TOL
        assert fc.err(Y, g["final_output"]) <= TOL
    else:
        assert fc.err_up_to_row_phase(fc.filter_action(m), g["final_action"]) <= TOL
        assert fc.err_up_to_row_phase(Y, g["final_output"]) <= TOL


def test_fixtures_hold_what_their_names_promise():
    seen = dict(sources=set(), floors=set(), restoration=set(), contrast=set())
    for name in fc.CASES:
        g, cfg = load_golden(name), fc.settings(name)
        N, F, T = cfg["shape"]
        assert g["X"].shape == (N, F, T) and tuple(g["meta_shape"]) == (N, F, T)
        assert str(g["meta_cls"]) == cfg["cls"] and name.startswith(cfg["cls"].lower())
        assert option(g["meta_scale_restoration"]) == cfg["scale_restoration"]
        assert int(g["meta_reference_id"]) == cfg["reference_id"]
        assert (str(g["meta_floor_kind"]), float(g["meta_floor_eps"])) == cfg["flooring"]
        assert ("demix_filter0" in g) == cfg["init_filter"]
        n_iter = int(g["meta_n_iter"])
        assert 2 <= n_iter <= 10 and g["loss"].shape == (n_iter + 1,)
        # the reference's own movement under a 2^-50 perturbation: 1/100 of the device's 1e-8 bar
        assert float(g["meta_ref_movement"]) <= 1e-10
        assert float(g["meta_min_gap"]) >= 1e-3
        assert float(g["meta_max_cond"]) <= 1e6
        C = fn.covariance(g["X"])
        assert np.max(np.linalg.cond(C)) <= 1e6
        if cfg["flooring"][0] == "max" and cfg["flooring"][1] > 1e-6:
            r2 = 2 * np.linalg.norm(g["whitened_input"], axis=1)
            assert 0 < np.sum(r2 < cfg["flooring"][1]) < r2.size
        seen["sources"].add(N)
        seen["floors"].add(cfg["flooring"][0])
        seen["restoration"].add(cfg["scale_restoration"])
        seen["contrast"].add((cfg["cls"], cfg["contrast"]))
    assert seen["sources"] == {2, 3, 4, 8, 9, 16}
    assert seen["floors"] == {"max", "add", "custom", "none"}
    assert seen["restoration"] == {False, True, "projection_back", "minimal_distortion_principle"}
    assert seen["contrast"] == {(c, k) for c in ("FastIVA", "FasterIVA") for k in fc.CLOSURES}
    assert any(fc.settings(n)["reference_id"] for n in fc.CASES)


@pytest.mark.parametrize("key", ["c3", "c4", "r2", "r3"])
def test_restated_transforms_replay_fixture(key):
    g = load_golden(fc.TRANSFORM_FIXTURE)
    x = g["x_" + key]
    single = [x] if x.ndim == (3 if np.iscomplexobj(x) else 2) else list(x)
    for b, xb in enumerate(single):
        for name, got in (("whiten_", fn.whiten(xb)), ("pca_ascend_", fn.pca(xb, ascend=True)),
                          ("pca_descend_", fn.pca(xb, ascend=False))):
            want = g[name + key] if len(single) == 1 and x is single[0] else g[name + key][b]
            assert fc.err_up_to_row_phase(got, want) <= TOL, (name, b)


def test_restatement_is_gauge_covariant():
    """Another phase choice in the whitening carries through: the loss and the restored output of
    projection back do not move, the unrestored output moves by a phase per (source, bin)."""
    for name in ("fastiva_n3_smooth_add", "fasteriva_n16", "fastiva_n4_init_pb"):
        g = load_golden(name)
        rng = np.random.default_rng(3)
        D = np.exp(2j * np.pi * rng.random(g["whitened_input"].shape[:2][::-1]))  # (F, N)
        like = D.T[:, :, np.newaxis] * g["whitened_input"]
        m, _, Y, _ = replay(name, gauge_like=like, regauge=D)
        np.testing.assert_allclose(m.loss, g["loss"], rtol=1e-10)
        assert fc.err_up_to_row_phase(Y, g["final_output"]) <= 1e-10
        if fc.settings(name)["scale_restoration"]:
            assert fc.err(Y, g["final_output"]) <= 1e-10
