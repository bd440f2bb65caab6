"""Pin the NumPy restatement of MaskingADMMHVA (tests/admmhva_numpy.py) against the golden vectors
generated from the reference (tests/golden/make_golden_admmhva.py).

Bar (that of tests/test_golden_admmbss.py): 1e-8 relative Frobenius on filters, states and outputs.
The generator checked every fixture to be conditioned 100x better than that.
"""

import numpy as np
import pytest

import admmbss_cases as ac
import admmhva_cases as hc
import admmhva_numpy as hn
from conftest import load_golden
from test_golden_admmbss import _unstack

TOL = 1e-8


@pytest.mark.parametrize("name", hc.CASES)
def test_restatement_replays_golden(name):
    g = load_golden(name)
    spec = hc.golden_spec(g)
    init = ac.golden_init(g)
    parts = [g] if spec["B"] == 1 else [_unstack(g, b) for b in range(spec["B"])]
    for part in parts:
        snap = ac.Snapshots("MaskingADMMBSS")
        m = hc.construct(hn.CLASSES, hn, spec, callbacks=snap)
        Y = m(part["X"], n_iter=spec["n_iter"], **init)
        ac.check_against_golden(part, m, Y, snap, TOL, None)
        assert m.attenuation == (spec["attenuation"] or 1 / spec["N"])
    for key, value in init.items():  # injected arrays are copied, never mutated
        assert np.array_equal(value, g[key + "0"])


def test_fixtures_hold_what_their_names_promise():
    gs = {name: load_golden(name) for name in hc.CASES}
    specs = {name: hc.golden_spec(g) for name, g in gs.items()}
    for name, g in gs.items():
        spec, want = specs[name], hc.spec_of(name)
        assert {k: spec[k] for k in want} == want, name
        N, F, T, B, n_iter = spec["N"], spec["F"], spec["T"], spec["B"], spec["n_iter"]
        lead = () if B == 1 else (B,)
        assert n_iter == 10 and g["loss"].size == 0  # (no case had to drop to 5 iterations)
        assert g["X"].shape == lead + (N, F, T) == g["final_output"].shape
        np.testing.assert_allclose(np.sqrt(np.mean(np.abs(g["X"]) ** 2, axis=(-3, -2, -1))), ac.RMS,
                                   rtol=1e-12)
        shapes = {"demix_filter": (F, N, N), "auxiliary1": (F, N, N), "dual1": (F, N, N),
                  "auxiliary2": (N, F, T), "dual2": (N, F, T)}
        for it in (1, 2, n_iter):
            for state, shape in shapes.items():
                value = g["it{}_{}".format(it, state)]
                assert value.shape == lead + shape and np.isfinite(value).all()
        assert "n{}".format(N) in name.split("_") and "f{}".format(F) in name.split("_")
        assert ("init" in name) == ("auxiliary10" in g) == spec["inject"]
        if not spec["inject"]:
            # the first iteration from the zero state: W = 0 and so Z = 0 exactly; with a floor the
            # mask is finite there and auxiliary2 = dual2 = 0
            assert spec["flooring"] != "none"
            assert not np.any(g["it1_demix_filter"])
            eye = np.broadcast_to(np.sqrt(1 / spec["rho"]) * np.eye(N), g["it1_auxiliary1"].shape)
            assert np.array_equal(g["it1_auxiliary1"], eye)
            assert not np.any(g["it1_auxiliary2"]) and not np.any(g["it1_dual2"])
        else:
            assert all(np.linalg.norm(g[k + "0"]) > 0 for k in ac.ADMM_STATES)
    assert {s["flooring"] for s in specs.values()} == {"max", "add", "none", "lambda"}
    assert {s["mask_iter"] for s in specs.values()} == {0, 1, 3}
    iter3 = specs["admmhva_n3_f17_iter3"]
    assert (iter3["rho"], iter3["relaxation"], iter3["reference_id"]) == (0.5, 1.5, 1)
    add = specs["admmhva_n3_f6_add_att"]
    assert (add["attenuation"], add["alpha"]) == (0.4, 1.25)
    assert specs["admmhva_n9_f12_none_init_noscale"]["scale_restoration"] is False
    assert specs["admmhva_n2_f12_lambda_mdp"]["scale_restoration"] == "minimal_distortion_principle"
    assert specs["admmhva_n3_f9_batch"]["B"] == 3
    # both transform routes and the run-time source count are among the shapes
    assert {(s["F"] - 1) & (s["F"] - 2) == 0 for s in specs.values()} == {True, False}
    assert max(s["N"] for s in specs.values()) > 8
