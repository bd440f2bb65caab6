"""Pin the NumPy restatement of ADMMBSS / MaskingADMMBSS / ADMMIVA / PDSIVA (tests/admmbss_numpy.py)
against the golden vectors generated from the reference (tests/golden/make_golden_admmbss.py).

Bars (those of tests/test_golden_pdsbss.py): 1e-8 relative Frobenius on filters, states and outputs,
rtol 1e-9 on the finite loss entries; the non-finite ones by position and sign.  The generator
checked every fixture to be conditioned 100x better than that.
"""

import warnings

import numpy as np
import pytest

import admmbss_cases as ac
import admmbss_numpy as an
from conftest import load_golden

TOL = 1e-8
LOSS_RTOL = 1e-9


def _unstack(g, b):
    """Mixture b of a batched fixture as a single one."""
    out = {}
    for k, v in g.items():
        if k.startswith("meta_"):
            out[k] = v
        else:
            out[k] = v[:, b] if k == "loss" else v[b]
    return out


@pytest.mark.parametrize("name", ac.CASES)
def test_restatement_replays_golden(name):
    g = load_golden(name)
    spec = ac.golden_spec(g)
    init = ac.golden_init(g)
    parts = [g] if spec["B"] == 1 else [_unstack(g, b) for b in range(spec["B"])]
    for part in parts:
        snap = ac.Snapshots(spec["cls"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            m = an.CLASSES[spec["cls"]](callbacks=snap, **ac.build_kwargs(spec, an))
        Y = m(part["X"], n_iter=spec["n_iter"], **init)
        ac.check_against_golden(part, m, Y, snap, TOL, LOSS_RTOL)
    for key, value in init.items():  # injected arrays are copied, never mutated
        assert np.array_equal(value, g[key + "0"])


def test_fixtures_hold_what_their_names_promise():
    gs = {name: load_golden(name) for name in ac.CASES}
    specs = {name: ac.golden_spec(g) for name, g in gs.items()}
    for name, g in gs.items():
        spec, want = specs[name], ac.spec_of(name)
        assert {k: spec[k] for k in want} == want, name
        N, F, T, B, n_iter = spec["N"], spec["F"], spec["T"], spec["B"], spec["n_iter"]
        lead = () if B == 1 else (B,)
        assert F <= 33 and T <= 64 and n_iter <= 10
        assert g["X"].shape == lead + (N, F, T) == g["final_output"].shape
        np.testing.assert_allclose(np.sqrt(np.mean(np.abs(g["X"]) ** 2, axis=(-3, -2, -1))), ac.RMS,
                                   rtol=1e-12)
        Q = max(len(spec["penalties"]), 1)
        big = (N, F, T) if spec["cls"] == "MaskingADMMBSS" else (Q, N, F, T)
        shapes = {"demix_filter": (F, N, N), "auxiliary1": (F, N, N), "dual1": (F, N, N),
                  "auxiliary2": big, "dual2": big, "dual": big}
        for it in (1, 2, n_iter):
            for state in ("demix_filter",) + ac.state_names(spec["cls"]):
                assert g["it{}_{}".format(it, state)].shape == lead + shapes[state]
        assert "n{}".format(N) in name.split("_")
        assert g["loss"].shape == ((n_iter + 1,) + lead if spec["record_loss"] else (0,))
        assert ("init" in name) == ("auxiliary10" in g)
        if spec["cls"] != "PDSIVA" and not spec["inject"]:
            # the first iteration from the zero state: W = 0 exactly, auxiliary1 = sqrt(1 / rho) I
            # exactly, and the loss there is +inf
            assert not np.any(g["it1_demix_filter"])
            eye = np.broadcast_to(np.sqrt(1 / spec["rho"]) * np.eye(N), g["it1_auxiliary1"].shape)
            assert np.array_equal(g["it1_auxiliary1"], eye)
            assert np.array_equal(g["it1_dual1"], -eye)
            if g["loss"].size:
                assert np.all(g["loss"][1] == np.inf)
                assert np.isfinite(np.delete(g["loss"], 1, axis=0)).all()
        else:
            assert np.isfinite(g["loss"]).all()
    bins = {s["N"] for s in specs.values() if s["penalties"] == ["l21_bins"]}
    assert bins >= {2, 3, 4, 8, 10}
    kinds = {tuple(s["penalties"]) for s in specs.values()}
    assert kinds >= {("l1",), ("l21_frames",), ("l21_sources",), ("l21_bins", "l1"), ("elastic",),
                     ("mask",)}
    two = specs["admmbss_two_n4_mdp_loss"]
    assert two["record_loss"] is True
    assert two["scale_restoration"] == "minimal_distortion_principle"
    relax = specs["admmbss_l21bins_n3_relax"]
    assert (relax["relaxation"], relax["rho"]) == (1.5, 0.5)
    assert specs["admmbss_l21frames_n3_alpha"]["alpha"] is not None
    assert specs["admmbss_masking_n3"]["cls"] == "MaskingADMMBSS"
    assert {(s["cls"], s["user"]) for s in specs.values() if s["cls"].endswith("IVA")} == {
        ("ADMMIVA", False), ("ADMMIVA", True), ("PDSIVA", False), ("PDSIVA", True)}
    assert specs["admmbss_l21bins_n3_batch"]["B"] == 3
    init = gs["admmbss_l21bins_n4_init"]
    assert all(np.linalg.norm(init[k + "0"]) > 0 for k in ac.ADMM_STATES)
    assert any(s["scale_restoration"] is False for s in specs.values())
    assert any(s["reference_id"] != 0 for s in specs.values())
