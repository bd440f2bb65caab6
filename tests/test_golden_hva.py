"""Pin the NumPy restatement of MaskingPDSHVA / HVA (tests/hva_numpy.py) against the golden vectors
generated from the reference (tests/golden/make_golden_hva.py).

Bars: 1e-8 relative Frobenius on filters, dual variables and outputs; the
generator checked every fixture to be conditioned 100x better than that.  The mask on its own and its
intermediate varrho: 1e-12 (the restatement sums the DCT-I as a matrix product of at most 12 terms
where the reference runs a real FFT; the DESIGN bar of single operators is 1e-10).
"""

import numpy as np
import pytest

import hva_cases as hc
import hva_numpy as hn
import pdsbss_cases as pc
from conftest import load_golden, rel_err

TOL = 1e-8
MASK_TOL = 1e-12


@pytest.mark.parametrize("name", hc.CASES)
def test_restatement_replays_golden(name):
    g = load_golden(name)
    spec = hc.golden_spec(g)
    snap = pc.Snapshots()
    m = hc.construct(hn.CLASSES, hn, spec, callbacks=snap)
    init = pc.golden_init(g)
    Y = m(g["X"], n_iter=spec["n_iter"], **init)
    pc.check_against_golden(g, m, Y, snap, TOL, None)
    if init:  # injected arrays are copied, never mutated
        assert np.array_equal(init["demix_filter"], g["demix_filter0"])
        assert np.array_equal(init["dual"], g["dual0"])


def test_restated_mask_matches_the_references():
    g = load_golden("hva_mask")
    gamma, mask_iter = float(g["meta_attenuation"]), int(g["meta_mask_iter"])
    for F in hc.MASK_BINS:
        Z = g["Z_f{}".format(F)]
        assert np.array_equal(Z, hc.mask_input(F))
        varrho = hn.varrho(Z, hn.max_flooring, mask_iter)
        assert rel_err(varrho, g["varrho_f{}".format(F)]) < MASK_TOL
        for mask in (hn.mask_of(varrho, gamma), hn.stable_mask_of(varrho, gamma)):
            assert rel_err(mask, g["mask_f{}".format(F)]) < MASK_TOL
        extended = hn.varrho(Z, hn.max_flooring, mask_iter, dtype=np.longdouble)
        assert rel_err(extended.astype(np.float64), g["varrho_f{}".format(F)]) < MASK_TOL


def test_fixtures_hold_what_their_names_promise():
    gs = {name: load_golden(name) for name in hc.CASES}
    specs = {name: hc.golden_spec(g) for name, g in gs.items()}
    for name, g in gs.items():
        spec, want = specs[name], hc.spec_of(name)
        assert {k: spec[k] for k in want} == want, name
        N, F, T, n_iter = spec["N"], spec["F"], spec["T"], spec["n_iter"]
        assert N <= 12 and F <= 33 and T <= 64 and n_iter == 10
        assert "n{}".format(N) in name.split("_") and "f{}".format(F) in name.split("_")
        assert g["X"].shape == g["final_output"].shape == (N, F, T)
        assert g["final_demix_filter"].shape == (F, N, N) and g["loss"].shape == (0,)
        for it in (1, 2, n_iter):
            assert g["it{}_demix_filter".format(it)].shape == (F, N, N)
            assert g["it{}_dual".format(it)].shape == (N, F, T)
            assert np.linalg.norm(g["it{}_dual".format(it)]) > 0
        assert ("init" in name) == ("demix_filter0" in g) == ("dual0" in g)
        norms = np.linalg.svd(g["X"].transpose(1, 0, 2), compute_uv=False)[:, 0]
        np.testing.assert_allclose(np.max(norms), 1.0, rtol=1e-12)
    assert {s["N"] for s in specs.values()} >= {2, 3, 4} and any(
        9 <= s["N"] <= 16 for s in specs.values())
    bins = {s["F"] for s in specs.values()}
    assert bins >= {9, 17, 33, 6, 12}
    assert {s["mask_iter"] for s in specs.values()} == {0, 1, 3}
    assert {s["flooring"] for s in specs.values()} == {"max", "add", "none", "lambda"}
    assert any(s["attenuation"] is not None for s in specs.values())
    assert any(s["relaxation"] != 1 for s in specs.values())
    assert {s["scale_restoration"] for s in specs.values()} >= {False, "minimal_distortion_principle"}
    assert {s["cls"] for s in specs.values()} == {"MaskingPDSHVA", "HVA"}
    init = gs["hva_n4_f33_iter0_init"]
    assert np.linalg.norm(init["demix_filter0"] - np.eye(4)) > 0.1 and np.linalg.norm(init["dual0"]) > 0
