"""Pin the NumPy restatement of PDSBSS / MaskingPDSBSS (tests/pdsbss_numpy.py) against the golden
vectors generated from the reference (tests/golden/make_golden_pdsbss.py).

Bars: 1e-8 relative Frobenius on filters, dual variables and outputs, rtol 1e-9 on
loss lists.  The generator checked every fixture to be conditioned 100x better than that.
"""

import warnings

import numpy as np
import pytest

import pdsbss_cases as pc
import pdsbss_numpy as pn
from conftest import load_golden

TOL = 1e-8
LOSS_RTOL = 1e-9


@pytest.mark.parametrize("name", pc.CASES)
def test_restatement_replays_golden(name):
    g = load_golden(name)
    spec = pc.golden_spec(g)
    snap = pc.Snapshots()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        m = pn.CLASSES[spec["cls"]](callbacks=snap, **pc.build_kwargs(spec, pn))
    init = pc.golden_init(g)
    Y = m(g["X"], n_iter=spec["n_iter"], **init)
    pc.check_against_golden(g, m, Y, snap, TOL, LOSS_RTOL)
    if init:  # injected arrays are copied, never mutated
        assert np.array_equal(init["demix_filter"], g["demix_filter0"])
        assert np.array_equal(init["dual"], g["dual0"])


def test_fixtures_hold_what_their_names_promise():
    gs = {name: load_golden(name) for name in pc.CASES}
    for name, g in gs.items():
        spec = pc.golden_spec(g)
        want = pc.spec_of(name)
        assert {k: spec[k] for k in want} == want, name
        N, F, T, n_iter = spec["N"], spec["F"], spec["T"], spec["n_iter"]
        Q = len(spec["penalties"])
        assert N <= 12 and F <= 33 and T <= 200 and n_iter == 10
        assert g["X"].shape == (N, F, T) and g["final_output"].shape == (N, F, T)
        assert g["final_demix_filter"].shape == (F, N, N)
        dual_shape = (N, F, T) if spec["cls"] == "MaskingPDSBSS" else (Q, N, F, T)
        for it in (1, 2, n_iter):
            assert g["it{}_demix_filter".format(it)].shape == (F, N, N)
            assert g["it{}_dual".format(it)].shape == dual_shape
            assert np.linalg.norm(g["it{}_dual".format(it)]) > 0
        assert "n{}".format(N) in name.split("_")
        assert g["loss"].shape == ((n_iter + 1,) if spec["record_loss"] else (0,))
        assert np.isfinite(g["loss"]).all()
        assert ("init" in name) == ("demix_filter0" in g) == ("dual0" in g)
        # the mixture went through normalize_by_spectral_norm: the largest spectral norm of a bin
        norms = np.linalg.svd(g["X"].transpose(1, 0, 2), compute_uv=False)[:, 0]
        np.testing.assert_allclose(np.max(norms) * np.sqrt(Q), 1.0, rtol=1e-12)
    specs = {name: pc.golden_spec(g) for name, g in gs.items()}
    bins = {s["N"] for s in specs.values() if s["penalties"] == ["l21_bins"]}
    assert bins == {2, 3, 4, 8, 10}
    kinds = {tuple(s["penalties"]) for s in specs.values()}
    assert kinds >= {("l1",), ("l21_frames",), ("l21_bins", "l1"), ("elastic",), ("mask",)}
    two = specs["pdsbss_two_n4_mdp_loss"]
    assert (two["mu1"], two["relaxation"], two["record_loss"]) == (0.5, 1.5, True)
    assert two["scale_restoration"] == "minimal_distortion_principle"
    assert specs["pdsbss_masking_n3"]["cls"] == "MaskingPDSBSS"
    init = gs["pdsbss_l21bins_n4_init"]
    assert np.linalg.norm(init["demix_filter0"] - np.eye(4)) > 0.1 and np.linalg.norm(init["dual0"]) > 0
    assert any(s["scale_restoration"] is False for s in specs.values())
    assert any(s["reference_id"] != 0 for s in specs.values())
    assert any(s["alpha"] is not None for s in specs.values())
