"""tests/gmnmf_reference.py on the CPU: the float64 restatement meets every bar at every shape family
of tests/test_gpu_gmnmf_pass_elementwise.py (the bars are attainable), the solve constants are 8 x
what that restatement measures, and seven mutants of it each break a bar (the bars notice)."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmnmf_reference as gr  # noqa: E402
import mnmf_reference as mr  # noqa: E402
import pass_reference as pr  # noqa: E402

LD, U = pr.LD, pr.U
MAXF, ADDF, NOF = (pr.FLOOR_MAX, pr.EPS), (pr.FLOOR_ADD, pr.EPS), (pr.FLOOR_NONE, 0.0)
C0F = (pr.FLOOR_ADD, 0.05)  # the floor family in which c0 of the floored x x^H is visible

# (B, N, M, F, T, K, partitioning, flooring): one small member of every family of the GPU test --
# forms (full / packed 4 / packed 8 / wide; the floors), a basis form beyond the registers, chunked
# activation sums, partitioning on both sides of max(F, T), the large-K LDS shapes, the c0 family
FAMILIES = [(2, 1, 2, 9, 40, 3, 0, MAXF), (2, 5, 3, 9, 40, 3, 0, ADDF), (2, 4, 4, 9, 129, 3, 0, NOF),
            (2, 9, 6, 9, 40, 3, 0, MAXF), (2, 16, 8, 9, 40, 3, 0, ADDF), (1, 2, 2, 5, 513, 9, 0, MAXF),
            (1, 1, 2, 17, 40, 9, 0, MAXF), (2, 3, 4, 9, 40, 9, 1, MAXF), (2, 9, 7, 40, 9, 3, 1, MAXF),
            (1, 8, 2, 2, 3, 800, 0, MAXF), (2, 3, 3, 9, 40, 3, 0, C0F)]


def _state(fam):
    B, N, M, F, T, K, part, flooring = fam
    return gr.gen_state(B * 7 + N * 5 + M * 11 + F * 3 + T * 2 + K, B, N, M, F, T, K, bool(part)), flooring


def _inside(a, ref, bar):
    err = np.abs(np.asarray(a).astype(ref.dtype) - ref)
    return float(np.max(err / bar))


def _outputs(st, flooring, dtype, mutant=None, pt=None):
    """Every entry of the restatement as name -> (value, bar or None)."""
    X, basis, act, H, z = st
    args = (X, basis, act, H, flooring, z)
    kw = dict(dtype=dtype, mutant=mutant, pt=pt)
    out = {"basis": gr.update_basis(*args, **kw), "activation": gr.update_activation(*args, **kw)}
    P, barP, Q, barQ, _ = gr.spatial_sums(*args, **kw)
    out["P"], out["Q"] = (P, barP), (Q, barQ)
    Hn, _, _, kap = gr.update_spatial(*args, **kw)
    out["spatial"] = (Hn, kap)
    if z is not None:
        out["latent"] = gr.update_latent(*args, **kw)
    else:
        v, bar, _ = gr.loss(X, basis, act, H, flooring, **kw)
        out["loss"] = (v, bar)
        Y, p = gr.separate(X, basis, act, H, X.shape[1] - 1, flooring, **kw)
        out["separate"] = (Y, p.kappa)
    return out


def _ratios(st, flooring, mutant=None):
    """error / bar of the (mutated) float64 restatement against the long-double one, per entry."""
    ref = _outputs(st, flooring, LD)
    got = _outputs(st, flooring, np.float64, mutant)
    r = {}
    for k in ref:
        if k == "spatial":
            r[k] = gr.spatial_error(got[k][0], ref[k][0], ref[k][1]) / gr.C["gmean"]
        elif k == "separate":
            r[k] = mr.separate_error(got[k][0], ref[k][0], st[0], ref[k][1]) / gr.C["separate"]
        else:
            r[k] = _inside(got[k][0], ref[k][0], ref[k][1])
    return r


@pytest.fixture(scope="module")
def clean():
    return {fam: _ratios(*_state(fam)) for fam in FAMILIES}


def test_float64_restatement_meets_every_bar(clean):
    for fam, r in clean.items():
        for k, v in r.items():
            print(fam, k, round(v, 4))
            assert v <= 1.0, (fam, k, v)


def test_constants_are_eight_times_the_yardsticks():
    """MEASURED holds the largest kappa-normalised float64 error over the families, rounded up to two
    digits (so C = 8 x MEASURED); a drift of the restatement or of the families shows here."""
    worst = {k: 0.0 for k in gr.C}
    for fam in FAMILIES:
        (X, basis, act, H, z), flooring = _state(fam)
        for k, v in gr.yardsticks(X, basis, act, H, flooring, z).items():
            worst[k] = max(worst[k], v)
    for k, v in worst.items():
        print("yardstick", k, round(v, 4), "MEASURED", gr.MEASURED[k])
        assert v <= gr.MEASURED[k] <= 1.06 * v + 0.01, (k, v, gr.MEASURED[k])
        assert gr.C[k] == 8.0 * gr.MEASURED[k]


def test_normalize_float64_inside_bars():
    (X, basis, act, H, z), _ = _state(FAMILIES[2])
    Hn, barH, Tn, barT = gr.normalize(basis, H)
    Hf, _, Tf, _ = gr.normalize(basis, H, dtype=np.float64)
    assert _inside(Hf, Hn, barH) <= 1.0 and _inside(Tf, Tn, barT) <= 1.0


# mutant -> the families it is tried on (any broken bar of any of them kills it)
MUTANTS = {
    "frame": [0, 3],        # last frame dropped from a frame sum
    "bin": [0, 3],          # last bin dropped from a bin sum
    "basis": [0, 7],        # last basis index dropped
    "source": [1, 3],       # last source dropped from R
    "c0": [10],             # the c0 tr(R^-1 H R^-1) term dropped (floor family with a visible c0)
    "hermitize": [0, 3],    # H not Hermitised before use
    "floor_first": [10],    # floor applied before instead of after the square root
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_breaks_a_bar(mutant):
    for idx in MUTANTS[mutant]:
        st, flooring = _state(FAMILIES[idx])
        r = _ratios(st, flooring, mutant)
        broken = {k: v for k, v in r.items() if not v <= 1.0}
        print(mutant, FAMILIES[idx], {k: float("%.3g" % v) for k, v in r.items()})
        assert broken, "mutant {} survives at {}: {}".format(mutant, FAMILIES[idx], r)
