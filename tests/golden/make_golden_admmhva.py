#!/usr/bin/env python3
"""Golden vectors of MaskingADMMHVA.

Runs ONLY where the reference checkout is available, as make_golden.py does (whose ``save`` and
``meta`` it reuses unchanged):

    python tests/golden/make_golden_admmhva.py            # write the fixtures
    python tests/golden/make_golden_admmhva.py --seeds    # the gate values of seeds 1..10, no files

Writes the ``tests/golden/admmhva_*.npz`` fixtures (the cases of tests/admmhva_cases.py) and
``admmhva_repr.npz``, the ``repr`` strings of the reference's class; re-running it reproduces them
byte for byte.  Each fixture holds the mixture (scaled to RMS 0.1, as for ADMMBSS), the injected
states where there are any, ``demix_filter`` and the four states after iterations 1, 2 and the last,
an empty loss list (the masking classes of the reference record none), the final filters and the
final output.  The batched fixture holds the runs of the reference on each mixture, stacked.

Every fixture passes the two gates of make_golden_admmbss.py, unchanged (``STABILITY``,
``MIN_SV_RATIO``, ``WatchNegLogdet`` are imported from there): the reference, run again three times on
the input perturbed by 1e-15 relative, stays within 1e-10 of itself in filters, every state and the
output, and every argument handed to ``prox.neg_logdet`` (the first one from the zero state aside: it
is the zero matrix) has a smallest-to-largest singular-value ratio of at least 1e-6.  The measured
values are printed.  A case that fails takes the next seed of 1..10 (``--seeds`` shows them all).
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import admmbss_cases as ac  # noqa: E402
import admmhva_cases as hc  # noqa: E402
from make_golden import meta, save, skipped  # noqa: E402
from make_golden_admmbss import (MIN_SV_RATIO, STABILITY, Snapshots,  # noqa: E402
                                 WatchNegLogdet, rel)
from ssspy.bss import hva as ref_hva  # noqa: E402
from ssspy.special import flooring as ref_flooring  # noqa: E402

NAMES = ("demix_filter",) + ac.ADMM_STATES


def gates(spec, X, init):
    """One mixture through the reference: (the arrays of its fixture, how far it moves under the
    perturbations, the smallest singular-value ratio)."""
    n_iter = spec["n_iter"]
    kept = {k: v.copy() for k, v in init.items()}
    snap = Snapshots("MaskingADMMBSS", n_iter)
    m = hc.construct(ref_hva, ref_flooring, spec, callbacks=snap)
    with WatchNegLogdet(skip=0 if init else 1) as watch:
        Y = m(X, n_iter=n_iter, **init)
    assert all(np.array_equal(init[k], kept[k]) for k in init)
    assert m.loss is None
    rng = np.random.default_rng(spec["seed"] + 11)
    worst = 0.0
    for _ in range(3):
        Xp = X * (1 + 1e-15 * rng.standard_normal(X.shape))
        mp = hc.construct(ref_hva, ref_flooring, spec)
        Yp = mp(Xp, n_iter=n_iter, **init)
        worst = max([worst, rel(Yp, Y)] + [rel(getattr(mp, k), getattr(m, k)) for k in NAMES])
    out = dict(X=X, loss=np.array([], dtype=np.float64), final_output=Y,
               final_demix_filter=m.demix_filter)
    out.update(snap.store)
    return out, worst, watch.worst


def run_one(name, spec, X, init):
    out, worst, ratio = gates(spec, X, init)
    print("{}: stable to {:.1e}, singular-value ratio >= {:.1e}".format(name, worst, ratio))
    assert ratio >= MIN_SV_RATIO, "{}: a neg_logdet argument has singular-value ratio {:.1e}" \
        .format(name, ratio)
    assert worst < STABILITY, "{}: the reference moves by {:.1e} under a 1e-15 perturbation".format(
        name, worst)
    return out


def run(name):
    if skipped(name):
        return
    spec = hc.spec_of(name)
    N, F, T, B = spec["N"], spec["F"], spec["T"], spec["B"]
    X = hc.mixtures(spec)
    init = hc.injected(spec)
    if B == 1:
        out = run_one(name, spec, X, init)
    else:
        parts = [run_one("{}[{}]".format(name, b), spec, X[b], init) for b in range(B)]
        out = {k: np.stack([p[k] for p in parts], axis=1 if k == "loss" else 0) for k in parts[0]}
    out.update({k + "0": v.copy() for k, v in init.items()})
    out.update(meta(kind="admmhva", cls=spec["cls"], n_iter=spec["n_iter"], seed=spec["seed"],
                    shape=(N, F, T), B=B, rho=spec["rho"], relaxation=spec["relaxation"],
                    alpha=np.nan if spec["alpha"] is None else spec["alpha"],
                    attenuation=np.nan if spec["attenuation"] is None else spec["attenuation"],
                    mask_iter=spec["mask_iter"], flooring=spec["flooring"],
                    scale_restoration=spec["scale_restoration"], reference_id=spec["reference_id"]))
    save(name, **out)


def seeds():
    """The gate values of every case at every seed of 1..10: how SPECS' seeds were chosen."""
    for name in hc.CASES:
        for seed in hc.SEEDS:
            spec = dict(hc.spec_of(name), seed=seed)
            X = hc.mixtures(spec)
            parts = [X] if spec["B"] == 1 else list(X)
            values = [gates(spec, Xb, hc.injected(spec))[1:] for Xb in parts]
            worst, ratio = max(v[0] for v in values), min(v[1] for v in values)
            print("{:36s} seed {:2d}: stable to {:.1e}, singular-value ratio >= {:.1e}  {}".format(
                name, seed, worst, ratio,
                "pass" if worst < STABILITY and ratio >= MIN_SV_RATIO else "FAIL"), flush=True)


def reprs():
    if skipped("admmhva_repr"):
        return
    save("admmhva_repr", **{k: np.array(repr(v)) for k, v in hc.repr_objects(ref_hva).items()})


def main():
    if "--seeds" in sys.argv:
        return seeds()
    for name in hc.CASES:
        run(name)
    reprs()


if __name__ == "__main__":
    main()
