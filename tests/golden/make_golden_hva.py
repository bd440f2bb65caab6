#!/usr/bin/env python3
"""Golden vectors of MaskingPDSHVA and HVA.

Runs ONLY where the reference checkout is available, as make_golden.py does (whose ``save`` and
``meta`` it reuses unchanged):

    python tests/golden/make_golden_hva.py

Writes the ``tests/golden/hva_*.npz`` fixtures (the cases of tests/hva_cases.py), ``hva_mask.npz``
(the reference's ``mask_fn`` alone: ``Z``, the mask and the intermediate ``varrho``, see ``masks``)
and ``hva_repr.npz``, the ``repr`` strings of the reference's classes before and after the first
evaluation of the mask; re-running it reproduces them byte for byte.  Each class fixture holds the
mixture (already through ``normalize_by_spectral_norm``), the injected ``demix_filter0`` / ``dual0``
where there are any,
``demix_filter`` and ``dual`` after iterations 1, 2 and the last, an empty loss list (the masking
classes of the reference record none), the final filters and the final output.

Every fixture is checked for conditioning as in make_golden_pdsbss.py: the reference is run again,
three times, on the input perturbed by 1e-15 relative and must stay within 1e-10 of itself in
filters, dual and output.  A case that fails is replaced by another seed or shape.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import hva_cases as hc  # noqa: E402
import pdsbss_cases as pc  # noqa: E402
from make_golden import meta, save, skipped  # noqa: E402
from make_golden_pdsbss import STABILITY, Snapshots, rel  # noqa: E402
from ssspy.bss import hva as ref_hva  # noqa: E402
from ssspy.special import flooring as ref_flooring  # noqa: E402


def run(name):
    if skipped(name):
        return
    spec = hc.spec_of(name)
    N, F, T, n_iter = spec["N"], spec["F"], spec["T"], spec["n_iter"]
    X = pc.laplace_mixture(spec["seed"], N, F, T)
    X = hc.construct(ref_hva, ref_flooring, spec).normalize_by_spectral_norm(X)
    init, out = {}, {}
    if spec["inject"]:
        W0, dual0 = pc.injected_state(spec["seed"], 1, N, F, T)
        dual0 = dual0[0]
        init = {"demix_filter": W0, "dual": dual0}
        out.update(demix_filter0=W0.copy(), dual0=dual0.copy())
    snap = Snapshots(n_iter)
    m = hc.construct(ref_hva, ref_flooring, spec, callbacks=snap)
    Y = m(X, n_iter=n_iter, **init)
    rng = np.random.default_rng(spec["seed"] + 11)
    worst = 0.0
    for _ in range(3):
        Xp = X * (1 + 1e-15 * rng.standard_normal(X.shape))
        mp = hc.construct(ref_hva, ref_flooring, spec)
        Yp = mp(Xp, n_iter=n_iter, **init)
        worst = max(worst, rel(Yp, Y), rel(mp.demix_filter, m.demix_filter), rel(mp.dual, m.dual))
    assert worst < STABILITY, "{}: the reference moves by {:.1e} under a 1e-15 perturbation".format(
        name, worst)
    assert m.loss is None
    out.update(X=X, loss=np.array([], dtype=np.float64), final_output=Y,
               final_demix_filter=m.demix_filter)
    out.update(snap.store)
    out.update(meta(kind="hva", cls=spec["cls"], n_iter=n_iter, seed=spec["seed"], shape=(N, F, T),
                    mu1=spec["mu1"], mu2=spec["mu2"], relaxation=spec["relaxation"],
                    alpha=np.nan if spec["alpha"] is None else spec["alpha"],
                    attenuation=np.nan if spec["attenuation"] is None else spec["attenuation"],
                    mask_iter=spec["mask_iter"], flooring=spec["flooring"],
                    scale_restoration=spec["scale_restoration"], reference_id=spec["reference_id"]))
    save(name, **out)
    print("{}: stable to {:.1e}".format(name, worst))


class NumpyTap:
    """numpy, except that ``exp`` keeps its argument: the reference's mask_fn calls it once, on
    ``2 * varrho``."""

    def __init__(self):
        self.exp_arg = None

    def __getattr__(self, name):
        return getattr(np, name)

    def exp(self, x):
        self.exp_arg = np.array(x, copy=True)
        return np.exp(x)


def masks():
    """The reference's mask_fn on its own, with the intermediate varrho read out of that very call
    (half the argument of its one ``exp``)."""
    if skipped("hva_mask"):
        return
    out = {}
    for F in hc.MASK_BINS:
        Z = hc.mask_input(F)
        m = ref_hva.MaskingPDSHVA(attenuation=hc.MASK_ATTENUATION, mask_iter=hc.MASK_ITER)
        tap = NumpyTap()
        ref_hva.np = tap
        try:
            mask = m.mask_fn(Z)
        finally:
            ref_hva.np = np
        varrho = tap.exp_arg / 2
        assert varrho.shape == Z.shape and np.array_equal(mask, m.mask_fn(Z))
        out.update({"Z_f{}".format(F): Z, "mask_f{}".format(F): mask, "varrho_f{}".format(F): varrho})
    save("hva_mask", **out, **meta(kind="hva_mask", attenuation=hc.MASK_ATTENUATION,
                                   mask_iter=hc.MASK_ITER))


def reprs():
    if skipped("hva_repr"):
        return
    out = {}
    for key, obj in hc.repr_objects(ref_hva).items():
        out[key] = np.array(repr(obj))
        obj.mask_fn(hc.repr_probe())
        out[key + "_after"] = np.array(repr(obj))
    save("hva_repr", **out)


def main():
    for name in hc.CASES:
        run(name)
    masks()
    reprs()


if __name__ == "__main__":
    main()
