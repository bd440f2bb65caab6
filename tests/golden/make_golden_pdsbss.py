#!/usr/bin/env python3
"""Golden vectors of PDSBSS and MaskingPDSBSS.

Runs ONLY where the reference checkout is available, as make_golden.py does (whose ``save`` and
``meta`` it reuses unchanged):

    python tests/golden/make_golden_pdsbss.py

Writes the ``tests/golden/pdsbss_*.npz`` fixtures (the cases of tests/pdsbss_cases.py) and
``pdsbss_repr.npz``, the ``repr`` strings of the reference's classes; re-running it reproduces them
byte for byte.  Each fixture holds the mixture (already through ``normalize_by_spectral_norm``), the
injected ``demix_filter0`` / ``dual0`` where there are any, ``demix_filter`` and ``dual`` after
iterations 1, 2 and the last, the loss list (empty when none is recorded), the final filters and the
final output.

Every fixture is checked for conditioning: the reference is run again, three times, on the input
perturbed by 1e-15 relative and must stay within 1e-10 of itself in filters, dual and output -- 100
times under the parity bar of the tests.  A case that fails is replaced by another seed or shape.
"""

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import pdsbss_cases as pc  # noqa: E402
from make_golden import meta, save, skipped  # noqa: E402
from ssspy.bss.pdsbss import PDSBSS, MaskingPDSBSS  # noqa: E402
from ssspy.bss.proxbss import ProxBSSBase  # noqa: E402
from ssspy.linalg import prox  # noqa: E402

CLASSES = {"PDSBSS": PDSBSS, "MaskingPDSBSS": MaskingPDSBSS}
STABILITY = 1e-10


class Snapshots:
    """demix_filter and dual after iterations 1, 2 and the last."""

    def __init__(self, n_iter):
        self.iters, self.count, self.store = (1, 2, n_iter), -1, {}

    def __call__(self, method):
        self.count += 1
        if self.count in self.iters:
            for name in ("demix_filter", "dual"):
                self.store["it{}_{}".format(self.count, name)] = np.array(getattr(method, name),
                                                                          copy=True)


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def construct(spec, **extra):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return CLASSES[spec["cls"]](**pc.build_kwargs(spec, prox), **extra)


def run(name):
    if skipped(name):
        return
    spec = pc.spec_of(name)
    N, F, T, n_iter = spec["N"], spec["F"], spec["T"], spec["n_iter"]
    Q = len(spec["penalties"])
    X = pc.laplace_mixture(spec["seed"], N, F, T)
    X = construct(spec).normalize_by_spectral_norm(X)
    init, out = {}, {}
    if spec["inject"]:
        W0, dual0 = pc.injected_state(spec["seed"], Q, N, F, T)
        init = {"demix_filter": W0, "dual": dual0}
        out.update(demix_filter0=W0.copy(), dual0=dual0.copy())
    snap = Snapshots(n_iter)
    m = construct(spec, callbacks=snap)
    Y = m(X, n_iter=n_iter, **init)
    if init:
        assert np.array_equal(W0, out["demix_filter0"]) and np.array_equal(dual0, out["dual0"])
    rng = np.random.default_rng(spec["seed"] + 11)
    worst = 0.0
    for _ in range(3):
        Xp = X * (1 + 1e-15 * rng.standard_normal(X.shape))
        mp = construct(spec)
        Yp = mp(Xp, n_iter=n_iter, **init)
        worst = max(worst, rel(Yp, Y), rel(mp.demix_filter, m.demix_filter), rel(mp.dual, m.dual))
    assert worst < STABILITY, "{}: the reference moves by {:.1e} under a 1e-15 perturbation".format(
        name, worst)
    out.update(X=X, loss=np.array(m.loss if m.loss is not None else [], dtype=np.float64),
               final_output=Y, final_demix_filter=m.demix_filter)
    out.update(snap.store)
    record = spec["record_loss"]
    out.update(meta(kind="pdsbss", cls=spec["cls"], n_iter=n_iter, seed=spec["seed"], shape=(N, F, T),
                    penalties=np.array(spec["penalties"]), mu1=spec["mu1"], mu2=spec["mu2"],
                    relaxation=spec["relaxation"],
                    alpha=np.nan if spec["alpha"] is None else spec["alpha"],
                    record_loss=-1 if record is None else int(record),
                    scale_restoration=spec["scale_restoration"], reference_id=spec["reference_id"]))
    save(name, **out)
    print("{}: stable to {:.1e}".format(name, worst))


def reprs():
    """The repr strings of the reference, by a label the tests rebuild the object from."""
    if skipped("pdsbss_repr"):
        return
    def fn(y, step_size=1):
        return y
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        objs = {
            "base": ProxBSSBase(prox_penalty=fn),
            "base_noscale": ProxBSSBase(prox_penalty=[fn, fn], scale_restoration=False),
            "pds_default": PDSBSS(prox_penalty=fn),
            "pds_two_loss": PDSBSS(mu1=0.5, mu2=2, relaxation=1.5, penalty_fn=[fn, fn],
                                   prox_penalty=[fn, fn], record_loss=True, reference_id=2,
                                   scale_restoration="minimal_distortion_principle"),
            "pds_alpha_noscale": PDSBSS(alpha=1.25, prox_penalty=fn, scale_restoration=False),
            "masking_default": MaskingPDSBSS(mask_fn=fn),
            "masking_loss": MaskingPDSBSS(mu1=2.0, penalty_fn=fn, mask_fn=fn, record_loss=False,
                                          scale_restoration=False),
        }
    save("pdsbss_repr", **{k: np.array(repr(v)) for k, v in objs.items()})


def main():
    for name in pc.CASES:
        run(name)
    reprs()


if __name__ == "__main__":
    main()
