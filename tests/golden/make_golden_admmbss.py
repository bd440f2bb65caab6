#!/usr/bin/env python3
"""Golden vectors of ADMMBSS, MaskingADMMBSS, ADMMIVA and PDSIVA.

Runs ONLY where the reference checkout is available, as make_golden.py does (whose ``save`` and
``meta`` it reuses unchanged):

    python tests/golden/make_golden_admmbss.py

Writes the ``tests/golden/admm*.npz`` / ``pdsiva*.npz`` fixtures (the cases of tests/admmbss_cases.py)
and ``admmbss_repr.npz``, the ``repr`` strings of the reference's classes; re-running it reproduces
them byte for byte.  Each fixture holds the mixture (scaled to RMS 0.1: at RMS 1 the reference's ADMM
iteration diverges), the injected states where there are any, ``demix_filter`` and every state
after iterations 1, 2 and the last, the loss list (empty when none is recorded), the final filters and
the final output.  A batched fixture holds the runs of the reference on each mixture, stacked.

Every fixture is checked for conditioning: the reference is run again, three times, on the input
perturbed by 1e-15 relative and must stay within 1e-10 of itself in filters, every state and the
output -- 100 times under the parity bar of the tests -- and every argument handed to
``prox.neg_logdet`` after the first iteration (whose argument is the zero matrix from the default
state) must have a smallest-to-largest singular-value ratio of at least 1e-6.  A case that fails is
replaced by another seed.
"""

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import admmbss_cases as ac  # noqa: E402
from make_golden import meta, save, skipped  # noqa: E402
from ssspy.bss.admmbss import ADMMBSS, ADMMBSSBase, MaskingADMMBSS  # noqa: E402
from ssspy.bss.iva import ADMMIVA, PDSIVA  # noqa: E402
from ssspy.linalg import prox  # noqa: E402

CLASSES = {"ADMMBSS": ADMMBSS, "MaskingADMMBSS": MaskingADMMBSS, "ADMMIVA": ADMMIVA,
           "PDSIVA": PDSIVA}
STABILITY = 1e-10
MIN_SV_RATIO = 1e-6


class Snapshots:
    """demix_filter and the states after iterations 1, 2 and the last."""

    def __init__(self, cls, n_iter):
        self.names = ("demix_filter",) + ac.state_names(cls)
        self.iters, self.count, self.store = (1, 2, n_iter), -1, {}

    def __call__(self, method):
        self.count += 1
        if self.count in self.iters:
            for name in self.names:
                self.store["it{}_{}".format(self.count, name)] = np.array(getattr(method, name),
                                                                          copy=True)


class WatchNegLogdet:
    """Wraps the reference's ``prox.neg_logdet`` and keeps the smallest singular-value ratio of its
    arguments, the first ``skip`` calls aside."""

    def __init__(self, skip):
        self.skip, self.calls, self.worst = skip, 0, np.inf
        self.inner = prox.neg_logdet

    def __call__(self, X, step_size=1):
        self.calls += 1
        if self.calls > self.skip:
            s = np.linalg.svd(X, compute_uv=False)
            self.worst = min(self.worst, float(np.min(s[..., -1] / s[..., 0])))
        return self.inner(X, step_size=step_size)

    def __enter__(self):
        prox.neg_logdet = self
        return self

    def __exit__(self, *exc):
        prox.neg_logdet = self.inner


def rel(a, b):
    denom = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (denom if denom > 0 else 1.0)


def construct(spec, **extra):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return CLASSES[spec["cls"]](**ac.build_kwargs(spec, prox), **extra)


def run_one(name, spec, X, init):
    """One mixture through the reference and the conditioning gate: the arrays of its fixture."""
    n_iter, names = spec["n_iter"], ("demix_filter",) + ac.state_names(spec["cls"])
    kept = {k: v.copy() for k, v in init.items()}
    snap = Snapshots(spec["cls"], n_iter)
    m = construct(spec, callbacks=snap)
    # (from the zero state the first argument of an ADMM class is the zero matrix)
    with WatchNegLogdet(skip=0 if init or spec["cls"] == "PDSIVA" else 1) as watch:
        Y = m(X, n_iter=n_iter, **init)
    assert all(np.array_equal(init[k], kept[k]) for k in init)
    assert watch.worst >= MIN_SV_RATIO, "{}: a neg_logdet argument has singular-value ratio {:.1e}" \
        .format(name, watch.worst)
    rng = np.random.default_rng(spec["seed"] + 11)
    worst = 0.0
    for _ in range(3):
        Xp = X * (1 + 1e-15 * rng.standard_normal(X.shape))
        mp = construct(spec)
        Yp = mp(Xp, n_iter=n_iter, **init)
        worst = max([worst, rel(Yp, Y)] + [rel(getattr(mp, k), getattr(m, k)) for k in names])
    assert worst < STABILITY, "{}: the reference moves by {:.1e} under a 1e-15 perturbation".format(
        name, worst)
    out = dict(X=X, loss=np.array(m.loss if m.loss is not None else [], dtype=np.float64),
               final_output=Y, final_demix_filter=m.demix_filter)
    out.update(snap.store)
    print("{}: stable to {:.1e}, singular-value ratio >= {:.1e}".format(name, worst, watch.worst))
    return out


def run(name):
    if skipped(name):
        return
    spec = ac.spec_of(name)
    N, F, T, B = spec["N"], spec["F"], spec["T"], spec["B"]
    X = ac.mixtures(spec)
    init = {}
    if spec["inject"]:
        init = ac.injected_state(spec["seed"], max(len(spec["penalties"]), 1), N, F, T)
    if B == 1:
        out = run_one(name, spec, X, init)
    else:
        parts = [run_one("{}[{}]".format(name, b), spec, X[b], init) for b in range(B)]
        out = {k: np.stack([p[k] for p in parts], axis=1 if k == "loss" else 0) for k in parts[0]}
    out.update({k + "0": v.copy() for k, v in init.items()})
    record = spec["record_loss"]
    out.update(meta(kind="admmbss", cls=spec["cls"], n_iter=spec["n_iter"], seed=spec["seed"],
                    shape=(N, F, T), B=B, penalties=np.array(spec["penalties"], dtype=str),
                    rho=spec["rho"], relaxation=spec["relaxation"],
                    alpha=np.nan if spec["alpha"] is None else spec["alpha"],
                    record_loss=-1 if record is None else int(record), user=spec["user"],
                    scale_restoration=spec["scale_restoration"], reference_id=spec["reference_id"]))
    save(name, **out)


def reprs():
    """The repr strings of the reference, by a label the tests rebuild the object from."""
    if skipped("admmbss_repr"):
        return

    def fn(y, step_size=1):
        return y

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        objs = {
            "base": ADMMBSSBase(prox_penalty=fn),
            "base_noscale": ADMMBSSBase(prox_penalty=[fn, fn], scale_restoration=False),
            "admm_default": ADMMBSS(penalty_fn=fn, prox_penalty=fn),
            "admm_two": ADMMBSS(rho=0.5, relaxation=1.5, penalty_fn=[fn, fn], prox_penalty=[fn, fn],
                                reference_id=2, scale_restoration="minimal_distortion_principle"),
            "admm_alpha_noscale": ADMMBSS(alpha=1.25, prox_penalty=fn, record_loss=False,
                                          scale_restoration=False),
            "masking_default": MaskingADMMBSS(mask_fn=fn),
            "masking_loss": MaskingADMMBSS(rho=2.0, penalty_fn=fn, mask_fn=fn, record_loss=False,
                                           scale_restoration=False),
            "admmiva_default": ADMMIVA(),
            "pdsiva_default": PDSIVA(),
        }
    save("admmbss_repr", **{k: np.array(repr(v)) for k, v in objs.items()})


def main():
    for name in ac.CASES:
        run(name)
    reprs()


if __name__ == "__main__":
    main()
