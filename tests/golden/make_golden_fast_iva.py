#!/usr/bin/env python3
"""Golden vectors of FastIVA / FasterIVA and of ``whiten`` / ``pca``.

Runs ONLY where the reference checkout is available, as make_golden.py does (whose ``save`` and
``meta`` it reuses unchanged):

    python tests/golden/make_golden_fast_iva.py

Writes the ``tests/golden/fastiva_*.npz`` / ``fasteriva_*.npz`` fixtures (tests/fast_iva_cases.py
lists them); re-running it reproduces them byte for byte.  Each holds the input, the reference's
whitened input (its phase gauge), the injected filter where there is one, the loss list, W P after
iterations 1 and 2 and at the end, the final output and the meta fields.

FasterIVA amplifies rounding, more so with the source count.  So for every fixture the reference is
run a second time on the input perturbed by 2^-50 relative, and the iteration count is lowered from
10 until its own output and losses move by at most 5e-12 -- half of the 1e-11 bar the NumPy restatement
is held to, and well inside the 1e-10 (1/100 of the device's 1e-8 bar) every fixture has to meet; 2e-11
at 16 channels, where the whitening alone moves the mixture by cond * 2^-50 ~ 7e-12 and no
iteration count gets below that; the measured movement is stored as ``meta_ref_movement``.  Also asserted: the relative
gap (lam_max - lam_2) / lam_max of every U_in at every recorded state is at least 1e-3, and
cond(mean x x^H) <= 1e6 in every bin.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import meta, save, skipped  # noqa: E402
import fast_iva_cases as fc  # noqa: E402
from ssspy.bss.iva import FasterIVA, FastIVA  # noqa: E402
from ssspy.special import flooring as ref_flooring  # noqa: E402
from ssspy.transform import pca, whiten  # noqa: E402

CLASSES = {"FastIVA": FastIVA, "FasterIVA": FasterIVA}
MAX_ITER = 10
MOVEMENT_BOUND = 5e-12
MOVEMENT_BOUND_16 = 2e-11
GAP_BOUND = 1e-3
COND_BOUND = 1e6


class Recorder(fc.ActionSnapshots):
    """W P after iterations 1 and 2, and the eigenvalue gaps of U_in of every state."""

    def __init__(self, faster):
        super().__init__()
        self.faster = faster
        self.min_gap = np.inf

    def __call__(self, method):
        super().__call__(method)
        if self.faster:
            Z = method.whitened_input
            Y = method.separate(Z, demix_filter=method.demix_filter, use_whitening=False)
            r = np.linalg.norm(Y, axis=1)
            phi = method.d_contrast_fn(r) / method.flooring_fn(2 * r)
            U = np.einsum("nt,aft,bft->fnab", phi, Z, Z.conj()) / Z.shape[-1]
            lam = np.linalg.eigvalsh(U)
            self.min_gap = min(self.min_gap, np.min((lam[..., -1] - lam[..., -2]) / lam[..., -1]))


def run_reference(cfg, X, n_iter, W0):
    rec = Recorder(cfg["cls"] == "FasterIVA")
    m = CLASSES[cfg["cls"]](flooring_fn=fc.flooring_for(cfg["flooring"], ref_flooring),
                            callbacks=rec, scale_restoration=cfg["scale_restoration"],
                            reference_id=cfg["reference_id"],
                            **fc.closures_for(cfg["cls"], cfg["contrast"]))
    init = {} if W0 is None else {"demix_filter": W0.copy()}
    Y = m(X, n_iter=n_iter, **init)
    return m, rec, Y


def run_case(name):
    if skipped(name):
        return
    cfg = fc.settings(name)
    N, F, T = cfg["shape"]
    X = fc.gen_mixture(cfg["seed"], N, F, T)
    C = np.einsum("mft,nft->fmn", X, X.conj()) / T
    cond = float(np.max(np.linalg.cond(C)))
    assert cond <= COND_BOUND, (name, cond)
    W0 = fc.initial_filter(cfg["seed"], N, F) if cfg["init_filter"] else None
    rng = np.random.default_rng(cfg["seed"] + 99)
    X2 = X * (1 + 2.0 ** -50 * rng.uniform(-1, 1, X.shape))
    bound = MOVEMENT_BOUND_16 if N == 16 else MOVEMENT_BOUND
    for n_iter in range(MAX_ITER, 0, -1):
        m, rec, Y = run_reference(cfg, X, n_iter, W0)
        m2, _, Y2 = run_reference(cfg, X2, n_iter, W0)
        loss, loss2 = np.array(m.loss), np.array(m2.loss)
        movement = max(fc.err(Y2, Y), float(np.max(np.abs(loss2 - loss) / np.abs(loss))))
        if movement <= bound:
            break
    assert movement <= bound, (name, movement)
    assert n_iter >= 2, (name, n_iter)
    if cfg["cls"] == "FasterIVA":
        assert rec.min_gap >= GAP_BOUND, (name, rec.min_gap)
    if cfg["flooring"][0] == "max" and cfg["flooring"][1] > 1e-6:
        # the floor acts on some frame norms and not on others
        r2 = 2 * np.linalg.norm(m.whitened_input, axis=1)
        assert 0 < np.sum(r2 < cfg["flooring"][1]) < r2.size, name
    out = dict(X=X, whitened_input=m.whitened_input, loss=loss, final_output=Y,
               final_action=fc.filter_action(m))
    out.update(rec.store)
    if W0 is not None:
        out["demix_filter0"] = W0
    out.update(meta(kind="fast_iva", cls=cfg["cls"], n_iter=n_iter, seed=cfg["seed"],
                    shape=(N, F, T), contrast=cfg["contrast"], floor_kind=cfg["flooring"][0],
                    floor_eps=cfg["flooring"][1], scale_restoration=cfg["scale_restoration"],
                    reference_id=cfg["reference_id"], ref_movement=movement,
                    min_gap=(rec.min_gap if cfg["cls"] == "FasterIVA" else 1.0), max_cond=cond))
    save(name, **out)


def run_transforms():
    if skipped(fc.TRANSFORM_FIXTURE):
        return
    rng = np.random.default_rng(520)

    def cplx(*shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)

    inputs = {"c3": fc.gen_mixture(521, 3, 6, 20),
              "c4": np.stack([fc.gen_mixture(522 + b, 5, 3, 18) for b in range(2)]),
              "r2": rng.standard_normal((3, 3)) @ rng.standard_normal((3, 50)),
              "r3": rng.standard_normal((2, 4, 4)) @ rng.standard_normal((2, 4, 40))}
    out = {}
    for key, x in inputs.items():
        out["x_" + key] = x
        out["whiten_" + key] = whiten(x)
        out["pca_ascend_" + key] = pca(x, ascend=True)
        out["pca_descend_" + key] = pca(x, ascend=False)
    out.update(meta(kind="fast_iva_transforms"))
    save(fc.TRANSFORM_FIXTURE, **out)


def main():
    for name in fc.CASES:
        run_case(name)
    run_transforms()


if __name__ == "__main__":
    main()
