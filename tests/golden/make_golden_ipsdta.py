#!/usr/bin/env python3
"""Golden vectors of GaussIPSDTA / TIPSDTA and of the VCD operator.

Runs ONLY where the reference checkout is available, as make_golden.py does (whose ``save`` and
``meta`` it reuses unchanged):

    python tests/golden/make_golden_ipsdta.py

Writes the ``tests/golden/ipsdta_*.npz`` fixtures (tests/ipsdta_cases.py lists them); re-running it
reproduces them byte for byte.  Each holds the input, the initial basis, activation and filter
(after the reference's own normalisation at reset they are ``basis0_*`` / ``activation0``; the
seeded draw is reproduced by the classes under test), output and filter after iterations 1 and 2
and at the end, the loss list and the settings.

For every fixture the reference is run a second time on the input perturbed by 2^-50 relative; the
iteration count is lowered from 5 until its own output, filter and losses (relative to the largest
loss of the run: they cross zero) move by at most 1e-10; the movement is stored as
``meta_ref_movement``.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import meta, save, skipped  # noqa: E402
import ipsdta_cases as ic  # noqa: E402
from ssspy.bss._update_spatial_model import update_by_block_decomposition_vcd  # noqa: E402
from ssspy.bss.ipsdta import TIPSDTA, GaussIPSDTA  # noqa: E402
from ssspy.special import flooring as ref_flooring  # noqa: E402

MAX_ITER = 5
MOVEMENT_BOUND = 1e-10


class Recorder(ic.Snapshots):
    """Also the state the reference starts from (after its normalisation at reset)."""

    def __call__(self, method):
        if self.calls == 0:
            basis = method.basis
            low, high = basis if type(basis) is tuple else (basis, None)
            self.store["basis0_low"] = np.array(low)
            if high is not None:
                self.store["basis0_high"] = np.array(high)
            self.store["activation0"] = np.array(method.activation)
            self.store["demix_filter0"] = np.array(method.demix_filter)
        super().__call__(method)


def run_reference(cfg, X, n_iter):
    rec = Recorder()
    kwargs = dict(n_basis=cfg["n_basis"], n_blocks=cfg["n_blocks"],
                  flooring_fn=ic.flooring_for(cfg["flooring"], ref_flooring), callbacks=rec,
                  source_normalization=cfg["source_normalization"],
                  scale_restoration=cfg["scale_restoration"], reference_id=cfg["reference_id"],
                  rng=np.random.default_rng(cfg["seed"] + 1))
    if cfg["cls"] == "TIPSDTA":
        m = TIPSDTA(dof=cfg["dof"], **kwargs)
    else:
        m = GaussIPSDTA(**kwargs)
    init = ic.initial_state(cfg) if cfg["inject"] else {}
    Y = m(X, n_iter=n_iter, **init)
    return m, rec, Y


def run_case(name):
    if skipped(name):
        return
    cfg = ic.CASES[name]
    N, F, T = cfg["shape"]
    X = ic.gen_mixture(cfg["seed"], N, F, T)
    rng = np.random.default_rng(cfg["seed"] + 99)
    X2 = X * (1 + 2.0 ** -50 * rng.uniform(-1, 1, X.shape))
    for n_iter in range(MAX_ITER, 0, -1):
        m, rec, Y = run_reference(cfg, X, n_iter)
        m2, _, Y2 = run_reference(cfg, X2, n_iter)
        loss, loss2 = np.array(m.loss), np.array(m2.loss)
        movement = max(ic.err(Y2, Y), ic.err(m2.demix_filter, m.demix_filter),
                       float(np.max(np.abs(loss2 - loss)) / np.max(np.abs(loss))))
        if movement <= MOVEMENT_BOUND:
            break
    assert movement <= MOVEMENT_BOUND, (name, movement)
    assert n_iter >= 2, (name, n_iter)
    out = dict(X=X, loss=loss, final_output=Y, final_demix_filter=np.array(m.demix_filter))
    out.update(rec.store)
    out.update(meta(kind="ipsdta", cls=cfg["cls"], n_iter=n_iter, seed=cfg["seed"], shape=(N, F, T),
                    n_blocks=cfg["n_blocks"], n_basis=cfg["n_basis"],
                    dof=(-1.0 if cfg["dof"] is None else cfg["dof"]), flooring=cfg["flooring"],
                    source_normalization=cfg["source_normalization"],
                    scale_restoration=str(cfg["scale_restoration"]),
                    reference_id=cfg["reference_id"], inject=cfg["inject"],
                    ref_movement=movement))
    save(name, **out)


def run_vcd_operator():
    if skipped(ic.VCD_FIXTURE):
        return
    rng = np.random.default_rng(640)
    out = {}
    for key, (C, L, N) in {"a": (3, 2, 2), "b": (2, 4, 3), "c": (1, 1, 4), "d": (2, 3, 8)}.items():
        W = np.eye(N) + 0.3 * (rng.standard_normal((C, L, N, N)) + 1j * rng.standard_normal((C, L, N, N)))
        G = rng.standard_normal((C, N, L * N, 2 * L * N)) + 1j * rng.standard_normal((C, N, L * N, 2 * L * N))
        H = (G @ np.conj(np.swapaxes(G, -2, -1)) / (2 * L * N)).reshape(C, N, L, N, L, N)
        RXX = np.ascontiguousarray(H.transpose(0, 2, 4, 1, 3, 5))  # (C, L, L, N, M, M)
        out["W_" + key], out["RXX_" + key] = W, RXX
        out["out_" + key] = update_by_block_decomposition_vcd(W, RXX, overwrite=False)
        out["out_floor_" + key] = update_by_block_decomposition_vcd(
            W, RXX, singular_fn=lambda x: np.abs(x) < 1e-10, overwrite=False)
    out.update(meta(kind="ipsdta_vcd_operator"))
    save(ic.VCD_FIXTURE, **out)


def main():
    for name in ic.CASES:
        run_case(name)
    run_vcd_operator()


if __name__ == "__main__":
    main()
