#!/usr/bin/env python3
"""Golden vectors of CACGMM.

Runs ONLY where the reference checkout is available, as make_golden.py does (whose ``save`` and
``meta`` it reuses unchanged):

    python tests/golden/make_golden_cacgmm.py

Writes the ``tests/golden/cacgmm_*.npz`` fixtures listed in ``tests/cacgmm_numpy.GOLDEN``;
re-running it reproduces them byte for byte.  Each holds the input, the options, the reference's
``mixing`` / ``covariance`` at the initial call and after every iteration (its callback hook), the
loss list, and the final (aligned) ``mixing`` / ``covariance`` / ``posterior`` / ``output``.
"""

import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import cacgmm_numpy as cn  # noqa: E402
from make_golden import meta, save, skipped  # noqa: E402
from ssspy.bss.cacgmm import CACGMM  # noqa: E402
from ssspy.special.flooring import add_flooring, max_flooring  # noqa: E402


def reference_floor(spec):
    if spec is None:
        return None
    kind, eps = spec
    return functools.partial(max_flooring if kind == "max" else add_flooring, eps=eps)


def run_cacgmm(name, case, options):
    if skipped(name):
        return
    M, N, F, T = case
    X = cn.make_mixture(M, N, F, T)
    options = dict(options)
    flooring = options.pop("flooring", ("max", 1e-10))
    snaps = {"mixing": [], "covariance": []}

    def snapshot(method):
        snaps["mixing"].append(method.mixing.copy())
        snaps["covariance"].append(method.covariance.copy())

    m = CACGMM(n_sources=N, flooring_fn=reference_floor(flooring), callbacks=snapshot,
               rng=np.random.default_rng(0), **options)
    Y = m(X, n_iter=cn.N_ITER)
    save(name, input=X, mixing=np.stack(snaps["mixing"]), covariance=np.stack(snaps["covariance"]),
         loss=np.array(m.loss), final_mixing=m.mixing, final_covariance=m.covariance,
         posterior=m.posterior, output=Y,
         **meta(n_sources=N, floor_kind="none" if flooring is None else flooring[0],
                floor_eps=0.0 if flooring is None else flooring[1],
                normalization=options.get("normalization", True),
                permutation_alignment=str(options.get("permutation_alignment", True)),
                reference_id=options.get("reference_id", 0),
                global_iter=options.get("global_iter", 1),
                local_iter=options.get("local_iter", 1)))


if __name__ == "__main__":
    for name, (case, options) in cn.GOLDEN.items():
        run_cacgmm(name, case, options)
