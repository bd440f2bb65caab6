#!/usr/bin/env python3
"""Golden vectors of the time-domain ICA classes.

Runs ONLY where the reference checkout is available, as make_golden.py does (whose helpers it reuses
unchanged):

    python tests/golden/make_golden_ica.py

Writes the ``tests/golden/ica_*.npz`` fixtures; re-running it reproduces them byte for byte.  Each
holds the input, the initial filter where one is injected, the filters after iterations 1 / 2 / last
(the reference's callback hook), the loss list, the final filter and the final output.

Every fixture is checked for conditioning: the reference is run again on the input perturbed by
1e-15 relative and must stay within 1e-10 of itself in filter and output.  A case that fails is
replaced by another seed or shape (FastICA with the logistic triple at 16 sources moves by 2e-10:
the 16-source FastICA fixture takes log-cosh).
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import meta, save, skipped  # noqa: E402
from ssspy.bss.ica import (  # noqa: E402
    FastICA, GradICA, GradLaplaceICA, NaturalGradICA, NaturalGradLaplaceICA,
)

from ica_cases import CASES, Snapshots, gen_sources, nonlinearity  # noqa: E402

CLASSES = {cls.__name__: cls for cls in (GradICA, NaturalGradICA, FastICA, GradLaplaceICA,
                                         NaturalGradLaplaceICA)}
STABILITY = 1e-10
N_ITER = 10
made = []


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def run_ica(name, *, cls, N, T, seed, nonlin="laplace", is_holonomic=False, step_size=0.1,
            init_filter=False, zero_run=None):
    made.append(name)
    if skipped(name):
        return
    X = gen_sources(seed, N, T, zero_run)
    kwargs = nonlinearity(nonlin, cls)
    if cls != "FastICA":
        kwargs.update(step_size=step_size, is_holonomic=is_holonomic)
    init, out = {}, {}
    if init_filter:
        W0 = np.eye(N) + 0.2 * np.random.default_rng(seed + 7).standard_normal((N, N))
        init["demix_filter"] = W0
        out["demix_filter0"] = W0.copy()
    snap = Snapshots(N_ITER)
    m = CLASSES[cls](callbacks=snap, **kwargs)
    Y = m(X, n_iter=N_ITER, **init)
    if init_filter:
        assert np.array_equal(W0, out["demix_filter0"])
    rng = np.random.default_rng(seed + 11)
    for _ in range(3):
        Xp = X * (1 + 1e-15 * rng.standard_normal(X.shape))
        mp = CLASSES[cls](**kwargs)
        Yp = mp(Xp, n_iter=N_ITER, **init)
        d = max(rel(Yp, Y), rel(mp.demix_filter, m.demix_filter))
        assert d < STABILITY, "{}: the reference moves by {:.1e} under a 1e-15 perturbation".format(
            name, d)
    out.update(X=X, loss=np.array(m.loss), final_output=Y, final_demix_filter=m.demix_filter)
    out.update(snap.store)
    if cls == "FastICA":
        out["whitened_input"] = m.whitened_input
    out.update(meta(kind="ica", cls=cls, n_iter=N_ITER, seed=seed, shape=(N, T), nonlinearity=nonlin,
                    is_holonomic=is_holonomic, step_size=step_size,
                    zero_run=(-1, -1) if zero_run is None else zero_run))
    save(name, **out)
    print("{}: stable to {:.1e}".format(name, d))


def main():
    run_ica("ica_glap_n2", cls="GradLaplaceICA", N=2, T=65, seed=700)
    run_ica("ica_glap_n3_hol", cls="GradLaplaceICA", N=3, T=130, seed=701, is_holonomic=True)
    run_ica("ica_glap_n4_zeros", cls="GradLaplaceICA", N=4, T=200, seed=702, zero_run=(40, 52),
            step_size=0.05)
    run_ica("ica_nglap_n4", cls="NaturalGradLaplaceICA", N=4, T=257, seed=703)
    run_ica("ica_nglap_n3_init", cls="NaturalGradLaplaceICA", N=3, T=150, seed=704,
            init_filter=True)
    run_ica("ica_nglap_n8_hol", cls="NaturalGradLaplaceICA", N=8, T=300, seed=705,
            is_holonomic=True)
    run_ica("ica_nglap_n16", cls="NaturalGradLaplaceICA", N=16, T=400, seed=706)
    run_ica("ica_grad_n3_logistic_hol", cls="GradICA", N=3, T=120, seed=707, nonlin="logistic",
            is_holonomic=True)
    run_ica("ica_ngrad_n4_logcosh", cls="NaturalGradICA", N=4, T=160, seed=708, nonlin="logcosh")
    run_ica("ica_grad_n2_closure", cls="GradICA", N=2, T=100, seed=709, nonlin="closure",
            init_filter=True)
    run_ica("ica_ngrad_n3_closure_hol", cls="NaturalGradICA", N=3, T=140, seed=710,
            nonlin="closure", is_holonomic=True)
    run_ica("ica_fast_n2_logistic", cls="FastICA", N=2, T=65, seed=711, nonlin="logistic")
    run_ica("ica_fast_n4_logcosh", cls="FastICA", N=4, T=300, seed=712, nonlin="logcosh",
            init_filter=True)
    run_ica("ica_fast_n8_logistic", cls="FastICA", N=8, T=1000, seed=713, nonlin="logistic")
    run_ica("ica_fast_n16_logcosh", cls="FastICA", N=16, T=1000, seed=714, nonlin="logcosh")
    run_ica("ica_fast_n3_closure", cls="FastICA", N=3, T=200, seed=715, nonlin="closure")
    assert made == CASES, "tests/ica_cases.py lists other fixtures"


if __name__ == "__main__":
    main()
