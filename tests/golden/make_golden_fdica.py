#!/usr/bin/env python3
"""Golden vectors of the FDICA classes.

Runs ONLY where the reference checkout is available, as make_golden.py does (whose helpers it reuses
unchanged):

    python tests/golden/make_golden_fdica.py

Writes the ``tests/golden/fdica_*.npz`` fixtures; re-running it reproduces them byte for byte.
Each holds the input, the initial filter where one is injected, the filters after iterations
1 / 2 / last (the reference's callback hook), the loss list, the final filters and the final output.

Per-bin Laplace IP overfits short bins and 1 / |y| amplifies rounding, so the runs are short (10
iterations, 5 for IP2) and every fixture is checked for conditioning: the reference is run again on
the input perturbed by 1e-15 relative and must stay within 1e-10 of itself in filters and output
(which also means the same permutation: another one moves whole rows).  A case that fails is
replaced by another seed or shape.
"""

import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import (  # noqa: E402
    custom_floor, flooring_of, gen_iid, gen_mixture, meta, save, skipped,
)
from ssspy.bss.fdica import (  # noqa: E402
    AuxFDICA, AuxLaplaceFDICA, GradFDICA, GradLaplaceFDICA, NaturalGradLaplaceFDICA,
)

CLASSES = {cls.__name__: cls for cls in (GradFDICA, AuxFDICA, GradLaplaceFDICA,
                                         NaturalGradLaplaceFDICA, AuxLaplaceFDICA)}
GENERIC_FLOOR = 1e-10
STABILITY = 1e-10


def generic_contrast_fn(y):
    return 2 * np.abs(y)


def generic_score_fn(y):
    return y / np.maximum(np.abs(y), GENERIC_FLOOR)


def generic_d_contrast_fn(y):
    return 2 * np.ones_like(y)


def combination_pairs(n_sources):
    return itertools.combinations(range(n_sources), 2)


class Snapshots:
    """The filters after iterations 1, 2 and the last."""

    def __init__(self, n_iter):
        self.iters, self.count, self.store = (1, 2, n_iter), -1, {}

    def __call__(self, method):
        self.count += 1
        if self.count in self.iters:
            self.store["it{}_demix_filter".format(self.count)] = np.array(method.demix_filter,
                                                                          copy=True)


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def run_fdica(name, *, cls, N, F, T, seed, gen=gen_mixture, flooring=("max", 1e-10),
              is_holonomic=False, step_size=0.1, spatial_algorithm="IP", pair_selector="sequential",
              permutation_alignment=True, scale_restoration=True, reference_id=0, n_iter=10,
              init_filter=False):
    if skipped(name):
        return
    X = gen(seed, N, F, T)
    aux = "Aux" in cls
    kwargs = dict(permutation_alignment=permutation_alignment, scale_restoration=scale_restoration,
                  reference_id=reference_id)
    kwargs["flooring_fn"] = custom_floor if flooring[0] == "custom" else flooring_of(flooring)
    if aux:
        kwargs["spatial_algorithm"] = spatial_algorithm
        if pair_selector == "combination":
            kwargs["pair_selector"] = combination_pairs
        if cls == "AuxFDICA":
            kwargs.update(contrast_fn=generic_contrast_fn, d_contrast_fn=generic_d_contrast_fn)
    else:
        kwargs.update(step_size=step_size, is_holonomic=is_holonomic)
        if cls == "GradFDICA":
            kwargs.update(contrast_fn=generic_contrast_fn, score_fn=generic_score_fn)
    init, out = {}, {}
    if init_filter:
        rng = np.random.default_rng(seed + 7)
        W0 = np.eye(N) + 0.2 * (rng.standard_normal((F, N, N)) + 1j * rng.standard_normal((F, N, N)))
        init["demix_filter"] = W0
        out["demix_filter0"] = W0.copy()
    snap = Snapshots(n_iter)
    m = CLASSES[cls](callbacks=snap, **kwargs)
    Y = m(X, n_iter=n_iter, **init)
    if init_filter:
        assert np.array_equal(W0, out["demix_filter0"])
    # conditioning: the reference against itself on an input perturbed by 1e-15 relative
    rng = np.random.default_rng(seed + 11)
    for _ in range(3):
        Xp = X * (1 + 1e-15 * rng.standard_normal(X.shape))
        mp = CLASSES[cls](**kwargs)
        Yp = mp(Xp, n_iter=n_iter, **init)
        d = max(rel(Yp, Y), rel(mp.demix_filter, m.demix_filter))
        assert d < STABILITY, "{}: the reference moves by {:.1e} under a 1e-15 perturbation".format(
            name, d)
    out.update(X=X, loss=np.array(m.loss), final_output=Y, final_demix_filter=m.demix_filter)
    out.update(snap.store)
    out.update(meta(kind="fdica", cls=cls, n_iter=n_iter, seed=seed, shape=(N, F, T),
                    floor_kind=flooring[0], floor_eps=flooring[1], is_holonomic=is_holonomic,
                    step_size=step_size, spatial_algorithm=spatial_algorithm,
                    pair_selector=pair_selector, permutation_alignment=permutation_alignment,
                    scale_restoration=scale_restoration, reference_id=reference_id))
    save(name, **out)
    print("{}: stable to {:.1e}".format(name, d))


def main():
    run_fdica("fdica_glap_n2", cls="GradLaplaceFDICA", N=2, F=12, T=40, seed=500)
    run_fdica("fdica_glap_n3_hol_add", cls="GradLaplaceFDICA", N=3, F=10, T=45, seed=501,
              is_holonomic=True, flooring=("add", 1e-3), scale_restoration=False)
    run_fdica("fdica_nglap_n4_init", cls="NaturalGradLaplaceFDICA", N=4, F=9, T=60, seed=502,
              init_filter=True, scale_restoration="projection_back", reference_id=1)
    # (a floor large enough to act: the magnitudes of this mixture lie on both sides of it)
    run_fdica("fdica_nglap_n3_hol_maxfloor", cls="NaturalGradLaplaceFDICA", N=3, F=8, T=50, seed=503,
              is_holonomic=True, flooring=("max", 0.3), step_size=0.05)
    run_fdica("fdica_nglap_n8_mdp", cls="NaturalGradLaplaceFDICA", N=8, F=5, T=100, seed=504,
              scale_restoration="minimal_distortion_principle", reference_id=2)
    run_fdica("fdica_glap_n8_hol_noperm", cls="GradLaplaceFDICA", N=8, F=4, T=90, seed=505,
              gen=gen_iid, is_holonomic=True, permutation_alignment=False, reference_id=5)
    run_fdica("fdica_aux_ip1_n2", cls="AuxLaplaceFDICA", N=2, F=12, T=40, seed=506)
    run_fdica("fdica_aux_ip1_n4_init_none", cls="AuxLaplaceFDICA", N=4, F=9, T=70, seed=507,
              spatial_algorithm="IP1", flooring=("none", 0.0), init_filter=True, reference_id=3)
    run_fdica("fdica_aux_ip1_n8_mdp", cls="AuxLaplaceFDICA", N=8, F=5, T=300, seed=508,
              scale_restoration="minimal_distortion_principle", reference_id=4)
    run_fdica("fdica_aux_ip2_n3", cls="AuxLaplaceFDICA", N=3, F=10, T=120, seed=509,
              spatial_algorithm="IP2", n_iter=5)
    run_fdica("fdica_aux_ip2_n4_comb", cls="AuxLaplaceFDICA", N=4, F=8, T=150, seed=510,
              spatial_algorithm="IP2", pair_selector="combination", n_iter=5,
              scale_restoration=False)
    run_fdica("fdica_aux_ip1_n3_customfloor", cls="AuxLaplaceFDICA", N=3, F=8, T=100, seed=511,
              flooring=("custom", 0.0))
    run_fdica("fdica_aux_ip1_n10_noperm", cls="AuxLaplaceFDICA", N=10, F=3, T=300, seed=512,
              gen=gen_iid, permutation_alignment=False)
    run_fdica("fdica_generic_grad_n3", cls="GradFDICA", N=3, F=8, T=48, seed=513, init_filter=True,
              is_holonomic=True)
    run_fdica("fdica_generic_aux_ip2_n3", cls="AuxFDICA", N=3, F=8, T=120, seed=514,
              spatial_algorithm="IP2", n_iter=5)


if __name__ == "__main__":
    main()
