#!/usr/bin/env python3
"""Golden vectors of the gradient / natural-gradient IVA classes.

Runs ONLY where the reference checkout is available, as make_golden.py does (whose helpers it reuses
unchanged):

    python tests/golden/make_golden_grad_iva.py

Writes the ``tests/golden/gradiva_*.npz`` fixtures; re-running it reproduces them byte for byte.
Each holds the input, the initial filter where one is injected, the filters after iterations
1 / 2 / 10 (the reference's callback hook), the loss list, the final filters and the final output.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import (  # noqa: E402
    Snapshots, custom_floor, flooring_of, gen_iid, gen_mixture, meta, save, skipped,
)
from ssspy.bss.iva import (  # noqa: E402
    GradGaussIVA, GradLaplaceIVA, NaturalGradGaussIVA, NaturalGradIVA, NaturalGradLaplaceIVA,
)

CLASSES = {cls.__name__: cls for cls in (GradLaplaceIVA, GradGaussIVA, NaturalGradLaplaceIVA,
                                         NaturalGradGaussIVA, NaturalGradIVA)}

GENERIC_FLOOR = 1e-10


def generic_contrast_fn(y):
    return 2 * np.linalg.norm(y, axis=1)


def generic_score_fn(y):
    norm = np.linalg.norm(y, axis=1, keepdims=True)
    return y / np.maximum(norm, GENERIC_FLOOR)


def run_grad_iva(name, *, cls, N, F, T, seed, gen=gen_mixture, flooring=("max", 1e-10),
                 is_holonomic=True, step_size=0.1, scale_restoration=True, reference_id=0,
                 n_iter=10, init_filter=False):
    if skipped(name):
        return
    X = gen(seed, N, F, T)
    names = ["demix_filter"] + (["variance"] if "Gauss" in cls else [])
    snap = Snapshots(names)
    kwargs = dict(step_size=step_size, callbacks=snap, is_holonomic=is_holonomic,
                  scale_restoration=scale_restoration, reference_id=reference_id)
    if flooring[0] == "custom":
        kwargs["flooring_fn"] = custom_floor
    else:
        kwargs["flooring_fn"] = flooring_of(flooring)
    if cls == "NaturalGradIVA":
        kwargs.update(contrast_fn=generic_contrast_fn, score_fn=generic_score_fn)
    m = CLASSES[cls](**kwargs)
    init = {}
    out = {}
    if init_filter:
        rng = np.random.default_rng(seed + 7)
        W0 = np.eye(N) + 0.2 * (rng.standard_normal((F, N, N)) + 1j * rng.standard_normal((F, N, N)))
        init["demix_filter"] = W0
        out["demix_filter0"] = W0.copy()
    Y = m(X, n_iter=n_iter, **init)
    if init_filter:
        assert np.array_equal(W0, out["demix_filter0"])
    out.update(X=X, loss=np.array(m.loss), final_output=Y, final_demix_filter=m.demix_filter)
    out.update(snap.store)
    out.update(meta(kind="grad_iva", cls=cls, n_iter=n_iter, seed=seed, shape=(N, F, T),
                    floor_kind=flooring[0], floor_eps=flooring[1], is_holonomic=is_holonomic,
                    step_size=step_size, scale_restoration=scale_restoration,
                    reference_id=reference_id))
    save(name, **out)


def main():
    run_grad_iva("gradiva_nglap_n2", cls="NaturalGradLaplaceIVA", N=2, F=12, T=40, seed=400)
    run_grad_iva("gradiva_nglap_n3_nonhol_add", cls="NaturalGradLaplaceIVA", N=3, F=10, T=45,
                 seed=401, is_holonomic=False, flooring=("add", 1e-3), scale_restoration=False)
    run_grad_iva("gradiva_glap_n4_init", cls="GradLaplaceIVA", N=4, F=9, T=60, seed=402,
                 init_filter=True, scale_restoration="projection_back", reference_id=1)
    # (a floor large enough to act: the frame norms of this mixture lie on both sides of it)
    run_grad_iva("gradiva_glap_n3_nonhol_maxfloor", cls="GradLaplaceIVA", N=3, F=8, T=50, seed=403,
                 is_holonomic=False, flooring=("max", 2.0), step_size=0.05)
    run_grad_iva("gradiva_ngauss_n6", cls="NaturalGradGaussIVA", N=6, F=6, T=70, seed=404,
                 scale_restoration="minimal_distortion_principle", reference_id=2)
    run_grad_iva("gradiva_ggauss_n2_nonhol", cls="GradGaussIVA", N=2, F=12, T=40, seed=405,
                 is_holonomic=False, step_size=0.2)
    run_grad_iva("gradiva_ggauss_n8", cls="GradGaussIVA", N=8, F=4, T=90, seed=406, gen=gen_iid)
    run_grad_iva("gradiva_nglap_n8_nonhol", cls="NaturalGradLaplaceIVA", N=8, F=4, T=90, seed=407,
                 is_holonomic=False, reference_id=5)
    run_grad_iva("gradiva_glap_n10", cls="GradLaplaceIVA", N=10, F=3, T=110, seed=408, gen=gen_iid,
                 n_iter=6, flooring=("none", 0.0))
    run_grad_iva("gradiva_ngauss_n12_nonhol", cls="NaturalGradGaussIVA", N=12, F=3, T=120,
                 seed=409, gen=gen_iid, n_iter=6, is_holonomic=False)
    run_grad_iva("gradiva_nglap_n4_customfloor", cls="NaturalGradLaplaceIVA", N=4, F=8, T=48,
                 seed=410, flooring=("custom", 0.0))
    run_grad_iva("gradiva_generic_ng_n3", cls="NaturalGradIVA", N=3, F=8, T=48, seed=411,
                 init_filter=True)


if __name__ == "__main__":
    main()
