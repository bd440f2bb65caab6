"""What the fixture generator (tests/golden/make_golden_admmhva.py) and the CPU and GPU tests of
MaskingADMMHVA share: the list of fixtures and how each was made, and the ``repr`` objects.  The
mixtures (RMS 0.1), the injected states, the snapshot callback and the comparison with a fixture are
those of tests/admmbss_cases.py, the flooring functions by name those of tests/hva_cases.py."""

import warnings

import numpy as np

import admmbss_cases as ac
import hva_cases as hc
from conftest import option as _option

# name -> how the fixture is made.  flooring: a key of ``hva_cases.flooring_of``.  The seeds are the
# first of 1..10 that pass the generator's two gates.
SPECS = {
    "admmhva_n2_f9": dict(N=2, F=9, T=40),
    "admmhva_n3_f17_iter3": dict(N=3, F=17, T=50, mask_iter=3, rho=0.5, relaxation=1.5,
                                 reference_id=1),
    "admmhva_n4_f33_iter0_init": dict(N=4, F=33, T=40, mask_iter=0, inject=True),
    "admmhva_n3_f6_add_att": dict(N=3, F=6, T=50, flooring="add", attenuation=0.4, alpha=1.25),
    "admmhva_n9_f12_none_init_noscale": dict(N=9, F=12, T=40, flooring="none", inject=True,
                                             scale_restoration=False),
    "admmhva_n2_f12_lambda_mdp": dict(N=2, F=12, T=40, flooring="lambda",
                                      scale_restoration="minimal_distortion_principle"),
    "admmhva_n3_f9_batch": dict(N=3, F=9, T=40, B=3),
}
CASES = list(SPECS)
DEFAULTS = dict(cls="MaskingADMMHVA", seed=1, B=1, rho=1.0, relaxation=1.0, alpha=None,
                attenuation=None, mask_iter=1, flooring="max", scale_restoration=True,
                reference_id=0, inject=False, n_iter=10)
SEEDS = range(1, 11)  # what the generator tries, in order


def spec_of(name):
    return dict(DEFAULTS, **SPECS[name])


def mixtures(spec):
    """admmbss_cases.mixtures: (N, F, T), or (B, N, F, T) with seed + 20 b."""
    return ac.mixtures(spec)


def injected(spec):
    """The injected states of a spec, ``auxiliary2`` / ``dual2`` without the penalty axis."""
    if not spec["inject"]:
        return {}
    init = ac.injected_state(spec["seed"], 1, spec["N"], spec["F"], spec["T"])
    init["auxiliary2"], init["dual2"] = init["auxiliary2"][0], init["dual2"][0]
    return init


def build_kwargs(spec, ns):
    """Constructor arguments; ``ns`` holds ``max_flooring`` / ``add_flooring``."""
    kwargs = dict(rho=spec["rho"], attenuation=spec["attenuation"], mask_iter=spec["mask_iter"],
                  flooring_fn=hc.flooring_of(spec["flooring"], ns),
                  scale_restoration=spec["scale_restoration"], reference_id=spec["reference_id"])
    if spec["alpha"] is None:
        kwargs["relaxation"] = spec["relaxation"]
    else:
        kwargs["alpha"] = spec["alpha"]
    return kwargs


def construct(classes, ns, spec, **extra):
    """``classes``: a mapping or module with MaskingADMMHVA."""
    cls = classes[spec["cls"]] if isinstance(classes, dict) else getattr(classes, spec["cls"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return cls(**build_kwargs(spec, ns), **extra)


def golden_spec(g):
    """The spec a fixture was made with, from its meta data."""
    alpha, att = float(g["meta_alpha"]), float(g["meta_attenuation"])
    shape = [int(v) for v in g["meta_shape"]]
    return dict(cls=str(g["meta_cls"]), seed=int(g["meta_seed"]), B=int(g["meta_B"]),
                rho=float(g["meta_rho"]), relaxation=float(g["meta_relaxation"]),
                alpha=None if np.isnan(alpha) else alpha,
                attenuation=None if np.isnan(att) else att, mask_iter=int(g["meta_mask_iter"]),
                flooring=str(g["meta_flooring"]),
                scale_restoration=_option(g["meta_scale_restoration"]),
                reference_id=int(g["meta_reference_id"]), inject="auxiliary10" in g,
                n_iter=int(g["meta_n_iter"]), N=shape[0], F=shape[1], T=shape[2])


def repr_objects(classes):
    """Objects whose ``repr`` the fixture admmhva_repr.npz holds."""
    cls = classes["MaskingADMMHVA"] if isinstance(classes, dict) else classes.MaskingADMMHVA
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        evaluated = cls()
        evaluated.mask_fn(hc.repr_probe())  # three sources: attenuation becomes 1 / 3
        return {
            "default": cls(),
            "attenuation_alpha_noscale": cls(rho=0.5, attenuation=0.25, alpha=1.25, mask_iter=3,
                                             scale_restoration=False),
            "default_after_mask": evaluated,
        }
