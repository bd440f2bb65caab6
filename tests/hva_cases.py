"""What the fixture generator (tests/golden/make_golden_hva.py) and the CPU and GPU tests of the HVA
classes share: the list of fixtures and how each was made, the flooring functions by name, the
``repr`` objects and the inputs of the mask fixture.  Mixtures, injected states, snapshots and the
comparison with a fixture are those of tests/pdsbss_cases.py."""

import functools
import warnings

import numpy as np

from conftest import option as _option

# name -> how the fixture is made.  flooring: a key of ``flooring_of``.
SPECS = {
    "hva_n2_f9": dict(N=2, F=9, T=40),
    "hva_n3_f17_iter3": dict(N=3, F=17, T=50, mask_iter=3, reference_id=1),
    "hva_n4_f33_iter0_init": dict(N=4, F=33, T=40, mask_iter=0, inject=True),
    "hva_n3_f6_add_att": dict(N=3, F=6, T=50, flooring="add", attenuation=0.4, relaxation=1.25),
    "hva_n9_f12_none_noscale": dict(N=9, F=12, T=40, flooring="none", scale_restoration=False),
    "hva_n2_f12_lambda_mdp": dict(N=2, F=12, T=40, cls="HVA", flooring="lambda", mu1=0.5,
                                  scale_restoration="minimal_distortion_principle"),
}
CASES = list(SPECS)
DEFAULTS = dict(cls="MaskingPDSHVA", seed=1, mu1=1.0, mu2=1.0, relaxation=1.0, alpha=None,
                attenuation=None, mask_iter=1, flooring="max", scale_restoration=True,
                reference_id=0, inject=False, n_iter=10)
LAMBDA_EPS = 1e-8
MASK_BINS = (2, 3, 9, 12)  # the mask fixture: Z, mask and varrho at these bin counts
MASK_SOURCES, MASK_FRAMES, MASK_ITER, MASK_ATTENUATION = 3, 7, 2, 0.5


def spec_of(name):
    return dict(DEFAULTS, **SPECS[name])


def flooring_of(name, ns):
    """``flooring_fn`` by name; ``ns`` holds ``max_flooring`` / ``add_flooring``.  "lambda" is none of
    the recognised callables: the compatibility route."""
    if name == "max":
        return functools.partial(ns.max_flooring, eps=1e-10)
    if name == "add":
        return functools.partial(ns.add_flooring, eps=1e-6)
    if name == "none":
        return None
    if name == "lambda":
        return lambda x: np.maximum(x, LAMBDA_EPS) + 0.0
    raise KeyError(name)


def build_kwargs(spec, ns):
    kwargs = dict(mu1=spec["mu1"], mu2=spec["mu2"], attenuation=spec["attenuation"],
                  mask_iter=spec["mask_iter"], flooring_fn=flooring_of(spec["flooring"], ns),
                  scale_restoration=spec["scale_restoration"], reference_id=spec["reference_id"])
    if spec["alpha"] is None:
        kwargs["relaxation"] = spec["relaxation"]
    else:
        kwargs["alpha"] = spec["alpha"]
    return kwargs


def construct(classes, ns, spec, **extra):
    """``classes``: a mapping or module with MaskingPDSHVA / HVA."""
    cls = classes[spec["cls"]] if isinstance(classes, dict) else getattr(classes, spec["cls"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return cls(**build_kwargs(spec, ns), **extra)


def golden_spec(g):
    """The spec a fixture was made with, from its meta data."""
    alpha, att = float(g["meta_alpha"]), float(g["meta_attenuation"])
    return dict(cls=str(g["meta_cls"]), seed=int(g["meta_seed"]), mu1=float(g["meta_mu1"]),
                mu2=float(g["meta_mu2"]), relaxation=float(g["meta_relaxation"]),
                alpha=None if np.isnan(alpha) else alpha,
                attenuation=None if np.isnan(att) else att, mask_iter=int(g["meta_mask_iter"]),
                flooring=str(g["meta_flooring"]),
                scale_restoration=_option(g["meta_scale_restoration"]),
                reference_id=int(g["meta_reference_id"]), inject="demix_filter0" in g,
                n_iter=int(g["meta_n_iter"]), N=int(g["meta_shape"][0]), F=int(g["meta_shape"][1]),
                T=int(g["meta_shape"][2]))


def repr_objects(classes):
    """Objects whose ``repr`` the fixture hva_repr.npz holds, before (key) and after (key + "_after")
    the first evaluation of the mask."""
    get = classes.__getitem__ if isinstance(classes, dict) else functools.partial(getattr, classes)
    pds, hva = get("MaskingPDSHVA"), get("HVA")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return {
            "pds_default": pds(),
            "hva_default": hva(),
            "pds_attenuation": pds(mu1=0.5, mu2=2, relaxation=1.5, attenuation=0.25, mask_iter=3,
                                   reference_id=2,
                                   scale_restoration="minimal_distortion_principle"),
            "hva_alpha_noscale": hva(alpha=1.25, mask_iter=0, scale_restoration=False,
                                     record_loss=False),
        }


def repr_probe():
    """The array whose mask the repr objects evaluate once: three sources."""
    rng = np.random.default_rng(5)
    return rng.standard_normal((3, 5, 4)) + 1j * rng.standard_normal((3, 5, 4))


def mask_input(F):
    rng = np.random.default_rng(100 + F)
    shape = (MASK_SOURCES, F, MASK_FRAMES)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
