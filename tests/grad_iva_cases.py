"""What the CPU and the GPU tests of the gradient IVA classes share: the list of fixtures, the
constructor arguments a fixture was made with, the closures and the flooring callable of
tests/golden/make_golden_grad_iva.py, the snapshot callback and the comparison with a fixture."""

import functools

import numpy as np

from conftest import load_golden, rel_err
from conftest import option as _option

CASES = [
    "gradiva_nglap_n2", "gradiva_nglap_n3_nonhol_add", "gradiva_glap_n4_init",
    "gradiva_glap_n3_nonhol_maxfloor", "gradiva_ngauss_n6", "gradiva_ggauss_n2_nonhol",
    "gradiva_ggauss_n8", "gradiva_nglap_n8_nonhol", "gradiva_glap_n10",
    "gradiva_ngauss_n12_nonhol", "gradiva_nglap_n4_customfloor", "gradiva_generic_ng_n3",
]

GENERIC_FLOOR = 1e-10  # (the closures of make_golden_grad_iva.py)


def custom_floor(x):
    """make_golden.custom_floor: none of the reference's three flooring functions."""
    return np.maximum(x, 1e-8) + 1e-12


def generic_contrast_fn(y):
    return 2 * np.linalg.norm(y, axis=1)


def generic_score_fn(y):
    norm = np.linalg.norm(y, axis=1, keepdims=True)
    return y / np.maximum(norm, GENERIC_FLOOR)


def golden_kwargs(g, flooring_fns):
    """Constructor arguments a fixture was made with; ``flooring_fns``: the namespace that provides
    max_flooring / add_flooring (the restatement's or the package's)."""
    kind, eps = str(g["meta_floor_kind"]), float(g["meta_floor_eps"])
    if kind == "max":
        floor = functools.partial(flooring_fns.max_flooring, eps=eps)
    elif kind == "add":
        floor = functools.partial(flooring_fns.add_flooring, eps=eps)
    elif kind == "custom":
        floor = custom_floor
    else:
        floor = None
    kwargs = dict(step_size=float(g["meta_step_size"]), flooring_fn=floor,
                  is_holonomic=bool(g["meta_is_holonomic"]),
                  scale_restoration=_option(g["meta_scale_restoration"]),
                  reference_id=int(g["meta_reference_id"]))
    if str(g["meta_cls"]) in ("GradIVA", "NaturalGradIVA"):
        kwargs.update(contrast_fn=generic_contrast_fn, score_fn=generic_score_fn)
    return kwargs


def golden_init(g):
    return {"demix_filter": g["demix_filter0"]} if "demix_filter0" in g else {}


class Snapshots:
    def __init__(self, names=("demix_filter", "variance")):
        self.names, self.count, self.store = names, -1, {}

    def __call__(self, method):
        self.count += 1
        for name in self.names:
            value = getattr(method, name, None)
            if value is not None:
                self.store["it{}_{}".format(self.count, name)] = np.array(value, copy=True)


def check_against_golden(g, m, Y, snap, tol, loss_rtol):
    """The snapshots the fixture holds, the loss list, the final filters and the output."""
    checked = 0
    for key in g:
        if key.startswith("it"):
            assert rel_err(snap.store[key], g[key]) < tol, key
            checked += 1
    assert checked >= 2
    np.testing.assert_allclose(np.array(m.loss), g["loss"], rtol=loss_rtol)
    assert rel_err(np.asarray(m.demix_filter), g["final_demix_filter"]) < tol
    assert rel_err(Y, g["final_output"]) < tol

