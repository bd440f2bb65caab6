"""What the CPU and the GPU tests of the FDICA classes share: the list of fixtures, the constructor
arguments a fixture was made with, the closures and the flooring callable of
tests/golden/make_golden_fdica.py, the snapshot callback and the comparison with a fixture."""

import functools
import itertools

import numpy as np

from conftest import rel_err
from conftest import option as _option

CASES = [
    "fdica_glap_n2", "fdica_glap_n3_hol_add", "fdica_nglap_n4_init", "fdica_nglap_n3_hol_maxfloor",
    "fdica_nglap_n8_mdp", "fdica_glap_n8_hol_noperm", "fdica_aux_ip1_n2", "fdica_aux_ip1_n4_init_none",
    "fdica_aux_ip1_n8_mdp", "fdica_aux_ip2_n3", "fdica_aux_ip2_n4_comb", "fdica_aux_ip1_n3_customfloor",
    "fdica_aux_ip1_n10_noperm", "fdica_generic_grad_n3", "fdica_generic_aux_ip2_n3",
]

GENERIC_FLOOR = 1e-10  # (the closures of make_golden_fdica.py)
GENERIC = ("GradFDICA", "NaturalGradFDICA", "AuxFDICA")


def custom_floor(x):
    """make_golden.custom_floor: none of the reference's three flooring functions."""
    return np.maximum(x, 1e-8) + 1e-12


def generic_contrast_fn(y):
    return 2 * np.abs(y)


def generic_score_fn(y):
    return y / np.maximum(np.abs(y), GENERIC_FLOOR)


def generic_d_contrast_fn(y):
    return 2 * np.ones_like(y)


def combination_pairs(n_sources):
    return itertools.combinations(range(n_sources), 2)


def floor_of(kind, eps, flooring_fns):
    if kind == "max":
        return functools.partial(flooring_fns.max_flooring, eps=eps)
    if kind == "add":
        return functools.partial(flooring_fns.add_flooring, eps=eps)
    if kind == "custom":
        return custom_floor
    return None


def golden_kwargs(g, flooring_fns):
    """Constructor arguments a fixture was made with; ``flooring_fns``: the namespace that provides
    max_flooring / add_flooring (the restatement's or the package's)."""
    cls = str(g["meta_cls"])
    kwargs = dict(flooring_fn=floor_of(str(g["meta_floor_kind"]), float(g["meta_floor_eps"]),
                                       flooring_fns),
                  permutation_alignment=bool(g["meta_permutation_alignment"]),
                  scale_restoration=_option(g["meta_scale_restoration"]),
                  reference_id=int(g["meta_reference_id"]))
    if "Aux" in cls:
        kwargs["spatial_algorithm"] = str(g["meta_spatial_algorithm"])
        if str(g["meta_pair_selector"]) == "combination":
            kwargs["pair_selector"] = combination_pairs
        if cls in GENERIC:
            kwargs.update(contrast_fn=generic_contrast_fn, d_contrast_fn=generic_d_contrast_fn)
    else:
        kwargs.update(step_size=float(g["meta_step_size"]),
                      is_holonomic=bool(g["meta_is_holonomic"]))
        if cls in GENERIC:
            kwargs.update(contrast_fn=generic_contrast_fn, score_fn=generic_score_fn)
    return kwargs


def golden_init(g):
    return {"demix_filter": g["demix_filter0"]} if "demix_filter0" in g else {}


class Snapshots:
    def __init__(self, names=("demix_filter",)):
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
    assert checked >= 3
    np.testing.assert_allclose(np.array(m.loss), g["loss"], rtol=loss_rtol)
    assert rel_err(np.asarray(m.demix_filter), g["final_demix_filter"]) < tol
    assert rel_err(Y, g["final_output"]) < tol
