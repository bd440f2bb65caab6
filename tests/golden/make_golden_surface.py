#!/usr/bin/env python3
"""Golden vectors and the name table of the public surface that has no separator run of its own:
``update_by_ip2_one_pair``, the PSDTF reconstructions and normalisation of IPSDTA, ``quadratic``,
``cbrt``, ``solve_cubic``, ``softmax``, ``logsumexp`` and ``compute_logdet`` of ILRMA / IVA.

Runs ONLY where the reference checkout is available, as make_golden.py does (whose ``save`` and
``meta`` it reuses unchanged):

    python tests/golden/make_golden_surface.py

Writes ``tests/golden/surface_*.npz`` (inputs and the reference's outputs, float64 / complex128) and
``tests/golden/public_api.json``: for every reference module and class in scope the public names,
and for every callable its parameter names, read with ``inspect`` -- names only.  Re-running it
reproduces every file byte for byte.
"""

import functools
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import OUT_DIR, meta, save, skipped  # noqa: E402
import ssspy  # noqa: E402,F401
from ssspy.bss import _update_spatial_model as ref_spatial  # noqa: E402
from ssspy.bss.ilrma import GaussILRMA  # noqa: E402
from ssspy.bss.ipsdta import GaussIPSDTA, IPSDTABase  # noqa: E402
from ssspy.bss.iva import AuxLaplaceIVA  # noqa: E402
from ssspy.linalg import cbrt, quadratic, solve_cubic  # noqa: E402
from ssspy.special import logsumexp, softmax  # noqa: E402
from ssspy.special.flooring import add_flooring, max_flooring  # noqa: E402

# (N, pair) of the update_by_ip2_one_pair fixtures, F = 3
PAIR_CASES = ((2, (0, 1)), (3, (0, 1)), (3, (2, 0)), (4, (0, 1)), (4, (2, 0)), (9, (8, 3)))
PAIR_FLOORS = (("max", 1e-10), ("add", 1e-10))


def cgauss(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def pair_inputs(N, F, seed):
    """A well-conditioned filter and two positive definite covariances per bin."""
    rng = np.random.default_rng(seed)
    W = np.eye(N) + 0.3 * cgauss(rng, (F, N, N))
    A = cgauss(rng, (F, 2, N, 2 * N))
    U = A @ A.conj().swapaxes(-1, -2) / (2 * N)
    return W, U


def psd_basis(rng, shape):
    """(..., L, L) Hermitian positive semidefinite."""
    L = shape[-1]
    A = cgauss(rng, shape[:-1] + (L,))
    return A @ A.conj().swapaxes(-1, -2) / L


def gen_pair():
    for N, pair in PAIR_CASES:
        for kind, eps in PAIR_FLOORS:
            name = "surface_ip2_pair_n{}_{}{}_{}".format(N, pair[0], pair[1], kind)
            if skipped(name):
                continue
            W, U = pair_inputs(N, 3, 100 + N)
            fn = functools.partial(max_flooring if kind == "max" else add_flooring, eps=eps)
            out = ref_spatial.update_by_ip2_one_pair(W.copy(), U.copy(), pair, flooring_fn=fn)
            save(name, demix_filter=W, weighted_covariance_pair=U, pair=np.asarray(pair), out=out,
                 **meta(flooring=kind, eps=eps))


def gen_psdtf():
    N, K, T, C = 2, 3, 5, 2
    for L in (1, 2, 8):
        name = "surface_block_psdtf_l{}".format(L)
        if skipped(name):
            continue
        rng = np.random.default_rng(200 + L)
        basis = psd_basis(rng, (N, K, C, L, L))
        act = rng.random((N, K, T))
        m = GaussIPSDTA(n_basis=K, n_blocks=C)
        out = m.reconstruct_block_decomposition_psdtf(basis, act)
        last = np.ascontiguousarray(basis.transpose(0, 2, 3, 4, 1))
        out_last = m.reconstruct_block_decomposition_psdtf(last, act, axis1=-3, axis2=-2)
        save(name, basis=basis, basis_last=last, activation=act, out=out, out_last=out_last)
    name = "surface_block_psdtf_rem"
    if not skipped(name):
        rng = np.random.default_rng(210)
        low, high = psd_basis(rng, (N, K, 1, 2, 2)), psd_basis(rng, (N, K, 1, 3, 3))
        act = rng.random((N, K, T))
        m = GaussIPSDTA(n_basis=K, n_blocks=2)
        m.n_bins = 5
        out_low, out_high = m.reconstruct_block_decomposition_psdtf((low, high), act)
        save(name, basis_low=low, basis_high=high, activation=act, out_low=out_low, out_high=out_high,
             **meta(n_bins=5, n_blocks=2))
    for F in (4, 18):
        name = "surface_psdtf_f{}".format(F)
        if skipped(name):
            continue
        rng = np.random.default_rng(220 + F)
        basis = psd_basis(rng, (N, K, F, F))
        act = rng.random((N, K, T))
        m = IPSDTABase(n_basis=K)
        out = m.reconstruct_psdtf(basis, act)
        last = np.ascontiguousarray(basis.transpose(0, 2, 3, 1))
        out_last = m.reconstruct_psdtf(last, act, axis1=-3, axis2=-2)
        save(name, basis=basis, basis_last=last, activation=act, out=out, out_last=out_last)
    name = "surface_normalize_psdtf"
    if not skipped(name):
        rng = np.random.default_rng(230)
        basis = psd_basis(rng, (N, K, 4, 4))
        act = rng.random((N, K, T))
        m = IPSDTABase(n_basis=K)
        m.source_normalization = True
        m.basis, m.activation = basis.copy(), act.copy()
        m.normalize_psdtf()
        save(name, basis=basis, activation=act, out_basis=m.basis, out_activation=m.activation)


def gen_functions():
    name = "surface_quadratic"
    if not skipped(name):
        rng = np.random.default_rng(300)
        X, A = cgauss(rng, (3, 5, 4)), cgauss(rng, (3, 5, 4, 4))
        Xr, Ar = rng.standard_normal((6, 3)), rng.standard_normal((6, 3, 3))
        save(name, X=X, A=A, out=quadratic(X, A), X_real=Xr, A_real=Ar, out_real=quadratic(Xr, Ar))
    name = "surface_softmax"
    if not skipped(name):
        rng = np.random.default_rng(310)
        X = 5.0 * rng.standard_normal((3, 7, 4))
        X[0, 0, 0], X[1, 2, 3] = 700.0, -700.0
        arrays = {"X": X, "softmax_none": softmax(X), "logsumexp_none": np.asarray(logsumexp(X)),
                  "logsumexp_02": logsumexp(X, axis=(0, 2)),
                  "logsumexp_02_keep": logsumexp(X, axis=(0, 2), keepdims=True),
                  "softmax_02": softmax(X, axis=(0, 2))}
        for axis in (0, 1, 2):
            arrays["softmax_{}".format(axis)] = softmax(X, axis=axis)
            arrays["logsumexp_{}".format(axis)] = logsumexp(X, axis=axis)
        save(name, **arrays)
    name = "surface_cbrt"
    if not skipped(name):
        rng = np.random.default_rng(320)
        xr = np.concatenate([-rng.random(6) * 10, rng.random(6) * 10, [-8.0, 0.0, 27.0]])
        xc = cgauss(rng, (16,)) * 3
        save(name, x_real=xr, out_real=cbrt(xr), x_complex=xc, out_complex=cbrt(xc))
    name = "surface_solve_cubic"
    if not skipped(name):
        rng = np.random.default_rng(330)
        # monic: x^3 + A x^2 + B x + C; the last element has P = B - A^2 / 3 == 0 exactly
        A = np.concatenate([rng.standard_normal(11) * 2, [3.0]])
        B = np.concatenate([rng.standard_normal(11) * 2, [3.0]])
        C = np.concatenate([rng.standard_normal(11) * 2, [-7.0]])
        assert (B - A**2 / 3)[-1] == 0 and np.count_nonzero(B - A**2 / 3 == 0) == 1
        # general: A4 x^3 + B4 x^2 + C4 x + D4
        A4 = rng.standard_normal(8) + np.sign(rng.standard_normal(8)) * 0.5
        B4, C4, D4 = (rng.standard_normal(8) * 2 for _ in range(3))
        for a, b, c in ((A, B, C), (B4 / A4, C4 / A4, D4 / A4)):
            # no double root: the discriminant of the depressed cubic stays away from zero
            P, Q = b - a**2 / 3, 2 * a**3 / 27 - a * b / 3 + c
            disc = (Q / 2) ** 2 + (P / 3) ** 3
            assert (np.abs(disc) > 1e-3 * ((Q / 2) ** 2 + np.abs(P / 3) ** 3)).all(), disc
        save(name, A=A, B=B, C=C, roots=solve_cubic(A, B, C), first=solve_cubic(A, B, C, all=False),
             A4=A4, B4=B4, C4=C4, D4=D4, roots4=solve_cubic(A4, B4, C4, D4),
             first4=solve_cubic(A4, B4, C4, D4, all=False))
    name = "surface_logdet"
    if not skipped(name):
        rng = np.random.default_rng(340)
        W3, W2 = cgauss(rng, (5, 3, 3)), cgauss(rng, (4, 2, 2))
        save(name, W_ilrma=W3, logdet_ilrma=GaussILRMA(n_basis=2).compute_logdet(W3),
             W_iva=W2, logdet_iva=AuxLaplaceIVA().compute_logdet(W2))


# reference modules (and the classes of those named in CLASS_MODULES) whose public names the table holds
API_MODULES = ("ssspy.linalg", "ssspy.special", "ssspy.algorithm", "ssspy.bss._update_spatial_model",
               "ssspy.utils.flooring", "ssspy.utils.select_pair")
CLASS_MODULES = ("ssspy.bss.ilrma", "ssspy.bss.iva", "ssspy.bss.ipsdta", "ssspy.bss.fdica",
                 "ssspy.bss.mnmf", "ssspy.bss.cacgmm", "ssspy.bss.ica", "ssspy.bss.pdsbss",
                 "ssspy.bss.admmbss", "ssspy.bss.hva", "ssspy.bss.proxbss")


def parameters(fn):
    try:
        return [p.name for p in inspect.signature(fn).parameters.values()
                if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY)]
    except (TypeError, ValueError):
        return None


def gen_api():
    import importlib

    table = {}
    for modname in API_MODULES:
        mod = importlib.import_module(modname)
        names = getattr(mod, "__all__", None) or [
            n for n, v in vars(mod).items()
            if not n.startswith("_") and inspect.isfunction(v) and v.__module__ == modname]
        entry = {}
        for n in sorted(names):
            v = getattr(mod, n)
            entry[n] = parameters(v) if inspect.isfunction(v) else None
        table[modname] = entry
    for modname in CLASS_MODULES:
        mod = importlib.import_module(modname)
        # the classes the module exports (every public class it defines where it names none), each
        # with what a user can reach on it: inherited methods and properties included
        exported = getattr(mod, "__all__", None)
        for cname, cls in sorted(vars(mod).items()):
            if not inspect.isclass(cls) or cls.__module__ != modname or cname.startswith("_"):
                continue
            if exported is not None and cname not in exported:
                continue
            entry = {"__init__": parameters(cls.__init__)}
            for n, v in inspect.getmembers(cls):
                if n.startswith("_"):
                    continue
                if inspect.isfunction(v):
                    entry[n] = parameters(v)
                elif isinstance(v, property):
                    entry[n] = None
            table[modname + "." + cname] = entry
    with open(os.path.join(OUT_DIR, "public_api.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    gen_pair()
    gen_psdtf()
    gen_functions()
    gen_api()
