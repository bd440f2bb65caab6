#!/usr/bin/env python3
"""Bit-for-bit comparison of two builds of the library on everything the per-lane Hermitian routines
(csrc/hermitian.hpp) reach: the ssspy.linalg operators at one size per route, and the separators that
call the routines, at the smallest shape that reaches each route.

    SSSPY_AMD_LIB=<build A> python benchmarks/tools/lane_linalg_bits.py dump a.npz
    SSSPY_AMD_LIB=<build B> python benchmarks/tools/lane_linalg_bits.py dump b.npz     (fresh process)
    python benchmarks/tools/lane_linalg_bits.py compare a.npz b.npz  -> entry point, arrays, differing

Inputs: the families of tests/linalg_reference.py, interleaved as its test interleaves them (the
clustered and graded ones decide the sweep counts, and so the bits); batches 72, 33 and 1.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def operators(out):
    import linalg_reference as lr
    import test_gpu_linalg_elementwise as t

    def put(entry, case, arrays):
        for i, a in enumerate(arrays if isinstance(arrays, (tuple, list)) else [arrays]):
            out["{}|{}|{}".format(entry, case, i)] = np.asarray(a)

    for M in lr.SIZES:
        A, _ = lr.gen_hermitian(0, t.N, M)
        X = lr.gen_pd(0, t.N, M)
        Ap, Bp, _ = lr.gen_pd_pairs(0, t.N, M)
        for n in t.BATCHES:
            case = "M{} n{}".format(M, n)
            put("ssspy_eigh", case, t.run_eigh(A[:n]))
            for fl in lr.FLOORS:
                put("ssspy_to_psd", "{} floor{}".format(case, fl), t.run_to_psd(A[:n], fl))
                put("ssspy_sqrtmh", "{} inverse floor{}".format(case, fl), t.run_sqrtmh(X[:n], 1, fl))
            put("ssspy_sqrtmh", case, t.run_sqrtmh(X[:n], 0))
            for type in (1, 2, 3):
                put("ssspy_gmeanmh", "{} type{}".format(case, type), t.run_gmeanmh(Ap[:n], Bp[:n], type))
                put("ssspy_eigh_general", "{} type{}".format(case, type),
                    t.run_general(Ap[:n], Bp[:n], type, "eigh_general")[:2])
    for Nn in lr.SOLVE_SIZES:
        A, Bm, _ = lr.gen_systems(0, t.N, Nn, 3)
        for n in t.BATCHES:
            put("ssspy_solve", "N{} n{}".format(Nn, n), t.run_solve(A[:n], Bm[:n])[0])


def mixtures(seed, batch, channels, F, T):
    rng = np.random.default_rng(seed)
    shape = (batch, channels, F, T)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def separators(out):
    import fast_iva_cases as fc
    from ssspy_amd.special.flooring import max_flooring
    from ssspy_amd.bss.ilrma import GaussILRMA
    from ssspy_amd.bss.ipsdta import GaussIPSDTA
    from ssspy_amd.bss.iva import FasterIVA, FastIVA
    from ssspy_amd.bss.mnmf import FastGaussMNMF, GaussMNMF

    acting = functools.partial(max_flooring, eps=0.5)   # an eigenvalue floor that acts: the repair route
    rng = lambda: np.random.default_rng(7)              # noqa: E731
    cases = []
    for n in (2, 7, 9):                                 # the three flavours of the Jacobi descriptor
        cases.append(("FastIVA", "N{}".format(n), n, lambda: FastIVA(**fc.closures_for("FastIVA", "laplace"))))
        cases.append(("FasterIVA", "N{}".format(n), n, lambda: FasterIVA(**fc.closures_for("FasterIVA", "laplace"))))
    for m in (4, 5, 6):                                 # psd_eigen unrolled (4) and rolled (5, 6)
        cases.append(("GaussMNMF", "M{}".format(m), m,
                      lambda: GaussMNMF(n_basis=2, n_sources=2, flooring_fn=acting, rng=rng())))
    for m in (5, 8, 9):                                 # fmnmf_generic.hip (5, 8), fmnmf_rt.hip (9)
        cases.append(("FastGaussMNMF", "M{}".format(m), m,
                      lambda: FastGaussMNMF(n_basis=2, flooring_fn=acting, rng=rng())))
    for n in (3, 9):                                    # ipa_kernels.hip, ipa_rt.hip
        cases.append(("GaussILRMA-IPA", "N{}".format(n), n,
                      lambda: GaussILRMA(n_basis=2, spatial_algorithm="IPA", rng=rng())))
    for blocks, F in ((2, 8), (1, 6)):                  # block size 4 and 6 (above 4: rolled rebuild)
        cases.append(("GaussIPSDTA", "F{} blocks{}".format(F, blocks), 2,
                      lambda blocks=blocks: GaussIPSDTA(n_basis=2, n_blocks=blocks, rng=rng())))
    for name, case, channels, make in cases:
        F = int(case[1:case.index(" ")]) if name == "GaussIPSDTA" else 7
        for batch in (2, 33):
            x = mixtures(channels * 100 + batch, batch, channels, F, 12)
            m = make()
            y = m(x, n_iter=2)
            key = "{}|{} B{}".format(name, case, batch)
            out[key + "|0"] = np.asarray(y)
            for i, attr in enumerate(("demix_filter", "spatial", "basis", "activation", "loss")):
                v = getattr(m, attr, None)
                if v is not None:
                    out["{}|{}".format(key, i + 1)] = np.asarray(v)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different arrays"
    count, differ = {}, {}
    for k in a.files:
        entry = k.split("|")[0]
        count[entry] = count.get(entry, 0) + 1
        same = a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))
        differ[entry] = differ.get(entry, 0) + (0 if same else 1)
        if not same:
            print("# differs: " + k)
    print("{:24s} {:>8s} {:>8s}".format("entry point", "arrays", "differ"))
    for entry in sorted(count):
        print("{:24s} {:8d} {:8d}".format(entry, count[entry], differ[entry]))
    return sum(differ.values())


if __name__ == "__main__":
    if sys.argv[1] == "compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    out = {}
    if "separators" not in sys.argv[3:]:
        operators(out)
    if "operators" not in sys.argv[3:]:
        separators(out)
    np.savez(sys.argv[2], **{k: np.ascontiguousarray(v) for k, v in out.items()})
    print("{} arrays with {}".format(len(out), os.environ.get("SSSPY_AMD_LIB", "the tree's library")))
