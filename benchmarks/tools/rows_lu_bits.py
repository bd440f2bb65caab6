#!/usr/bin/env python3
"""Bit-for-bit comparison of two builds of the library on every kernel that solves through the
row-distributed LU of csrc/rows_lu.hpp, the operators of ssspy_amd._ops driven directly at the smallest
shapes that reach each instantiation.

    SSSPY_AMD_LIB=<build A> python benchmarks/tools/rows_lu_bits.py dump a.npz
    SSSPY_AMD_LIB=<build B> python benchmarks/tools/rows_lu_bits.py dump b.npz     (fresh process)
    python benchmarks/tools/rows_lu_bits.py compare a.npz b.npz  -> entry point, arrays, differing

Inputs: the generators of the elementwise tests (pass_reference, test_gpu_spatial_pass_elementwise)
and the recipes of test_gpu_grad_iva / test_gpu_fdica's operator tests.  B = 2, F = 17: 34 bins
against 32 per workgroup of the 8-lane kernels, so idle lane groups exist.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, F = 2, 17


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def dump(out):
    import torch

    import pass_reference as pr
    import test_gpu_pass_elementwise as tp
    import test_gpu_spatial_pass_elementwise as ts
    from ssspy_amd import _device as dv
    from ssspy_amd import _lib
    from ssspy_amd import _ops as ops

    def dev(a):
        return dv.to_device(np.ascontiguousarray(a), dtype=np.asarray(a).dtype)

    def put(entry, case, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            out["{}|{}|{}".format(entry, case, i)] = np.array(dv.to_host(t))

    # ---- IP1 on 8 lanes per bin (k_ip1_rows), once more with a zero covariance: the zero pivot, info
    for N in (5, 6, 7, 8):
        W, Uc = pr.gen_ip1_inputs(80 + N + B, B, F, N)
        for case, U in (("N{}".format(N), Uc), ("N{} zero bin".format(N), Uc.copy())):
            if "zero" in case:
                U[1, 3] = 0.0
            info = dv.zeros((1,), dv.i32)
            Wd = dev(W)
            ops.update_by_ip1(Wd, dev(U), tp.MAXF, info)
            put("update_by_ip1", case, Wd, info)
            slots = ops.update_by_ip1_logdet_slots(B, F, N)
            Wd, shares = dev(W), dv.zeros((slots, B), dv.f64)
            info = dv.zeros((1,), dv.i32)
            ops.update_by_ip1_logdet(Wd, dev(U), tp.MAXF, info, shares, B)
            put("update_by_ip1_logdet", case, Wd, info, shares)

    # ---- IP2 on 8 lanes per bin (k_ip2_rows)
    for N in (5, 6, 7, 8):
        for pair_only in (0, 1):
            pairs = [(N - 1, 0)] if pair_only else ts.pair_lists(N)["seq"]
            W, Uc, _ = ts._ip2_inputs(900 + 7 * N + F + pair_only, B, F, N, pairs, pair_only)
            info = dv.zeros((1,), dv.i32)
            Wd = dev(W)
            ops.update_by_ip2(Wd, dev(Uc), pairs, tp.MAXF, info=info, pair_only=bool(pair_only))
            put("update_by_ip2", "N{} pair_only{}".format(N, pair_only), Wd, info)

    # ---- the fused ILRMA step on the latency route (k_ip1_small)
    T, K = 40, 12
    model, domain = tp.G2
    for N in (2, 3, 4):
        assert ops.ilrma_route(B, N, F, T, K, domain, model)[0] == tp.LAT
        X, W, basis, act, C = pr.gen_fused_inputs(300 + B + N + K, B, N, F, T, K)
        for normalize in (False, True):
            for with_slots in (False, True):
                ws, wsb = ops.ilrma_workspace(B, N, F, T, K, dv.device())
                Wd, bd, ad = dev(W), dev(basis), dev(act)
                Ud = dv.zeros((B, F, N, N, N), dv.c128)
                info = dv.zeros((1,), dv.i32)
                args = (dev(X), dev(C), Wd, bd, ad, Ud, domain, normalize, tp.MAXF, ws, wsb, info)
                case = "N{} normalize{}".format(N, int(normalize))
                if with_slots:
                    ns = ops.ilrma_deferred_loss_slots(B, N, F, T, K, domain, model)
                    nl = ops.ilrma_deferred_logdet_slots(B, N, F, T, K, domain, model)
                    sl, ll = dv.zeros((ns, B), dv.f64), dv.zeros((nl, B), dv.f64)
                    ops.ilrma_ip1_update_loss_slots(*args, sl, B, ll, model=model)
                    put("ilrma_ip1_update_loss_slots", case, Wd, bd, ad, info, sl, ll)
                else:
                    ops.ilrma_ip1_update(*args, model=model)
                    put("ilrma_ip1_update", case, Wd, bd, ad, info)

    # ---- the gradient IVA step (k_grad_step_rows), the inputs of test_step_operator_against_numpy
    for N in (2, 3, 4, 5, 8):
        rng = np.random.default_rng(600 + N)
        W = np.eye(N) + 0.3 * crandn(rng, B, F, N, N)
        A = crandn(rng, B, F, N, N, 2 * N)
        U = A @ A.conj().swapaxes(-1, -2) / (2 * N)
        slots = ops.iva_grad_step_logdet_slots(B, F, N)
        for natural in (True, False):
            for holonomic in (True, False):
                for with_logdet in (False, True):
                    Wd, info = dev(W), dv.zeros((2,), dv.i32)
                    shares = dv.zeros((slots, B), dv.f64)
                    ops.iva_grad_step(Wd, dev(U), natural, holonomic, 0.1, info,
                                      logdet=shares if with_logdet else None, logdet_stride=B)
                    put("iva_grad_step", "N{} natural{} holonomic{} logdet{}".format(
                        N, int(natural), int(holonomic), int(with_logdet)), Wd, info, shares)

    # ---- the bin-resident FDICA iterations (k_fdica_steps), the inputs of
    # test_steps_operator_against_numpy; T = 800 at 4 sources is the form that re-reads the slab
    Ff, steps = 5, 3
    for N, T in ((2, 40), (3, 40), (4, 40), (4, 800)):
        rng = np.random.default_rng(740 + N)
        X = crandn(rng, B, N, Ff, T)
        W = np.eye(N) + 0.3 * crandn(rng, B, Ff, N, N)
        S = (steps + 1) * B
        for alg in (_lib.FDICA_GRAD, _lib.FDICA_NATURAL_GRAD, _lib.FDICA_AUX_IP1):
            for holonomic in (False, True):
                Wd, info = dev(W), dv.zeros((2,), dv.i32)
                loss, logdet = dv.zeros((Ff, S), dv.f64), dv.zeros((Ff, S), dv.f64)
                ops.fdica_steps(dev(X), Wd, alg, holonomic, 0.1, (_lib.FLOOR_MAX, 1e-10), steps, info,
                                loss, logdet, S)
                put("fdica_steps", "N{} T{} alg{} holonomic{}".format(N, T, alg, int(holonomic)),
                    Wd, info, loss, logdet)


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
    print("{:32s} {:>8s} {:>8s}".format("entry point", "arrays", "differ"))
    for entry in sorted(count):
        print("{:32s} {:8d} {:8d}".format(entry, count[entry], differ[entry]))
    return sum(differ.values())


if __name__ == "__main__":
    if sys.argv[1] == "compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    out = {}
    dump(out)
    assert all(np.all(np.isfinite(v)) for k, v in out.items() if "zero bin" not in k)
    np.savez(sys.argv[2], **{k: np.ascontiguousarray(v) for k, v in out.items()})
    print("{} arrays with {}".format(len(out), os.environ.get("SSSPY_AMD_LIB", "the tree's library")))
