#!/usr/bin/env python3
"""WPD iterations beside two comparisons in the same process.

ms per WPD iteration of the mask form (ssspy_wpd_steps: STEPS iterations and the output walk in one
launch, divided by STEPS) at M=4, taps=10 (Lb=44) and at M=8, taps=7 (Lb=64), with N = 2 and 4 masks,
at 1 and 32 mixtures of F=1025, T=512, delay=3, beside
  * N times the WPE iteration of the same order (taps + 1 taps, so that L = Lb) on the same
    spectrograms: the operation-count expectation, R and the factorisation being the same size, and
  * the same WPD iteration written as a chain of torch operators (unfold, einsum,
    torch.linalg.cholesky, cholesky_solve) -- what a user would write today; it goes through the
    mixtures in chunks and through the sources one after the other (its stacked vectors are taps + 1
    times the input).
Medians of three regions after a warm-up, the methods of a shape alternating.

    python benchmarks/wpd.py [--small] > profiles/wpd.txt
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssspy_amd import _device as dv  # noqa: E402
from ssspy_amd import _lib, _ops  # noqa: E402
from ssspy_amd.utils.dataset import nmf_mixture_batch  # noqa: E402

REGIONS, STEPS = 3, 4
FLOOR = (_lib.FLOOR_MAX, 1e-6)
LOADING, DELAY, REF = 1e-6, 3, 0
ROUTE_NAMES = {_lib.WPD_ROUTE_RESIDENT: "resident", _lib.WPD_ROUTE_STREAMING: "streaming"}


def timed(fn, per):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / per


def stacked(X, taps, delay):
    """xb (B, F, T, Lb) of X (B, M, F, T)."""
    B, M, F, T = X.shape
    Xt = X.permute(0, 2, 3, 1)
    if taps == 0:
        return Xt
    pad = torch.zeros((B, M, F, delay + taps - 1), dtype=X.dtype, device=X.device)
    windows = torch.cat([pad, X], dim=-1)[..., :T + taps - 1].unfold(-1, taps, 1)  # (B, M, F, T, K)
    hist = windows.flip(-1).permute(0, 2, 3, 4, 1).reshape(B, F, T, taps * M)
    return torch.cat([Xt, hist], dim=-1)


def torch_iteration(X, mask, W, taps, delay):
    """One mask-form WPD iteration on X (B, M, F, T), mask (B, N, F, T), W (B, F, N, Lb) = conj(wb)
    with torch operators; returns the new W."""
    B, M, F, T = X.shape
    N = mask.shape[1]
    xb = stacked(X, taps, delay)
    Lb = xb.shape[-1]
    Xt = xb[..., :M]
    eye = torch.eye(Lb, dtype=X.dtype, device=X.device)
    out = []
    for n in range(N):
        m = mask[:, n]                                                        # (B, F, T)
        Phi = torch.einsum("bft,bfti,bftj->bfij", m.to(X.dtype), Xt, Xt.conj())
        Phi = Phi / m.sum(dim=-1).clamp(min=1e-10)[..., None, None]
        y = torch.einsum("bfl,bftl->bft", W[:, :, n], xb)
        lam = torch.clamp(y.real ** 2 + y.imag ** 2, min=FLOOR[1])
        R = torch.einsum("bftl,bftn->bfln", xb / lam[..., None], xb.conj()) / T
        tr = torch.diagonal(R, dim1=-2, dim2=-1).real.sum(dim=-1)
        R = R + (LOADING * tr / Lb)[..., None, None] * eye
        Z = torch.cholesky_solve(eye[:, :M].expand(B, F, Lb, M), torch.linalg.cholesky(R))
        A = Z @ Phi
        den = torch.diagonal(A[..., :M, :], dim1=-2, dim2=-1).real.sum(dim=-1)
        out.append((A[..., REF] / den[..., None]).conj())
    return torch.stack(out, dim=2)


def shape_times(label, X, mask, taps, chunk):
    B, M, F, T = X.shape
    N = mask.shape[1]
    Lb = (taps + 1) * M
    route, lds = _ops.wpd_route(B, M, N, F, T, taps)
    info = dv.zeros((2,), dv.i32, X.device)
    W = dv.zeros((B, F, N, Lb), dv.c128, X.device)
    Y = dv.empty((B, N, F, T), dv.c128, X.device)
    G = dv.zeros((B, F, Lb, M), dv.c128, X.device)
    Yw = dv.empty((B, M, F, T), dv.c128, X.device)

    def start():
        W.zero_()
        W[..., REF] = 1.0

    def wpd():
        start()
        _ops.wpd_steps(X, mask, None, W, taps, DELAY, REF, LOADING, FLOOR, STEPS, info, Y=Y)

    def wpe():
        G.zero_()
        _ops.wpe_steps(X, G, taps + 1, DELAY, (_lib.FLOOR_MAX, 1e-10), STEPS, info, Y=Yw)

    Wt = [None]

    def chain():
        parts = []
        for b0 in range(0, B, chunk):
            Xc, mc = X[b0:b0 + chunk], mask[b0:b0 + chunk]
            w = torch.zeros((Xc.shape[0], F, N, Lb), dtype=X.dtype, device=X.device)
            w[..., REF] = 1.0
            parts.append(torch_iteration(Xc, mc, w, taps, DELAY))
        Wt[0] = torch.cat(parts)

    entries = [("WPD kernel (" + ROUTE_NAMES[route] + ")", wpd, STEPS),
               ("WPE kernel, same order", wpe, STEPS), ("WPD torch operators", chain, 1)]
    for _, fn, _ in entries:
        fn()  # warm-up: first-use allocations, code loading
    ms = [[] for _ in entries]
    for _ in range(REGIONS):
        for k, (_, fn, per) in enumerate(entries):
            ms[k].append(timed(fn, per))
    # the two WPD forms agree: one iteration of each from wb = e_ref
    start()
    _ops.wpd_steps(X, mask, None, W, taps, DELAY, REF, LOADING, FLOOR, 1, info, Y=Y)
    agree = float((W - Wt[0]).abs().max())
    med = [statistics.median(v) for v in ms]
    expect = N * med[1]
    for (name, _, _), m, v in zip(entries, med, ms):
        print("{:26s} {:26s} {:10.4f} ms / iteration  (x{:.3f} of N WPE iterations, x{:.3f} of the "
              "torch chain; regions {})".format(label, name, m, m / expect, m / med[2],
                                                " ".join("{:.4f}".format(t) for t in v)), flush=True)
    print("{:26s} LDS {} bytes / workgroup; failed triples {}; max |W kernel - W torch| after 1 "
          "iteration {:.2e}".format(label, lds, int(info[0].item()), agree), flush=True)


def main():
    dev = torch.device("cuda", 0)
    shapes = []
    for M, taps, seed, chunk in ((4, 10, 1000, 4), (8, 7, 3000, 2)):
        for N in (2, 4):
            for B in (1, 32):
                shapes.append(("m{} k{} n{} f1025 t512 x{}".format(M, taps, N, B), seed, B, M, N, 1025,
                               512, taps, chunk))
    if "--small" in sys.argv:
        shapes = [("small m4 k10 n2 x2", 1000, 2, 4, 2, 33, 128, 10, 2),
                  ("small m8 k7 n4 x1", 3000, 1, 8, 4, 17, 600, 7, 1)]
    print("# WPD (mask form): ms per iteration, delay 3, max_flooring(1e-6), diagonal_loading 1e-6; {} "
          "iterations + the output walk in one launch, divided by {}".format(STEPS, STEPS))
    for label, seed, B, M, N, F, T, taps, chunk in shapes:
        X = torch.from_numpy(nmf_mixture_batch(seed, B, M, F, T)).to(dev)
        gen = torch.Generator(device="cpu").manual_seed(seed)
        mask = torch.rand((B, N, F, T), generator=gen, dtype=torch.float64) * 0.95 + 0.05
        mask = (mask / mask.sum(dim=1, keepdim=True)).to(dev)
        shape_times(label, X, mask, taps, chunk)
        del X, mask
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
