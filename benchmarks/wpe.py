#!/usr/bin/env python3
"""WPE iterations beside two comparisons in the same process.

ms per WPE iteration (ssspy_wpe_steps: STEPS iterations and the output walk in one launch, divided by
STEPS) at M=4, F=1025, T=512, taps=10, delay=3 with 1, 32 and 128 mixtures and at M=8, taps=8 with
one mixture, beside
  * the AuxLaplaceIVA-IP1 iteration on the same spectrograms, the project's usual yardstick, and
  * the same WPE iteration written as a chain of torch operators (unfold, einsum,
    torch.linalg.cholesky, cholesky_solve) -- what a user would write today; batches go through it
    in chunks of 8 mixtures (its stacked history is taps times the input).
Medians of three regions after a warm-up, the methods of a shape alternating.

    python benchmarks/wpe.py [--small] > profiles/wpe.txt
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssspy_amd import _device as dv  # noqa: E402
from ssspy_amd import _lib, _ops  # noqa: E402
from ssspy_amd.bss.iva import AuxLaplaceIVA  # noqa: E402
from ssspy_amd.utils.dataset import nmf_mixture_batch  # noqa: E402

REGIONS, STEPS, IVA_ITERS, TORCH_CHUNK = 3, 4, 10, 8
FLOOR = (_lib.FLOOR_MAX, 1e-10)
ROUTE_NAMES = {_lib.WPE_ROUTE_RESIDENT: "resident", _lib.WPE_ROUTE_STREAMING: "streaming"}


def timed(fn, per):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / per


def torch_iteration(X, G, taps, delay, eps):
    """One WPE iteration on X (B, M, F, T), G (B, F, L, M) with torch operators; returns the new G."""
    B, M, F, T = X.shape
    pad = torch.zeros((B, M, F, delay + taps - 1), dtype=X.dtype, device=X.device)
    windows = torch.cat([pad, X], dim=-1)[..., :T + taps - 1].unfold(-1, taps, 1)  # (B, M, F, T, K)
    xs = windows.flip(-1).permute(0, 2, 3, 4, 1).reshape(B, F, T, taps * M)
    Xt = X.permute(0, 2, 3, 1)
    Y = Xt - torch.einsum("bflm,bftl->bftm", G.conj(), xs)
    lam = torch.clamp((Y.real ** 2 + Y.imag ** 2).mean(dim=-1), min=eps)
    weighted = xs / lam[..., None]
    R = torch.einsum("bftl,bftn->bfln", weighted, xs.conj())
    P = torch.einsum("bftl,bftm->bflm", weighted, Xt.conj())
    return torch.cholesky_solve(P, torch.linalg.cholesky(R))


def shape_times(label, X, taps, delay):
    B, M, F, T = X.shape
    L = taps * M
    route, lds = _ops.wpe_route(B, M, F, T, taps)
    info = dv.zeros((2,), dv.i32, X.device)
    G = dv.zeros((B, F, L, M), dv.c128, X.device)
    Y = dv.empty((B, M, F, T), dv.c128, X.device)

    def wpe():
        G.zero_()
        _ops.wpe_steps(X, G, taps, delay, FLOOR, STEPS, info, Y=Y)

    iva = AuxLaplaceIVA(spatial_algorithm="IP", scale_restoration=False, record_loss=False)
    iva._bind_input(X)
    iva._reset()

    def yardstick():
        for _ in range(IVA_ITERS):
            iva.update_once()

    Gt = [None]

    def chain():
        parts = []
        for b0 in range(0, B, TORCH_CHUNK):
            Xc = X[b0:b0 + TORCH_CHUNK]
            g = torch.zeros((Xc.shape[0], F, L, M), dtype=X.dtype, device=X.device)
            for _ in range(2):
                g = torch_iteration(Xc, g, taps, delay, FLOOR[1])
            parts.append(g)
        Gt[0] = torch.cat(parts)

    entries = [("WPE kernel (" + ROUTE_NAMES[route] + ")", wpe, STEPS),
               ("AuxLaplaceIVA-IP1", yardstick, IVA_ITERS), ("WPE torch operators", chain, 2)]
    for _, fn, _ in entries:
        fn()  # warm-up: first-use allocations, code loading
    ms = [[] for _ in entries]
    for _ in range(REGIONS):
        for k, (_, fn, per) in enumerate(entries):
            ms[k].append(timed(fn, per))
    # the two WPE forms agree: two iterations of each from G = 0
    G.zero_()
    _ops.wpe_steps(X, G, taps, delay, FLOOR, 2, info, Y=Y)
    agree = float((G - Gt[0]).abs().max())
    med = [statistics.median(v) for v in ms]
    for (name, _, _), m, v in zip(entries, med, ms):
        print("{:24s} {:26s} {:10.4f} ms / iteration  (x{:.3f} of the yardstick, x{:.3f} of the torch "
              "chain; regions {})".format(label, name, m, m / med[1], m / med[2],
                                          " ".join("{:.4f}".format(t) for t in v)), flush=True)
    print("{:24s} LDS {} bytes / workgroup; singular bins {}; max |G kernel - G torch| after 2 "
          "iterations {:.2e}".format(label, lds, int(info[0].item()), agree), flush=True)


def main():
    dev = torch.device("cuda", 0)
    shapes = [("m4 k10 f1025 t512 x1", 1000, 1, 4, 1025, 512, 10), ("m4 k10 f1025 t512 x32", 1000, 32, 4, 1025, 512, 10),
              ("m4 k10 f1025 t512 x128", 1000, 128, 4, 1025, 512, 10), ("m8 k8 f1025 t512 x1", 3000, 1, 8, 1025, 512, 8)]
    if "--small" in sys.argv:
        shapes = [("small m4 k10 x2", 1000, 2, 4, 33, 128, 10), ("small m8 k8 x1", 3000, 1, 8, 17, 600, 8)]
    print("# WPE: ms per iteration, delay 3, max_flooring(1e-10); {} iterations + the output walk in one "
          "launch, divided by {}".format(STEPS, STEPS))
    for label, seed, B, M, F, T, taps in shapes:
        X = torch.from_numpy(nmf_mixture_batch(seed, B, M, F, T)).to(dev)
        shape_times(label, X, taps, 3)
        del X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
