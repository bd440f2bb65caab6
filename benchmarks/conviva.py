#!/usr/bin/env python3
"""ConvIVA iterations beside four comparisons in the same process.

ms per ConvLaplaceIVA iteration (frame powers, weights, ssspy_conviva_statistics, the IP1 sweep,
ssspy_conviva_compose and the output walk; no loss) at M=4, taps=10 (Lb=44) and at M=8, taps=7
(Lb=64), at 1 and 32 mixtures of F=1025, T=512, delay=3, beside
  (a) N = M WPD iterations of the same order on the same spectrograms (ssspy_wpd_steps with M
      masks): the operation-count expectation, the walks and the factorisations being the same size,
  (b) one AuxLaplaceIVA-IP1 iteration (frame powers, weights, covariances, sweep),
  (c) one WPE iteration of the same taps plus (b): the cascade ConvIVA replaces, and
  (d) the same ConvIVA iteration written as a chain of torch operators (unfold, einsum,
      torch.linalg.cholesky, cholesky_solve, torch.linalg.solve) -- what a user would write today;
      it goes through the mixtures in chunks (its stacked vectors are taps + 1 times the input).
Medians of three regions after a warm-up, the methods of a shape alternating; every region ends in a
device synchronise.

    python benchmarks/conviva.py [--small] > profiles/conviva.txt
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
FLOOR = (_lib.FLOOR_MAX, 1e-10)
DELAY = 3
ROUTE_NAMES = {_lib.CONVIVA_ROUTE_RESIDENT: "resident", _lib.CONVIVA_ROUTE_STREAMING: "streaming"}


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


def torch_iteration(X, W, taps, delay):
    """One ConvLaplaceIVA iteration on X (B, M, F, T), W (B, F, M, Lb) with torch operators; returns
    the new W."""
    B, M, F, T = X.shape
    xb = stacked(X, taps, delay)
    Y = torch.einsum("bfnl,bftl->bnft", W, xb)
    r = torch.sqrt((Y.real ** 2 + Y.imag ** 2).sum(dim=2))           # (B, M, T)
    phi = 2.0 / torch.clamp(2.0 * r, min=FLOOR[1])
    Sigma, G = [], []
    for n in range(M):
        Rb = torch.einsum("bftl,bftn->bfln", xb * phi[:, n, None, :, None], xb.conj()) / T
        C, P, R = Rb[..., :M, :M], Rb[..., M:, :M], Rb[..., M:, M:]
        g = torch.cholesky_solve(P, torch.linalg.cholesky(R))
        G.append(g)
        Sigma.append(C - P.mH @ g)
    Q = W[..., :M].clone()
    eye = torch.eye(M, dtype=X.dtype, device=X.device)
    rows = []
    for n in range(M):
        w = torch.linalg.solve(Q @ Sigma[n], eye[n].expand(B, F, M))
        d = torch.sqrt(torch.einsum("bfi,bfij,bfj->bf", w.conj(), Sigma[n], w).real.clamp(min=0))
        Q[:, :, n, :] = w.conj() / torch.clamp(d, min=FLOOR[1])[..., None]
        tail = -torch.einsum("bflm,bfm->bfl", G[n].conj(), Q[:, :, n, :])
        rows.append(torch.cat([Q[:, :, n, :], tail], dim=-1))
    return torch.stack(rows, dim=2)


def shape_times(label, X, taps, chunk):
    B, M, F, T = X.shape
    Lb = (taps + 1) * M
    dev = X.device
    route, lds = _ops.conviva_route(B, M, F, T, taps)
    info = dv.zeros((2,), dv.i32, dev)
    W = dv.zeros((B, F, M, Lb), dv.c128, dev)
    Y = dv.empty((B, M, F, T), dv.c128, dev)
    Sigma = dv.zeros((B, F, M, M, M), dv.c128, dev)
    G = dv.zeros((B, F, M, taps * M, M), dv.c128, dev)
    failed = dv.zeros((B, F, M), dv.i32, dev)
    Wd = dv.zeros((B, F, M, Lb), dv.c128, dev)
    Yd = dv.empty((B, M, F, T), dv.c128, dev)
    gen = torch.Generator(device="cpu").manual_seed(7)
    mask = torch.rand((B, M, F, T), generator=gen, dtype=torch.float64) * 0.95 + 0.05
    mask = (mask / mask.sum(dim=1, keepdim=True)).to(dev)
    Wi = dv.eye_filters(B, F, M, dev)
    Gw = dv.zeros((B, F, taps * M, M), dv.c128, dev)
    Yw = dv.empty((B, M, F, T), dv.c128, dev)

    def start():
        W.zero_()
        W[..., :M] = dv.eye_filters(B, F, M, dev)
        _ops.wpd_apply(X, W, taps, DELAY, Y=Y)

    def conviva_step():
        r2 = _ops.iva_frame_power(Y, None)
        phi = _ops.iva_weight(r2, F, _lib.CONTRAST_LAPLACE, FLOOR)
        _ops.conviva_statistics(X, phi, taps, DELAY, 0.0, info, Sigma=Sigma, G=G, failed=failed)
        Q = W[..., :M].clone()
        _ops.update_by_ip1(Q, Sigma, FLOOR, info)
        _ops.conviva_compose(Q, G, W, taps, failed)
        _ops.wpd_apply(X, W, taps, DELAY, Y=Y)

    def conviva():
        start()
        for _ in range(STEPS):
            conviva_step()

    def wpd():
        Wd.zero_()
        Wd[..., 0] = 1.0
        _ops.wpd_steps(X, mask, None, Wd, taps, DELAY, 0, 1e-6, (_lib.FLOOR_MAX, 1e-6), STEPS, info,
                       Y=Yd)

    def auxiva_step():
        r2 = _ops.iva_frame_power(X, Wi)
        weight = _ops.iva_weight(r2, F, _lib.CONTRAST_LAPLACE, FLOOR)
        U = _ops.weighted_covariance(X, weight, _lib.WEIGHT_FRAME, M)
        _ops.update_by_ip1(Wi, U, FLOOR, info)

    def auxiva():
        Wi.copy_(dv.eye_filters(B, F, M, dev))
        for _ in range(STEPS):
            auxiva_step()

    def cascade():
        Gw.zero_()
        _ops.wpe_steps(X, Gw, taps, DELAY, FLOOR, STEPS, info, Y=Yw)
        auxiva()

    Wt = [None]

    def chain():
        parts = []
        for b0 in range(0, B, chunk):
            Xc = X[b0:b0 + chunk]
            w = torch.zeros((Xc.shape[0], F, M, Lb), dtype=X.dtype, device=dev)
            w[..., :M] = torch.eye(M, dtype=X.dtype, device=dev)
            parts.append(torch_iteration(Xc, w, taps, DELAY))
        Wt[0] = torch.cat(parts)

    entries = [("ConvIVA (" + ROUTE_NAMES[route] + ")", conviva, STEPS),
               ("(a) N WPD iterations", wpd, STEPS), ("(b) AuxLaplaceIVA-IP1", auxiva, STEPS),
               ("(c) WPE + AuxIVA-IP1", cascade, STEPS), ("(d) ConvIVA torch operators", chain, 1)]
    for _, fn, _ in entries:
        fn()  # warm-up: first-use allocations, code loading
    ms = [[] for _ in entries]
    for _ in range(REGIONS):
        for k, (_, fn, per) in enumerate(entries):
            ms[k].append(timed(fn, per))
    # the two ConvIVA forms agree: one iteration of each from the start state
    start()
    conviva_step()
    agree = float((W - Wt[0]).abs().max())
    med = [statistics.median(v) for v in ms]
    for (name, _, _), m, v in zip(entries, med, ms):
        print("{:24s} {:28s} {:10.4f} ms / iteration  (x{:.3f} of (a), x{:.3f} of (a) + (b), x{:.3f} "
              "of (c), x{:.3f} of (d); regions {})".format(
                  label, name, m, m / med[1], m / (med[1] + med[2]), m / med[3], m / med[4],
                  " ".join("{:.4f}".format(t) for t in v)), flush=True)
    print("{:24s} LDS {} bytes / workgroup; failed triples {}; max |W kernel - W torch| after 1 "
          "iteration {:.2e}".format(label, lds, int(info[0].item()), agree), flush=True)


def main():
    dev = torch.device("cuda", 0)
    shapes = []
    for M, taps, seed, chunk in ((4, 10, 1000, 4), (8, 7, 3000, 2)):
        for B in (1, 32):
            shapes.append(("m{} k{} f1025 t512 x{}".format(M, taps, B), seed, B, M, 1025, 512, taps,
                           chunk))
    if "--small" in sys.argv:
        shapes = [("small m4 k10 x2", 1000, 2, 4, 33, 128, 10, 2),
                  ("small m8 k7 x1", 3000, 1, 8, 17, 600, 7, 1)]
    print("# ConvLaplaceIVA: ms per iteration, delay 3, max_flooring(1e-10), diagonal_loading 0; {} "
          "iterations per region, divided by {}".format(STEPS, STEPS))
    for label, seed, B, M, F, T, taps, chunk in shapes:
        X = torch.from_numpy(nmf_mixture_batch(seed, B, M, F, T)).to(dev)
        shape_times(label, X, taps, chunk)
        del X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
