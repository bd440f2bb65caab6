#!/usr/bin/env python3
"""ConvILRMA iterations beside their comparisons in the same process.

ms per ConvGaussILRMA iteration (the two on-Y NMF updates, ssspy_conviva_statistics_nmf, the IP1
sweep, ssspy_conviva_compose, the output walk and the power normalisation; no loss) at M=4, taps=10
(Lb=44, slab resident) and at M=8, taps=7 (Lb=64, slab re-read), n_basis=16, at 1 and 32 mixtures of
F=1025, T=512, delay=3, beside
  (a) one ConvGaussIVA iteration of the same shape (frame powers, weights, ssspy_conviva_statistics,
      sweep, composition, output walk) and the two on-Y NMF updates alone: the expectation to confirm
      or refute is "ConvILRMA = (a) + the two NMF passes",
  (b) one GaussILRMA-IP1 iteration (ssspy_ilrma_ip1_update, normalisation included),
  (c) one WPE iteration of the same taps plus (b): the cascade ConvILRMA replaces, and
  (d) what forming the weights in the kernel is worth, by the cheapest stand-in: the statistics
      kernel alone with the weights formed in the kernel against the frame-weight kernel alone on the
      same shape (what the in-kernel sum and division cost), and ssspy_ilrma_iss_weight alone (the
      launch and the (B, N, F, T) write a precomputed array would add; its read inside the statistics
      kernel would come on top and is not measured: no kernel reads a per-bin weight array).
Medians of three regions after a warm-up, the methods of a shape alternating; every region ends in a
device synchronise.

    python benchmarks/convilrma.py [--small] > profiles/convilrma.txt
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
DELAY, DOMAIN, N_BASIS = 3, 2.0, 16
ROUTE_NAMES = {_lib.CONVIVA_ROUTE_RESIDENT: "resident", _lib.CONVIVA_ROUTE_STREAMING: "streaming"}


def timed(fn, per):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / per


def shape_times(label, X, taps):
    B, M, F, T = X.shape
    Lb = (taps + 1) * M
    dev = X.device
    route, lds = _ops.conviva_route(B, M, F, T, taps)
    info = dv.zeros((2,), dv.i32, dev)
    gen = torch.Generator(device="cpu").manual_seed(11)
    basis0 = torch.rand((B, M, F, N_BASIS), generator=gen, dtype=torch.float64).clamp(min=1e-10).to(dev)
    act0 = torch.rand((B, M, N_BASIS, T), generator=gen, dtype=torch.float64).clamp(min=1e-10).to(dev)
    basis, act = basis0.clone(), act0.clone()
    W = dv.zeros((B, F, M, Lb), dv.c128, dev)
    Y = dv.empty((B, M, F, T), dv.c128, dev)
    Sigma = dv.zeros((B, F, M, M, M), dv.c128, dev)
    G = dv.zeros((B, F, M, taps * M, M), dv.c128, dev)
    failed = dv.zeros((B, F, M), dv.i32, dev)
    variance = dv.zeros((B, M, T), dv.f64, dev)
    ws, ws_bytes = _ops.ilrma_workspace(B, M, F, T, N_BASIS, dev)
    Wi = dv.eye_filters(B, F, M, dev)
    C = _ops.weighted_covariance(X).reshape(B, F, M, M)
    U = dv.empty((B, F, M, M, M), dv.c128, dev)
    Gw = dv.zeros((B, F, taps * M, M), dv.c128, dev)
    Yw = dv.empty((B, M, F, T), dv.c128, dev)
    phi_frame = (torch.rand((B, M, T), generator=gen, dtype=torch.float64) + 0.5).to(dev)
    varphi = dv.empty((B, M, F, T), dv.f64, dev)

    def start():
        W.zero_()
        W[..., :M] = dv.eye_filters(B, F, M, dev)
        _ops.wpd_apply(X, W, taps, DELAY, Y=Y)
        basis.copy_(basis0)
        act.copy_(act0)

    def nmf_updates():
        _ops.ilrma_update_basis(Y, None, basis, act, DOMAIN, FLOOR, ws, ws_bytes)
        _ops.ilrma_update_activation(Y, None, basis, act, DOMAIN, FLOOR, ws, ws_bytes)

    def tail():
        Q = W[..., :M].clone()
        _ops.update_by_ip1(Q, Sigma, FLOOR, info)
        _ops.conviva_compose(Q, G, W, taps, failed)
        _ops.wpd_apply(X, W, taps, DELAY, Y=Y)

    def convilrma_step():
        nmf_updates()
        _ops.conviva_statistics_nmf(X, basis, act, DOMAIN, taps, DELAY, 0.0, info, Sigma=Sigma, G=G,
                                    failed=failed)
        tail()
        _ops.convilrma_normalize(Y, W, basis, taps, DOMAIN, FLOOR)

    def convilrma():
        start()
        for _ in range(STEPS):
            convilrma_step()

    def conviva():
        start()
        for _ in range(STEPS):
            r2 = _ops.iva_frame_power(Y, None)
            phi = _ops.iva_weight(r2, F, _lib.CONTRAST_GAUSS, FLOOR, variance=variance)
            _ops.conviva_statistics(X, phi, taps, DELAY, 0.0, info, Sigma=Sigma, G=G, failed=failed)
            tail()

    def nmf_alone():
        start()
        for _ in range(STEPS):
            nmf_updates()

    def ilrma():
        Wi.copy_(dv.eye_filters(B, F, M, dev))
        basis.copy_(basis0)
        act.copy_(act0)
        for _ in range(STEPS):
            _ops.ilrma_ip1_update(X, C, Wi, basis, act, U, DOMAIN, True, FLOOR, ws, ws_bytes, info)

    def cascade():
        Gw.zero_()
        _ops.wpe_steps(X, Gw, taps, DELAY, FLOOR, STEPS, info, Y=Yw)
        ilrma()

    def statistics_nmf():
        for _ in range(STEPS):
            _ops.conviva_statistics_nmf(X, basis0, act0, DOMAIN, taps, DELAY, 0.0, info, Sigma=Sigma,
                                        G=G, failed=failed)

    def statistics_frame():
        for _ in range(STEPS):
            _ops.conviva_statistics(X, phi_frame, taps, DELAY, 0.0, info, Sigma=Sigma, G=G,
                                    failed=failed)

    def iss_weight():
        for _ in range(STEPS):
            _ops.ilrma_iss_weight(basis0, act0, DOMAIN, out=varphi)

    entries = [("ConvILRMA (" + ROUTE_NAMES[route] + ")", convilrma),
               ("(a) ConvGaussIVA", conviva), ("(a) two on-Y NMF updates", nmf_alone),
               ("(b) GaussILRMA-IP1", ilrma), ("(c) WPE + GaussILRMA-IP1", cascade),
               ("(d) statistics, NMF weights", statistics_nmf),
               ("(d) statistics, frame weights", statistics_frame),
               ("(d) ilrma_iss_weight alone", iss_weight)]
    for _, fn in entries:
        fn()  # warm-up: first-use allocations, code loading
    ms = [[] for _ in entries]
    for _ in range(REGIONS):
        for k, (_, fn) in enumerate(entries):
            ms[k].append(timed(fn, STEPS))
    med = [statistics.median(v) for v in ms]
    for (name, _), m, v in zip(entries, med, ms):
        print("{:24s} {:30s} {:10.4f} ms / iteration  (regions {})".format(
            label, name, m, " ".join("{:.4f}".format(t) for t in v)), flush=True)
    print("{:24s} ConvILRMA is x{:.3f} of (a) ConvGaussIVA + the two NMF updates, x{:.3f} of (a) alone, "
          "x{:.3f} of (b), x{:.3f} of (c); forming the weights in the kernel costs {:+.4f} ms over the "
          "frame-weight kernel, a precomputed array at least {:.4f} ms (its write alone)".format(
              label, med[0] / (med[1] + med[2]), med[0] / med[1], med[0] / med[3], med[0] / med[4],
              med[5] - med[6], med[7]), flush=True)
    print("{:24s} LDS {} bytes / workgroup; failed triples {}".format(
        label, lds + 8 * N_BASIS, int(info[0].item())), flush=True)


def main():
    dev = torch.device("cuda", 0)
    shapes = []
    for M, taps, seed in ((4, 10, 1000), (8, 7, 3000)):
        for B in (1, 32):
            shapes.append(("m{} k{} f1025 t512 x{}".format(M, taps, B), seed, B, M, 1025, 512, taps))
    if "--small" in sys.argv:
        shapes = [("small m4 k10 x2", 1000, 2, 4, 33, 128, 10), ("small m8 k7 x1", 3000, 1, 8, 17, 600, 7)]
    print("# ConvGaussILRMA: ms per iteration, n_basis {}, domain {}, delay {}, max_flooring(1e-10), "
          "diagonal_loading 0, power normalisation; {} iterations per region, divided by {}".format(
              N_BASIS, DOMAIN, DELAY, STEPS, STEPS))
    for label, seed, B, M, F, T, taps in shapes:
        X = torch.from_numpy(nmf_mixture_batch(seed, B, M, F, T)).to(dev)
        shape_times(label, X, taps)
        del X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
