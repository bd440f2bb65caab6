#!/usr/bin/env python3
"""CACGMM against AuxLaplaceIVA-IP1 in the same process.

ms per update_once() of CACGMM and of the AuxLaplaceIVA-IP1 yardstick on the same mixtures: 1, 32
and 128 mixtures of the configs[1] bins (M = N = 4, F = 1025, T = 512), then N = 2 and N = 8 sources
on the 4 channels at 32 mixtures.  Medians of three 20-iteration regions after a warm-up, the two
methods alternating.  AuxLaplaceIVA-IP1 is the comparison because its iteration has the same
ingredients: one pass over the mixture, one weighted covariance, one per-bin solve.

    python benchmarks/cacgmm.py [--small] [--profile]
    --small: a rehearsal at toy sizes;  --profile: only 20 iterations of each method at 128 mixtures
    (the run to put under rocprofv3 --kernel-trace --stats)
"""
import gc
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssspy_amd.bss.cacgmm import CACGMM  # noqa: E402
from ssspy_amd.bss.iva import AuxLaplaceIVA  # noqa: E402
from ssspy_amd.utils.dataset import nmf_mixture_batch  # noqa: E402

REGIONS, REGION_ITERS, WARMUP = 3, 20, 5


def prepared_cacgmm(X, n_sources):
    m = CACGMM(n_sources=n_sources, record_loss=False, permutation_alignment=False,
               rng=np.random.default_rng(0))
    m._bind_input(X)
    m._reset(flooring_fn=m.flooring_fn)
    return m


def prepared_auxiva(X):
    m = AuxLaplaceIVA(spatial_algorithm="IP", record_loss=False)
    m._bind_input(X)
    m._reset()
    return m


def region(m, iters=REGION_ITERS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        m.update_once()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def compare(X, label, n_sources):
    methods = [("AuxLaplaceIVA-IP1", prepared_auxiva(X)),
               ("CACGMM N={}".format(n_sources), prepared_cacgmm(X, n_sources))]
    for _, m in methods:
        for _ in range(WARMUP):
            m.update_once()
    gc.collect()
    ms = {name: [] for name, _ in methods}
    for _ in range(REGIONS):
        for name, m in methods:  # (alternating: a drift of the clocks hits both alike)
            ms[name].append(region(m))
    base = statistics.median(ms[methods[0][0]])
    for name, _ in methods:
        med = statistics.median(ms[name])
        print("{:24s} {:20s} {:9.4f} ms / iteration  (x{:.3f} of the yardstick; regions {})".format(
            label, name, med, med / base, " ".join("{:.4f}".format(v) for v in ms[name])), flush=True)


def main():
    small, profile = "--small" in sys.argv, "--profile" in sys.argv
    dev = torch.device("cuda", 0)
    M, F, T = (4, 33, 64) if small else (4, 1025, 512)
    shapes = [(1, 4), (32, 4), (128, 4), (32, 2), (32, 8)]
    if small:
        shapes = [(1, 4), (4, 4), (4, 2), (4, 8)]
    if profile:
        X = torch.from_numpy(nmf_mixture_batch(1000, 4 if small else 128, M, F, T)).to(dev)
        for m in (prepared_auxiva(X), prepared_cacgmm(X, 4)):
            region(m)
        return
    for B, N in shapes:
        X = torch.from_numpy(nmf_mixture_batch(1000, B, M, F, T)).to(dev)
        compare(X, "M=4 F={} T={} x{}".format(F, T, B), N)
        del X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
