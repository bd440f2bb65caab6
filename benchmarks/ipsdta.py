#!/usr/bin/env python3
"""GaussIPSDTA and TIPSDTA against GaussILRMA-IP1 on the same mixtures, in the same process.

ms per update_once() at 8 and 32 mixtures of N = 4, T = 512, K = 16: F = 1025 with n_blocks = 256
(blocks of 4, one of 5) and F = 1024 with n_blocks = 128 (blocks of 8; at F = 1025 the last block
would have 9 bins, past the device limit).  Medians of five regions of three iterations after a
warm-up, the methods of a shape alternating.  Beside every time: the fp64 flops and HBM bytes the
algorithm asks for per iteration ("IPSDTA") as a fraction of 78.6 TFLOP/s and 8 TB/s.
With --numpy: the NumPy restatement's time per iteration on this host's CPU at one mixture of the
first shape.

    python benchmarks/ipsdta.py [--small] [--numpy] [--out profiles/ipsdta_times.txt]
"""
import gc
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssspy_amd.bss.ilrma import GaussILRMA  # noqa: E402
from ssspy_amd.bss.ipsdta import TIPSDTA, GaussIPSDTA  # noqa: E402
from ssspy_amd.utils.dataset import nmf_mixture_batch  # noqa: E402

REGIONS, WARMUP, ITERS = 5, 2, 3
PEAK_FLOPS, PEAK_BYTES = 78.6e12, 8.0e12


def algorithmic_cost(B, N, F, T, K, n_blocks, t_model):
    """(fp64 flops, HBM bytes) of one iteration as DESIGN.md counts them: per (mixture, source,
    block, frame) and pass 8 N L for y, 8 K L^2 for R (complex basis, real weight), 8/3 L^3 + 8 L^3 for
    the two factorisations and the inverse, 8 L^2 for u; the basis pass adds 4 K L^2 (P, Q packed),
    the activation pass 16 K L^2, the covariance pass 8 L^2 N^2; the t model runs a quadratic-form
    pass in front of each.  Bytes: X once per pass and source group (the N sources of a block share
    it through L2), the activation terms written and read once, the covariance record."""
    L = F / n_blocks
    frames = B * N * n_blocks * T
    common = 8 * N * L + 8 * K * L * L + (8.0 / 3 + 8) * L ** 3 + 8 * L * L
    flops = frames * (3 * common + 4 * K * L * L + 16 * K * L * L + 8 * L * L * N * N)
    passes = 3
    if t_model:
        flops += frames * 3 * common
        passes = 6
    x_bytes = 16.0 * B * N * F * T
    act_bytes = 2 * 2 * 8.0 * B * N * K * n_blocks * T
    quad_bytes = (2 * 2 * 8.0 * B * N * n_blocks * T) * (3 if t_model else 0)
    cov_bytes = 16.0 * B * F * L * N * N * N
    return flops, passes * x_bytes + act_bytes + quad_bytes + 2 * cov_bytes


def prepared(make, X):
    m = make()
    m._bind_input(X)
    m._reset()
    for _ in range(WARMUP):
        m.update_once()
    return m


def region(m):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        m.update_once()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / ITERS


def main():
    small = "--small" in sys.argv
    out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    dev = torch.device("cuda", 0)
    shapes = [(B, 4, F, 512, 16, nb) for F, nb in ((1025, 256), (1024, 128)) for B in (8, 32)]
    if small:
        shapes = [(2, 4, 33, 64, 4, 8), (2, 4, 32, 64, 4, 4)]
    for B, N, F, T, K, nb in shapes:
        label = "B={} N={} F={} T={} K={} n_blocks={}".format(B, N, F, T, K, nb)
        X = torch.from_numpy(nmf_mixture_batch(1000, B, N, F, T)).to(dev)
        methods = [
            ("GaussILRMA-IP1", None,
             lambda: GaussILRMA(n_basis=K, spatial_algorithm="IP", record_loss=False,
                                rng=np.random.default_rng(0))),
            ("GaussIPSDTA", False,
             lambda: GaussIPSDTA(K, nb, record_loss=False, rng=np.random.default_rng(0))),
            ("TIPSDTA", True,
             lambda: TIPSDTA(K, nb, dof=100, record_loss=False, rng=np.random.default_rng(0))),
        ]
        live = [(name, t_model, prepared(make, X)) for name, t_model, make in methods]
        gc.collect()
        ms = {name: [] for name, _, _ in live}
        for _ in range(REGIONS):
            for name, _, m in live:
                ms[name].append(region(m))
        base = statistics.median(ms["GaussILRMA-IP1"])
        for name, t_model, _ in live:
            med = statistics.median(ms[name])
            line = "{:46s} {:15s} {:10.3f} ms / iteration  (x{:.1f} of ILRMA-IP1; regions {})".format(
                label, name, med, med / base, " ".join("{:.3f}".format(v) for v in ms[name]))
            if t_model is not None:
                flops, nbytes = algorithmic_cost(B, N, F, T, K, nb, t_model)
                line += "  fp64 {:.1f} % of peak, HBM {:.1f} % of peak".format(
                    100 * flops / (med * 1e-3) / PEAK_FLOPS, 100 * nbytes / (med * 1e-3) / PEAK_BYTES)
            emit(line)
        del live, X
        torch.cuda.empty_cache()
    if "--numpy" in sys.argv:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                        "tests"))
        import ipsdta_numpy as rn

        B, N, F, T, K, nb = shapes[0]
        X = nmf_mixture_batch(1000, 1, N, F, T)[0]
        m = rn.IPSDTA(K, nb, rng=np.random.default_rng(0))
        m.reset(X)
        t0 = time.perf_counter()
        m.update_once()
        emit("NumPy restatement, GaussIPSDTA, one mixture of N={} F={} T={} K={} n_blocks={}: "
             "{:.2f} s / iteration on the host CPU".format(N, F, T, K, nb, time.perf_counter() - t0))


if __name__ == "__main__":
    main()
