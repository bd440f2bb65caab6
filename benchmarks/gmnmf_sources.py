#!/usr/bin/env python3
"""GaussMNMF per-iteration time at 8 and 16 sources: `batch` mixtures of F = 513, T = 256, K = 8 at
(M, N) = (2, 8), (2, 16), (4, 8), (4, 16), (8, 8), (8, 16); the 16-source row also gives its ratio to
the 8-source row of the same channel count.  3 warm-up iterations, then `iters` timed ones.

    python benchmarks/gmnmf_sources.py [batch] [iters] [M:N ...]
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssspy_amd.bss.mnmf import GaussMNMF  # noqa: E402
from ssspy_amd.utils.dataset import nmf_mixture  # noqa: E402

F, T, K = 513, 256, 8
SHAPES = [(2, 8), (2, 16), (4, 8), (4, 16), (8, 8), (8, 16)]


def run(B, M, N, iters):
    X = np.stack([nmf_mixture(4000 + b, M, F, T) for b in range(B)])
    m = GaussMNMF(n_basis=K, n_sources=N, record_loss=False, rng=np.random.default_rng(0))
    m._bind_input(X)
    m._reset()
    for _ in range(3):
        m.update_once()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        m.update_once()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


if __name__ == "__main__":
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    shapes = [tuple(int(v) for v in a.split(":")) for a in sys.argv[3:]] or SHAPES
    eight = {}
    for M, N in shapes:
        ms = run(B, M, N, iters)
        if N == 8:
            eight[M] = ms
        ratio = round(ms / eight[M], 2) if N > 8 and M in eight else None
        print(json.dumps({"channels": M, "sources": N, "batch": B, "F": F, "T": T, "K": K,
                          "iterations": iters, "ms_per_iter": round(ms, 3),
                          "vs_8_sources": ratio}), flush=True)
