#!/usr/bin/env python3
"""FastIVA and FasterIVA against AuxLaplaceIVA-IP1 in the same process.

ms per update_once() with Laplace closures (G = 2 r) at 128 mixtures of configs[1] (N=4, F=1025,
T=512) and at 32 mixtures of configs[2] (N=8, F=2049, T=1024): medians of three regions after a
warm-up, the methods of a shape alternating.  With record_loss=False a region is 10 calls of
update_once(); with record_loss=True it is one round of update_once() + compute_loss(), because the
loss of the two fixed-point classes takes the whole estimate to the host for the user's contrast_fn
(4.3 GB per round at either shape) where AuxLaplaceIVA's stays on the device.  The fixed-point
classes also take the frame norms to the host once per iteration for d_contrast_fn / dd_contrast_fn.

    python benchmarks/fast_iva.py [--small] [--out profiles/fast_iva_times.txt]
"""
import gc
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssspy_amd.bss.iva import AuxLaplaceIVA, FasterIVA, FastIVA  # noqa: E402
from ssspy_amd.utils.dataset import nmf_mixture_batch  # noqa: E402


def contrast_fn(y):
    return 2 * np.linalg.norm(y, axis=1)


def d_contrast_fn(r):
    return 2 * np.ones_like(r)


def dd_contrast_fn(r):
    return np.zeros_like(r)


METHODS = [
    ("AuxLaplaceIVA-IP1", lambda **kw: AuxLaplaceIVA(spatial_algorithm="IP", **kw)),
    ("FastIVA", lambda **kw: FastIVA(contrast_fn=contrast_fn, d_contrast_fn=d_contrast_fn,
                                     dd_contrast_fn=dd_contrast_fn, **kw)),
    ("FasterIVA", lambda **kw: FasterIVA(contrast_fn=contrast_fn, d_contrast_fn=d_contrast_fn,
                                         **kw)),
]
REGIONS, WARMUP = 3, 3
ITERS = {False: 10, True: 1}


def prepared(make, X, record_loss):
    m = make(record_loss=record_loss)
    m._bind_input(X)
    m._reset()
    for _ in range(WARMUP):
        m.update_once()
    return m


def region(m, record_loss):
    n = ITERS[record_loss]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        m.update_once()
        if record_loss:
            m.compute_loss()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def iteration_times(X, label, record_loss, emit):
    ms = {name: [] for name, _ in METHODS}
    methods = [(name, prepared(make, X, record_loss)) for name, make in METHODS]
    gc.collect()
    for _ in range(REGIONS):
        for name, m in methods:  # (alternating: a drift of the clocks hits every method alike)
            ms[name].append(region(m, record_loss))
    base = statistics.median(ms[METHODS[0][0]])
    for name, _ in METHODS:
        med = statistics.median(ms[name])
        emit("{:18s} record_loss={:5s} {:18s} {:10.4f} ms / iteration  (x{:.3f} of the yardstick; "
             "regions {})".format(label, str(record_loss), name, med, med / base,
                                  " ".join("{:.4f}".format(v) for v in ms[name])))


def main():
    small = "--small" in sys.argv
    out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    dev = torch.device("cuda", 0)
    shapes = [("configs[1] x128", 1000, 128, 4, 1025, 512), ("configs[2] x32", 3000, 32, 8, 2049, 1024)]
    if small:
        shapes = [("small x4", 1000, 4, 4, 33, 64), ("small8 x2", 3000, 2, 8, 17, 64)]
    for label, seed, B, N, F, T in shapes:
        X = torch.from_numpy(nmf_mixture_batch(seed, B, N, F, T)).to(dev)
        for record_loss in (False, True):
            iteration_times(X, label, record_loss, emit)
        del X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
