#!/usr/bin/env python3
"""FDICA on both routes against AuxLaplaceIVA-IP1 in the same process.

ms per update_once() of GradLaplaceFDICA, NaturalGradLaplaceFDICA and AuxLaplaceFDICA-IP1 on (a) the
route ssspy_fdica_route picks (one ssspy_fdica_steps launch per iteration: resident or streaming)
and (b) the composed route (separate -> weight -> covariance -> step), with AuxLaplaceFDICA-IP2
(composed only) and the AuxLaplaceIVA-IP1 yardstick beside them, at configs[1] (N=4, F=1025, T=512)
with 1, 32 and 128 mixtures and at N=8, F=2049, T=1024 with 1 and 32: medians of three 20-iteration
regions after a warm-up, the methods of a shape alternating.  Then the
n_iter-iteration ``__call__`` with record_loss=True of the three kernel classes on either route (one
launch for all iterations on the kernel route).

    python benchmarks/fdica.py [--small | --classes]
    # --small: a rehearsal at toy sizes; --classes: iteration times of the shape classes the route
    # function tells apart (streaming at 2 and 4 sources, resident at 8 sources)
"""
import gc
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssspy_amd import _lib, _ops, _routes  # noqa: E402
from ssspy_amd.bss.fdica import (  # noqa: E402
    AuxLaplaceFDICA, GradLaplaceFDICA, NaturalGradLaplaceFDICA)
from ssspy_amd.bss.iva import AuxLaplaceIVA  # noqa: E402
from ssspy_amd.utils.dataset import nmf_mixture_batch  # noqa: E402

PLAIN = dict(permutation_alignment=False, scale_restoration=False)
FDICA = [
    ("GradLaplaceFDICA", lambda **kw: GradLaplaceFDICA(**PLAIN, **kw)),
    ("NaturalGradLaplaceFDICA", lambda **kw: NaturalGradLaplaceFDICA(**PLAIN, **kw)),
    ("AuxLaplaceFDICA-IP1", lambda **kw: AuxLaplaceFDICA(spatial_algorithm="IP1", **PLAIN, **kw)),
]
IP2 = ("AuxLaplaceFDICA-IP2", lambda **kw: AuxLaplaceFDICA(spatial_algorithm="IP2", **PLAIN, **kw))
YARDSTICK = ("AuxLaplaceIVA-IP1", lambda **kw: AuxLaplaceIVA(spatial_algorithm="IP",
                                                            scale_restoration=False, **kw))
REGIONS, REGION_ITERS, WARMUP = 3, 20, 5
ROUTE_NAMES = {_lib.FDICA_ROUTE_RESIDENT: "resident", _lib.FDICA_ROUTE_STREAMING: "streaming",
               _lib.FDICA_ROUTE_COMPOSED: "composed"}


def prepared(make, X, kernel):
    with _routes.override(fdica_kernel=kernel):
        m = make(record_loss=False)
        m._bind_input(X)
        m._reset()
        for _ in range(WARMUP):
            m.update_once()
    return m


def region(m, kernel):
    with _routes.override(fdica_kernel=kernel):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REGION_ITERS):
            m.update_once()
        torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / REGION_ITERS


def iteration_times(X, label, route):
    entries = [(YARDSTICK[0], "-", prepared(YARDSTICK[1], X, True), True)]
    for name, make in FDICA:
        entries.append((name, route, prepared(make, X, True), True))
        entries.append((name, "composed", prepared(make, X, False), False))
    entries.append((IP2[0], "composed", prepared(IP2[1], X, False), False))
    ms = [[] for _ in entries]
    gc.collect()
    for _ in range(REGIONS):
        for k, (_, _, m, kernel) in enumerate(entries):  # (alternating: drift hits every method alike)
            ms[k].append(region(m, kernel))
    base = statistics.median(ms[0])
    for (name, how, _, _), v in zip(entries, ms):
        med = statistics.median(v)
        print("{:22s} {:24s} {:10s} {:9.4f} ms / iteration  (x{:.3f} of the yardstick; regions {})"
              .format(label, name, how, med, med / base, " ".join("{:.4f}".format(t) for t in v)),
              flush=True)


def call_times(X, label, route, n_iter):
    for name, make in FDICA:
        for how, kernel in ((route, True), ("composed", False)):
            with _routes.override(fdica_kernel=kernel):
                make(record_loss=True).call_on_device(X, n_iter=2)  # (untimed: first-use allocations)
                times = []
                for _ in range(3):
                    m = make(record_loss=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    m.call_on_device(X, n_iter=n_iter)
                    torch.cuda.synchronize()
                    times.append(1e3 * (time.perf_counter() - t0))
            print("{:22s} {:24s} {:10s} {:9.2f} ms / {}-iteration __call__, record_loss=True "
                  "(runs {})".format(label, name, how, statistics.median(times), n_iter,
                                     " ".join("{:.2f}".format(v) for v in times)), flush=True)


def main():
    small = "--small" in sys.argv
    dev = torch.device("cuda", 0)
    shapes = [("configs[1] x1", 1000, 1, 4, 1025, 512), ("configs[1] x32", 1000, 32, 4, 1025, 512),
              ("configs[1] x128", 1000, 128, 4, 1025, 512), ("n8 f2049 t1024 x1", 3000, 1, 8, 2049, 1024),
              ("n8 f2049 t1024 x32", 3000, 32, 8, 2049, 1024)]
    if small:
        shapes = [("small x4", 1000, 4, 4, 33, 64), ("small8 x2", 3000, 2, 8, 17, 600)]
    classes = "--classes" in sys.argv
    if classes:
        shapes = [("n2 f1025 t2100 x32", 1000, 32, 2, 1025, 2100), ("n4 f1025 t1024 x1", 1000, 1, 4, 1025, 1024),
                  ("n4 f1025 t1024 x32", 1000, 32, 4, 1025, 1024), ("n8 f2049 t384 x1", 3000, 1, 8, 2049, 384),
                  ("n8 f2049 t384 x32", 3000, 32, 8, 2049, 384), ("n6 f1025 t512 x32", 3000, 32, 6, 1025, 512)]
    for label, seed, B, N, F, T in shapes:
        X = torch.from_numpy(nmf_mixture_batch(seed, B, N, F, T)).to(dev)
        route = ROUTE_NAMES[_ops.fdica_route(B, N, F, T, _lib.FDICA_AUX_IP1)]
        iteration_times(X, label, route)
        if not classes:
            call_times(X, label, route, 20 if B * N * F * T > 1 << 27 else 100)
        del X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
