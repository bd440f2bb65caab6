#!/usr/bin/env python3
"""ADMMIVA iterations against PDSBSS and AuxLaplaceIVA-IP1 in the same process.

ms per update_once() of ADMMIVA (ADMMBSS with l21 over bins on the device operators) beside PDSBSS
with the same penalty -- the yardstick -- and AuxLaplaceIVA-IP1: configs[1] (N=4, F=1025, T=512) with
1, 32 and 128 mixtures and configs[2] (N=8, F=2049, T=1024) with 32; at 1 and 32 mixtures of configs[1]
also the compatibility path (an equivalent user closure: Z to the host and the prox value back).
Medians of three 20-iteration regions after a warm-up, the methods of a shape
alternating.  For the device forms the achieved share of the HBM peak is printed from the algorithmic
bytes of the passes as written ("ADMMBSS").  The Gram inverse, once per call, is timed on
its own.  The mixtures are scaled to RMS 0.1 ("ADMMBSS": the scale condition).

    python benchmarks/admmbss.py [--small]      # --small: a rehearsal at toy sizes
"""
import functools
import gc
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssspy_amd import _ops  # noqa: E402
from ssspy_amd.bss.iva import ADMMIVA, AuxLaplaceIVA  # noqa: E402
from ssspy_amd.bss.pdsbss import PDSBSS  # noqa: E402
from ssspy_amd.linalg import prox  # noqa: E402
from ssspy_amd.utils.dataset import nmf_mixture_batch  # noqa: E402

REGIONS, REGION_ITERS, WARMUP = 3, 20, 3
HBM_PEAK = 8.0e12  # bytes / s
l21_bins = functools.partial(prox.l21, axis2=1)


def contrast(y):
    return np.linalg.norm(y, axis=1)


def closure_l21_bins(z, step_size=1):
    return prox.l21(z, step_size=step_size, axis2=1)


# (name, constructor, spectrogram-sized streams of 16 bytes per iteration as the passes are written;
# None: host-bound.  PDSBSS: the contraction reads 2, the norm pass 2, the dual step reads 2 and writes
# 1.  ADMMBSS with relaxation 1: the contraction reads 3, the norm pass 2, the auxiliary step reads 2
# and writes 2.)
FORMS = [
    ("PDSBSS l21-bins", lambda: PDSBSS(prox_penalty=l21_bins, scale_restoration=False), 7),
    ("ADMMIVA", lambda: ADMMIVA(scale_restoration=False, record_loss=False), 9),
    ("AuxLaplaceIVA-IP1", lambda: AuxLaplaceIVA(spatial_algorithm="IP", scale_restoration=False,
                                                record_loss=False), 0),
    ("ADMMIVA closure", lambda: ADMMIVA(contrast_fn=contrast, prox_penalty=closure_l21_bins,
                                        scale_restoration=False, record_loss=False), None),
]


def prepared(make, X, warmup):
    m = make()
    m._bind_input(X)
    m._reset()
    for _ in range(warmup):
        m.update_once()
    return m


def region(m, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        m.update_once()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def gram_inverse_time(X):
    out = _ops.admmbss_gram_inverse(X, 1)
    times = []
    for _ in range(REGIONS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _ops.admmbss_gram_inverse(X, 1, out=out)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def iteration_times(X, label, host_forms):
    B, N, F, T = X.shape
    entries = []
    for name, make, streams in FORMS:
        if streams is None and not host_forms:
            continue
        # (the host-bound form: two iterations per region, one warm-up)
        host = streams is None
        entries.append((name, prepared(make, X, 1 if host else WARMUP), streams,
                        2 if host else REGION_ITERS))
    ms = [[] for _ in entries]
    gc.collect()
    for _ in range(REGIONS):
        for k, (_, m, _, iters) in enumerate(entries):  # (alternating: drift hits every method alike)
            ms[k].append(region(m, iters))
    base = statistics.median(ms[0])
    for (name, _, streams, _), v in zip(entries, ms):
        med = statistics.median(v)
        share = ""
        if streams:
            nbytes = streams * 16.0 * B * N * F * T
            share = "  {} streams, {:.0f} MB / mixture, {:.2f} of the HBM peak".format(
                streams, nbytes / B / 1e6, nbytes / (med * 1e-3) / HBM_PEAK)
        print("{:22s} {:20s} {:9.4f} ms / iteration  (x{:.3f} of PDSBSS; regions {}){}"
              .format(label, name, med, med / base, " ".join("{:.4f}".format(t) for t in v), share),
              flush=True)
    print("{:22s} {:20s} {:9.4f} ms once per call".format(label, "Gram inverse",
                                                          gram_inverse_time(X)), flush=True)


def main():
    small = "--small" in sys.argv
    shapes = [(1, 4, 1025, 512), (32, 4, 1025, 512), (128, 4, 1025, 512), (32, 8, 2049, 1024)]
    if small:
        shapes = [(2, 4, 33, 64), (2, 8, 17, 64)]
    for B, N, F, T in shapes:
        X = torch.from_numpy(nmf_mixture_batch(7, B, N, F, T)).cuda()
        X = X * (0.1 / X.abs().pow(2).mean().sqrt())  # RMS 0.1
        label = "B={} N={} F={} T={}".format(B, N, F, T)
        iteration_times(X, label, host_forms=B <= 32 and N <= 4)
        del X
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
