#!/usr/bin/env python3
"""PDSBSS iterations against AuxLaplaceIVA-IP1 in the same process.

ms per update_once() of PDSBSS with l21 over bins (the IVA penalty) on the device operators, the same
iteration on the compatibility path (an equivalent user closure: Z to the host and Yt back), l1, two
penalties (l21 over bins + l1) and MaskingPDSBSS, with the AuxLaplaceIVA-IP1 yardstick beside them:
configs[1] (N=4, F=1025, T=512) with 1, 32 and 128 mixtures and configs[2] (N=8, F=2049, T=1024) with
32.  Medians of three 20-iteration regions after a warm-up, the methods of a
shape alternating.  For the device forms the achieved share of the HBM peak is printed from the
algorithmic bytes of the passes as written ("PDSBSS").

    python benchmarks/pdsbss.py [--small]      # --small: a rehearsal at toy sizes
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
from ssspy_amd.bss.iva import AuxLaplaceIVA  # noqa: E402
from ssspy_amd.bss.pdsbss import PDSBSS, MaskingPDSBSS  # noqa: E402
from ssspy_amd.linalg import prox  # noqa: E402
from ssspy_amd.utils.dataset import nmf_mixture_batch  # noqa: E402

REGIONS, REGION_ITERS, WARMUP = 3, 20, 3
HBM_PEAK = 8.0e12  # bytes / s
l21_bins = functools.partial(prox.l21, axis2=1)


def closure_l21_bins(z, step_size=1):
    return prox.l21(z, step_size=step_size, axis2=1)


def soft_mask(z):
    norm = np.linalg.norm(z, axis=1, keepdims=True)
    return np.maximum(1 - 0.5 / np.maximum(norm, 1e-12), 0)


# (name, constructor, spectrogram-sized streams of 16 bytes per iteration as the passes are written:
# the contraction reads Q + 1, the norm pass 2, a dual step reads 2 and writes 1; None: host-bound)
FORMS = [
    ("PDSBSS l21-bins", lambda: PDSBSS(prox_penalty=l21_bins, scale_restoration=False), 2 + 2 + 3),
    ("PDSBSS l1", lambda: PDSBSS(prox_penalty=prox.l1, scale_restoration=False), 2 + 3),
    ("PDSBSS l21-bins + l1", lambda: PDSBSS(prox_penalty=[l21_bins, prox.l1],
                                            scale_restoration=False), 3 + 2 + 3 + 3),
    ("PDSBSS closure l21-bins", lambda: PDSBSS(prox_penalty=closure_l21_bins,
                                               scale_restoration=False), None),
    ("MaskingPDSBSS", lambda: MaskingPDSBSS(mask_fn=soft_mask, scale_restoration=False), None),
]
YARDSTICK = ("AuxLaplaceIVA-IP1", lambda: AuxLaplaceIVA(spatial_algorithm="IP",
                                                        scale_restoration=False, record_loss=False))


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


def iteration_times(X, label, host_forms):
    B, N, F, T = X.shape
    entries = [(YARDSTICK[0], prepared(YARDSTICK[1], X, WARMUP), None, REGION_ITERS)]
    for name, make, streams in FORMS:
        if streams is None and not host_forms:
            continue
        # (the host-bound forms: two iterations per region, one warm-up)
        entries.append((name, prepared(make, X, WARMUP if streams else 1), streams,
                        REGION_ITERS if streams else 2))
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
            share = "  {:.0f} MB / mixture, {:.2f} of the HBM peak".format(
                nbytes / B / 1e6, nbytes / (med * 1e-3) / HBM_PEAK)
        print("{:22s} {:26s} {:9.4f} ms / iteration  (x{:.3f} of the yardstick; regions {}){}"
              .format(label, name, med, med / base, " ".join("{:.4f}".format(t) for t in v), share),
              flush=True)


def main():
    small = "--small" in sys.argv
    shapes = [(1, 4, 1025, 512), (32, 4, 1025, 512), (128, 4, 1025, 512), (32, 8, 2049, 1024)]
    if small:
        shapes = [(2, 4, 33, 64), (2, 8, 17, 64)]
    for B, N, F, T in shapes:
        X = torch.from_numpy(nmf_mixture_batch(7, B, N, F, T)).cuda()
        X = X / (X.abs().max() * (N * T) ** 0.5)  # (the scale normalize_by_spectral_norm leaves)
        label = "B={} N={} F={} T={}".format(B, N, F, T)
        iteration_times(X, label, host_forms=B <= 32 and N <= 4)
        del X
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
