#!/usr/bin/env python3
"""MaskingPDSHVA iterations on the device route against the only way to run HVA without it.

ms per update_once() of MaskingPDSHVA (the cepstral pass on its automatic route, the FFT at these
sizes), the same with the direct O(F^2) sum forced (N=4 only), MaskingPDSBSS carrying the same mask as
a host closure (Z to the host and a complex128 mask back up every iteration) and PDSBSS with
``prox.l1``, the cheapest on-device penalty: configs[1] (N=4, F=1025, T=512) with 1, 32 and 128
mixtures and configs[2] (N=8, F=2049, T=1024) with one.  Medians of three regions after a warm-up
(DESIGN.md section 5), the methods of a shape alternating.  For the device forms the achieved share
of the HBM peak is printed from the algorithmic bytes of the passes as written ("HVA").

    python benchmarks/hva.py [--small]      # --small: a rehearsal at toy sizes
"""
import gc
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssspy_amd import _lib  # noqa: E402
from ssspy_amd.bss.hva import MaskingPDSHVA  # noqa: E402
from ssspy_amd.bss.pdsbss import PDSBSS, MaskingPDSBSS  # noqa: E402
from ssspy_amd.linalg import prox  # noqa: E402
from ssspy_amd.utils.dataset import nmf_mixture_batch  # noqa: E402

REGIONS, REGION_ITERS, WARMUP = 3, 20, 3
HBM_PEAK = 8.0e12  # bytes / s


def direct_route():
    m = MaskingPDSHVA(scale_restoration=False)
    m._transform_route = _lib.HVA_ROUTE_DIRECT
    return m


def host_closure():
    """The parent's route: the mask of a MaskingPDSHVA object, passed as any user closure."""
    mask_fn = MaskingPDSHVA().mask_fn
    return MaskingPDSBSS(mask_fn=lambda z: mask_fn(z), scale_restoration=False)


# (name, constructor, 16-byte spectrogram-sized streams per iteration as the passes are written: the
# contraction reads 2; l1's dual step reads 2 and writes 1; the cepstral pass reads 2 and writes half
# a stream (real), the masked dual step reads 2 1/2 and writes 1.  None: host-bound)
FORMS = [
    ("PDSBSS l1", lambda: PDSBSS(prox_penalty=prox.l1, scale_restoration=False), 5.0),
    ("MaskingPDSHVA", lambda: MaskingPDSHVA(scale_restoration=False), 8.0),
    ("MaskingPDSHVA direct sum", direct_route, 8.0),
    ("MaskingPDSBSS host closure", host_closure, None),
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


def iteration_times(X, label, skip):
    B, N, F, T = X.shape
    entries = []
    for name, make, streams in FORMS:
        if name in skip:
            continue
        slow = streams is None or "direct" in name
        # (the host-bound form and the direct sum: two iterations per region, one warm-up)
        entries.append((name, prepared(make, X, 1 if slow else WARMUP), streams,
                        2 if slow else REGION_ITERS))
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
        print("{:22s} {:27s} {:10.4f} ms / iteration  (x{:.2f} of l1; regions {}){}"
              .format(label, name, med, med / base, " ".join("{:.4f}".format(t) for t in v), share),
              flush=True)


def main():
    small = "--small" in sys.argv
    shapes = [(1, 4, 1025, 512), (32, 4, 1025, 512), (128, 4, 1025, 512), (1, 8, 2049, 1024)]
    if small:
        shapes = [(2, 4, 33, 64), (1, 8, 17, 64)]
    for B, N, F, T in shapes:
        X = torch.from_numpy(nmf_mixture_batch(7, B, N, F, T)).cuda()
        X = X / (X.abs().max() * (N * T) ** 0.5)  # (the scale normalize_by_spectral_norm leaves)
        skip = set()
        if N > 4 and not small:
            skip.add("MaskingPDSHVA direct sum")
        iteration_times(X, "B={} N={} F={} T={}".format(B, N, F, T), skip)
        del X
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
