#!/usr/bin/env python3
"""MaskingADMMHVA iterations on the device route against the only way to run HVA under ADMM
without it.

ms per update_once() of MaskingADMMHVA (the cepstral pass on its automatic route, the FFT at these
sizes), of MaskingADMMBSS carrying the same mask as a host closure (Z to the host and a complex128
mask back up every iteration: the route before this class), and beside them MaskingPDSHVA and
ADMMIVA on the same mixtures: configs[1] (N=4, F=1025, T=512) with 1, 32 and 128 mixtures and
configs[2] (N=8, F=2049, T=1024) with one.  Relaxation 1.  The mixtures are scaled to RMS 0.1
("ADMMBSS": the scale condition).  Medians of three regions after a warm-up (DESIGN.md
section 5), a region of 20 iterations and 0.3 s at least (one iteration for the host closure), the
methods of a shape alternating.  For the device forms the achieved share of the HBM peak is printed
from the algorithmic bytes of the passes as written ("HVA"), and the ratio to
MaskingPDSHVA beside the ratio the two stream counts predict.

    python benchmarks/admmhva.py [--small]      # --small: a rehearsal at toy sizes
"""
import gc
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssspy_amd.bss.admmbss import MaskingADMMBSS  # noqa: E402
from ssspy_amd.bss.hva import MaskingADMMHVA, MaskingPDSHVA  # noqa: E402
from ssspy_amd.bss.iva import ADMMIVA  # noqa: E402
from ssspy_amd.utils.dataset import nmf_mixture_batch  # noqa: E402

REGIONS, REGION_ITERS, WARMUP = 3, 20, 3
REGION_SECONDS = 0.3
HBM_PEAK = 8.0e12  # bytes / s


def host_closure():
    """The parent's route: the mask of a MaskingADMMHVA object, passed as any user closure."""
    mask_fn = MaskingADMMHVA().mask_fn
    return MaskingADMMBSS(mask_fn=lambda z: mask_fn(z), scale_restoration=False)


# (name, constructor, 16-byte spectrogram-sized streams per iteration as the passes are written, at
# relaxation 1.  MaskingADMMHVA: the contraction reads 3 (auxiliary2, dual2, X); the cepstral pass
# reads 2 (X, dual2) and writes half a stream (real); the masked auxiliary step reads 2 1/2 and writes
# 2.  MaskingPDSHVA 8 and ADMMIVA 9: DESIGN.md.  None: host-bound)
FORMS = [
    ("MaskingPDSHVA", lambda: MaskingPDSHVA(scale_restoration=False), 8.0),
    ("MaskingADMMHVA", lambda: MaskingADMMHVA(scale_restoration=False), 10.0),
    ("ADMMIVA", lambda: ADMMIVA(scale_restoration=False, record_loss=False), 9.0),
    ("MaskingADMMBSS host closure", host_closure, None),
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


def iteration_times(X, label):
    B, N, F, T = X.shape
    entries = []
    for name, make, streams in FORMS:
        slow = streams is None
        # (the host-bound form: one iteration per region, one warm-up)
        m = prepared(make, X, 1 if slow else WARMUP)
        iters = 1
        if not slow:  # (a region of REGION_SECONDS at least: a short window times the scheduler)
            iters = min(max(REGION_ITERS, int(REGION_SECONDS / (1e-3 * region(m, 5))) + 1), 2000)
        entries.append((name, m, streams, iters))
    ms = [[] for _ in entries]
    gc.collect()
    for _ in range(REGIONS):
        for k, (_, m, _, iters) in enumerate(entries):  # (alternating: drift hits every method alike)
            ms[k].append(region(m, iters))
    base, base_streams = statistics.median(ms[0]), entries[0][2]
    for (name, _, streams, _), v in zip(entries, ms):
        med = statistics.median(v)
        share = ""
        if streams:
            nbytes = streams * 16.0 * B * N * F * T
            share = ("  {:.0f} streams, {:.0f} MB / mixture, {:.2f} of the HBM peak; streams predict "
                     "x{:.2f}").format(streams, nbytes / B / 1e6, nbytes / (med * 1e-3) / HBM_PEAK,
                                       streams / base_streams)
        print("{:22s} {:28s} {:10.4f} ms / iteration  (x{:.2f} of MaskingPDSHVA; regions {}){}"
              .format(label, name, med, med / base, " ".join("{:.4f}".format(t) for t in v), share),
              flush=True)


def main():
    small = "--small" in sys.argv
    shapes = [(1, 4, 1025, 512), (32, 4, 1025, 512), (128, 4, 1025, 512), (1, 8, 2049, 1024)]
    if small:
        shapes = [(2, 4, 33, 64), (1, 8, 17, 64)]
    for B, N, F, T in shapes:
        X = torch.from_numpy(nmf_mixture_batch(7, B, N, F, T)).cuda()
        X = X * (0.1 / X.abs().pow(2).mean().sqrt())  # RMS 0.1
        iteration_times(X, "B={} N={} F={} T={}".format(B, N, F, T))
        del X
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
