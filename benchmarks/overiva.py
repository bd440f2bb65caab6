#!/usr/bin/env python3
"""Per-iteration cost of OverIVA at 8 channels against the 8-source AuxLaplaceIVA-IP1 iteration.

    python benchmarks/overiva.py > profiles/overiva.txt

M = 8 channels, F = 1025 bins, T = 512 frames, 1 and 32 mixtures; OverLaplaceIVA with N = 1, 2, 4
sources and AuxLaplaceIVA (spatial_algorithm="IP", 8 sources) in the same process, alternating, on
the same mixtures.  An iteration is ``update_once()`` (no loss, no callbacks); a round is ``--iters``
iterations between two device synchronisations, timed with the host clock; the figure is the median
over ``--rounds`` rounds after a warm-up round, with the spread (min .. max) beside it.  Needs a
device: there is no CPU path.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mixture(torch, B, M, F, T, seed=0):
    """Two sources with frame-wise activity through random mixing per bin plus a weak white
    background, (B, M, F, T) complex128, drawn on the device."""
    gen = torch.Generator(device="cuda").manual_seed(seed)

    def randn(*shape):
        return torch.randn(*shape, dtype=torch.complex128, device="cuda", generator=gen)

    act = torch.rand(B, 2, 1, T, dtype=torch.float64, device="cuda", generator=gen) ** 4 + 0.05
    S = act * randn(B, 2, F, T)
    A = randn(B, F, M, 2)
    return (torch.einsum("bfmn,bnft->bmft", A, S) + 0.1 * randn(B, M, F, T)).contiguous()


def main():
    import torch

    from ssspy_amd.bss.iva import AuxLaplaceIVA
    from ssspy_amd.bss.overiva import OverLaplaceIVA

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bins", type=int, default=1025)
    ap.add_argument("--frames", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/overiva.py needs a HIP device")
    M, F, T = 8, args.bins, args.frames
    print("# {}  M={} F={} T={}  {} iterations per round, median of {} rounds (min .. max), ms per "
          "iteration".format(torch.cuda.get_device_name(0), M, F, T, args.iters, args.rounds))
    print("{:>9s} {:>26s} {:>10s} {:>20s} {:>8s}".format("mixtures", "separator", "ms / iter",
                                                       "spread", "ratio"))
    for B in (1, 32):
        X = mixture(torch, B, M, F, T)
        models = [("AuxLaplaceIVA-IP1 8 sources", AuxLaplaceIVA(spatial_algorithm="IP",
                                                                record_loss=False))]
        models += [("OverLaplaceIVA N={}".format(N), OverLaplaceIVA(n_sources=N, record_loss=False))
                   for N in (1, 2, 4)]
        for _, m in models:
            m._bind_input(X)
            m._reset()
        times = {name: [] for name, _ in models}
        for r in range(args.rounds + 1):
            for name, m in models:  # alternating: every round times every separator once
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    m.update_once()
                torch.cuda.synchronize()
                if r > 0:  # (round 0 warms every shape up)
                    times[name].append((time.perf_counter() - t0) / args.iters * 1e3)
        base = float(np.median(times[models[0][0]]))
        for name, m in models:
            m._check_device_errors()
            t = np.array(times[name])
            print("{:>9d} {:>26s} {:10.3f} {:>20s} {:8.2f}".format(
                B, name, float(np.median(t)), "{:.3f} .. {:.3f}".format(t.min(), t.max()),
                float(np.median(t)) / base))


if __name__ == "__main__":
    main()
