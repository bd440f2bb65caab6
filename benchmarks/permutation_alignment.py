"""Permutation alignment on the device against the host solvers, and inside a whole FDICA call.

    python benchmarks/permutation_alignment.py [--out FILE] [--quick]

Three measurements, all with a host clock around work that ends in a device synchronise, the
median of the repeats after a warm-up at the same shape:

* each device solver (csrc/permutation.hip: envelope/overlap + sweep; normalise + global + local,
  1 + 1 iterations) on a device-resident (B, N, F, T) sequence, per pass;
* the NumPy solver of ssspy_amd.algorithm.permutation_alignment on this machine's CPU, one mixture,
  host arrays in and out (what the host route runs per mixture, without its PCIe copies);
* the whole ``NaturalGradLaplaceFDICA`` call, 100 iterations, with route ``device_alignment`` on
  and off, and without alignment (the iterations alone).

Shapes: N=4, F=1025, T=512 with 1 / 32 / 128 mixtures, and N=8, F=2049, T=1024 with 1 mixture.
The algorithmic bytes of a pass are computed from the shapes ("Permutation
alignment") and printed beside its time.
"""

import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sources(seed, B, N, F, T):
    """(B, N, F, T) complex: sources with distinct frame envelopes, shuffled per bin."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    out = np.empty((B, N, F, T), dtype=np.complex128)
    for b in range(B):
        centre = (rng.permutation(N) + 0.5) * T / N
        env = 0.2 + 2.0 * np.exp(-0.5 * ((t[None, :] - centre[:, None]) / (0.4 * T / N)) ** 2)
        noise = rng.standard_normal((N, F, T)) + 1j * rng.standard_normal((N, F, T))
        Y = env[:, None, :] * noise
        for f in range(F):
            Y[:, f] = Y[rng.permutation(N), f]
        out[b] = Y
    return out


def timed(fn, repeats, sync):
    fn()
    sync()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=None)
    parser.add_argument("--quick", action="store_true", help="small shapes (a rehearsal)")
    args = parser.parse_args()

    import torch

    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    from ssspy_amd import _device as dv
    from ssspy_amd import _lib, _ops, _routes
    from ssspy_amd.algorithm.permutation_alignment import (
        correlation_based_permutation_solver,
        device_correlation_permutation,
        device_score_permutation,
        score_based_permutation_solver,
    )
    from ssspy_amd.bss.fdica import NaturalGradLaplaceFDICA
    from ssspy_amd.utils.dataset import nmf_mixture
    from ssspy_amd.utils.flooring import device_flooring

    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    sync = torch.cuda.synchronize
    floor = device_flooring(NaturalGradLaplaceFDICA().flooring_fn)
    shapes = [(4, 1025, 512, 1), (4, 1025, 512, 32), (4, 1025, 512, 128), (8, 2049, 1024, 1)]
    if args.quick:
        shapes = [(4, 65, 128, 1), (4, 65, 128, 4), (8, 17, 64, 1)]
    say("device: {}".format(torch.cuda.get_device_name(0)))
    say("times in ms: median (min .. max) of the repeats; MB: algorithmic bytes of the pass")

    for N, F, T, B in shapes:
        repeats = 3 if N == 8 or B > 32 else 7
        say()
        say("== N={} F={} T={} mixtures={}".format(N, F, T, B))
        Y = sources(1, min(B, 4), N, F, T)
        Yd = dv.to_device(np.concatenate([Y] * (B // len(Y) + 1))[:B])
        Sd = (Yd.real ** 2 + Yd.imag ** 2).contiguous()
        elems = B * N * F * T

        def ms(stat):
            return "{:9.3f} ({:.3f} .. {:.3f})".format(*(1e3 * s for s in stat))

        # ---- the device solvers, pass by pass
        env, overlap = _ops.permutation_envelope_overlap(Yd, floor)
        order = torch.argsort(overlap, dim=1).to(torch.int32).contiguous()
        say("correlation  envelope+overlap {}  {:8.1f} MB".format(
            ms(timed(lambda: _ops.permutation_envelope_overlap(Yd, floor), repeats, sync)),
            elems * 24 / 1e6))
        say("correlation  sweep            {}  {:8.1f} MB".format(
            ms(timed(lambda: _ops.permutation_correlation_sweep(env, order), repeats, sync)),
            elems * 16 / 1e6))
        dev_corr = timed(lambda: device_correlation_permutation(Yd, floor), repeats, sync)
        say("correlation  whole solver     {}  (with the overlaps down, the order up)".format(
            ms(dev_corr)))
        norm = _ops.permutation_score_normalize(Sd)
        perm = _ops.permutation_identity(B, F, N, Sd.device)
        say("score        normalize        {}  {:8.1f} MB".format(
            ms(timed(lambda: _ops.permutation_score_normalize(Sd), repeats, sync)),
            elems * 32 / 1e6))
        say("score        global, 1 round  {}  {:8.1f} MB".format(
            ms(timed(lambda: _ops.permutation_score_global(norm, perm.clone(), 1, floor), repeats,
                     sync)), elems * 16 / 1e6))
        cstd = _ops.permutation_score_global(norm, perm, 1, floor)
        say("score        local, 1 round   {}  {:8.1f} MB (13 neighbours)".format(
            ms(timed(lambda: _ops.permutation_score_local(norm, cstd, perm.clone(), 1, floor),
                     repeats, sync)), elems * 8 * 14 / 1e6))
        dev_score = timed(lambda: device_score_permutation(Sd, floor, 1, 1), repeats, sync)
        say("score        whole solver     {}".format(ms(dev_score)))
        say("gather       (B, N, F, T) c128 {}  {:8.1f} MB".format(
            ms(timed(lambda: _ops.permute_sources(Yd, perm, _lib.PERM_LAYOUT_SOURCE_BIN), repeats,
                     sync)), elems * 32 / 1e6))

        # ---- the host solvers on this machine's CPU, one mixture
        Yh = np.ascontiguousarray(Y[0].transpose(1, 0, 2))  # (F, N, T)
        Sh = np.abs(Yh) ** 2
        host_repeats = 1 if N == 8 else 3
        host_corr = timed(lambda: correlation_based_permutation_solver(Yh.copy()), host_repeats,
                          lambda: None)
        host_score = timed(lambda: score_based_permutation_solver(Sh.copy()), host_repeats,
                           lambda: None)
        say("host         correlation, 1 mixture {}".format(ms(host_corr)))
        say("host         score, 1 mixture       {}".format(ms(host_score)))
        say("ratio host x mixtures / device: correlation {:.1f}, score {:.1f}".format(
            host_corr[0] * B / dev_corr[0], host_score[0] * B / dev_score[0]))

        # ---- the whole FDICA call (N = 4 only: the bin-resident kernel takes 2..4 sources)
        if N != 4 and not args.quick:
            continue
        X = np.stack([nmf_mixture(1000 + b, N, F, T) for b in range(min(B, 4))])
        X = np.concatenate([X] * (B // len(X) + 1))[:B]
        n_iter = 100

        def call(alignment):
            m = NaturalGradLaplaceFDICA(permutation_alignment=alignment, record_loss=False)
            return m(X, n_iter=n_iter)

        results = {}
        for label, alignment, device in (("no alignment", False, True), ("device route", True, True),
                                         ("host route", True, False)):
            if label == "host route" and B > 32:
                say("FDICA call   {:13s} not measured (minutes on the host at this batch)".format(
                    label))
                continue
            with _routes.override(device_alignment=device):
                results[label] = timed(lambda: call(alignment), 3, sync)
            say("FDICA call   {:13s} {}  (uploads and the download of the output included)".format(
                label, ms(results[label])))
        # the 100 iterations alone, on the state the last call left (one launch of the kernel)
        m = NaturalGradLaplaceFDICA(permutation_alignment=False, record_loss=False)
        m(X, n_iter=1)
        loop = timed(lambda: m._kernel_steps(n_iter, m._floor), 5, sync)
        say("FDICA        100 iterations {}  (ssspy_fdica_steps alone)".format(ms(loop)))
        say("device correlation solver / 100 iterations: {:.2f}".format(dev_corr[0] / loop[0]))
        if "host route" in results:
            say("whole call, host route / device route: {:.2f}".format(
                results["host route"][0] / results["device route"][0]))
        say("alignment share of the device-route call: {:.3f} ms of {:.3f} ms".format(
            1e3 * (results["device route"][0] - results["no alignment"][0]),
            1e3 * results["device route"][0]))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
