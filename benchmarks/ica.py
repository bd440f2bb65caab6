#!/usr/bin/env python3
"""Time-domain ICA: ms per iteration of the device route, of the same iteration written as a chain
of torch-ROCm operators, and of the compatibility route.

Classes: GradLaplaceICA, NaturalGradLaplaceICA and FastICA with the log-cosh triple.  Sizes: N = 4,
T = 160000 (10 s at 16 kHz) at 1 / 32 / 128 mixtures; N = 8, T = 480000 at 1 / 32.  Medians of three
20-iteration regions after a warm-up, the contenders of a shape alternating.
An iteration of the device route is the statistics pass plus the step kernel; the share of the HBM
peak counts the one stream the pass reads (8 N T bytes per mixture) against the 8 TB/s of the part.
The compatibility route (a closure around the named functions) is timed over three iterations.

    python benchmarks/ica.py [--small] [--out profiles/ica.txt]
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ssspy_amd.bss import ica  # noqa: E402

HBM_PEAK = 8.0e12
REGIONS, REGION_ITERS, WARMUP = 3, 20, 5
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def named(closures=False):
    g, s, d = ica.NAMED["logcosh"]
    if closures:
        lg, ls, _ = ica.NAMED["laplace"]
        return [("GradLaplaceICA", lambda **kw: ica.GradICA(
                    contrast_fn=lambda y: lg(y), score_fn=lambda y: ls(y), **kw)),
                ("NaturalGradLaplaceICA", lambda **kw: ica.NaturalGradICA(
                    contrast_fn=lambda y: lg(y), score_fn=lambda y: ls(y), **kw)),
                ("FastICA-logcosh", lambda **kw: ica.FastICA(
                    contrast_fn=lambda y: g(y), score_fn=lambda y: s(y), d_score_fn=lambda y: d(y),
                    **kw))]
    return [("GradLaplaceICA", ica.GradLaplaceICA),
            ("NaturalGradLaplaceICA", ica.NaturalGradLaplaceICA),
            ("FastICA-logcosh", lambda **kw: ica.FastICA(contrast_fn=g, score_fn=s, d_score_fn=d,
                                                         **kw))]


def prepared(make, X, warmup=WARMUP):
    m = make(record_loss=False)
    m._bind_input(X)
    m._reset()
    for _ in range(warmup):
        m.update_once()
    return m


def torch_chain(name, X):
    """The same iteration as torch operators on the device (FastICA: the statistics only, its
    Gram-Schmidt step has no batched torch form worth the name)."""
    B, N, T = X.shape
    W = torch.eye(N, dtype=X.dtype, device=X.device).repeat(B, 1, 1)
    off = 1.0 - torch.eye(N, dtype=X.dtype, device=X.device)

    def step():
        Y = W @ X
        if name == "FastICA-logcosh":
            th = torch.tanh(Y)
            M = th @ X.transpose(1, 2) / T
            d = (1.0 - th * th).mean(dim=2)
            return M, d
        PhiY = torch.sign(Y) @ Y.transpose(1, 2) / T
        D = off * PhiY
        if name == "GradLaplaceICA":
            delta = D @ torch.linalg.inv(W).transpose(1, 2)
        else:
            delta = D @ W
        W.sub_(0.1 * delta)
        return W
    return step


def region(fn, iters=REGION_ITERS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def bench_shape(label, B, N, T, seed):
    rng = np.random.default_rng(seed)
    S = torch.from_numpy(rng.laplace(size=(B, N, T)))
    A = torch.eye(N, dtype=torch.float64) + 0.4 * torch.from_numpy(rng.standard_normal((B, N, N)))
    X = (A @ S).to(torch.device("cuda", 0))
    X *= 0.3 / X.pow(2).mean().sqrt()
    del S
    nbytes = 8.0 * B * N * T
    say("{}: B={} N={} T={} ({:.1f} MB read per pass{})".format(
        label, B, N, T, nbytes / 1e6,
        "; fits the caches, the share of the HBM peak is nominal" if nbytes < 256e6 else ""))
    contenders = []
    for name, make in named():
        m = prepared(make, X)
        chain = torch_chain(name, m._source())
        for _ in range(WARMUP):
            chain()
        contenders.append((name, m.update_once, chain))
    ms = {(name, k): [] for name, _, _ in contenders for k in (0, 1)}
    for _ in range(REGIONS):
        for name, kernel, chain in contenders:
            ms[(name, 0)].append(region(kernel))
            ms[(name, 1)].append(region(chain))
    for name, _, _ in contenders:
        k, c = statistics.median(ms[(name, 0)]), statistics.median(ms[(name, 1)])
        say("  {:22s} kernels {:9.4f} ms / iteration ({:5.1f} % of the HBM peak)   torch chain "
            "{:9.4f} ms   kernels / chain {:.3f}".format(name, k, 100 * nbytes / (k * 1e-3) / HBM_PEAK,
                                                         c, k / c))
    del contenders
    for name, make in named(closures=True):
        m = prepared(make, X, warmup=1)
        say("  {:22s} compatibility route {:9.2f} ms / iteration".format(
            name, region(m.update_once, iters=3)))
    del X
    torch.cuda.empty_cache()


def main():
    small = "--small" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "ica.txt")
    shapes = [("10 s x1", 1, 4, 160000), ("10 s x32", 32, 4, 160000), ("10 s x128", 128, 4, 160000),
              ("30 s, 8 ch x1", 1, 8, 480000), ("30 s, 8 ch x32", 32, 8, 480000)]
    if small:
        shapes = [("small x1", 1, 4, 5000), ("small x3", 3, 8, 7000)]
    say("benchmarks/ica.py on {}".format(torch.cuda.get_device_name(0)))
    for i, (label, B, N, T) in enumerate(shapes):
        bench_shape(label, B, N, T, 100 + i)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
