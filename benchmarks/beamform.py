#!/usr/bin/env python3
"""The mask-based beamformers beside two comparisons in the same process.

ms per call of ssspy_beamform_run (one launch: covariances, filters, output) for MVDR, GEV and MWF
at M=4, N=4, F=1025, T=512 and at M=8, N=2, F=2049, T=1024 with 1, 32 and 128 mixtures, beside
  * the same computation written as a chain of torch operators (a matmul per mask for the
    covariances, torch.linalg.cholesky / solve_triangular / eigh, an einsum for the output) -- what a
    user would write today; batches go through it in chunks of 8 mixtures, and
  * one CACGMM iteration on the same spectrograms, for scale.
Medians of three regions after a warm-up, the methods of a shape alternating.  The kernel lines also
give the fraction of the HBM peak (8.0 TB/s) on the algorithmic bytes,
B F (16 M T + 8 N T + 16 N T + 16 N M).

    python benchmarks/beamform.py [--small] [--mixtures 1 32] > profiles/beamform.txt
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssspy_amd import _device as dv  # noqa: E402
from ssspy_amd import _lib, _ops  # noqa: E402

REGIONS, TORCH_CHUNK = 3, 8
HBM_PEAK = 8.0e12
LOADING, MU, EPS = 1e-6, 1.0, 1e-10
ROUTE_NAMES = {_lib.BEAMFORM_ROUTE_RESIDENT: "resident", _lib.BEAMFORM_ROUTE_STREAMING: "streaming"}
KINDS = (("MVDR", _lib.BEAMFORM_MVDR, LOADING), ("GEV", _lib.BEAMFORM_GEV_REFERENCE, LOADING),
         ("MWF", _lib.BEAMFORM_MWF, 0.0))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def torch_chain(X, mask, kind, loading):
    """The beamformer on X (B, M, F, T), mask (B, N, F, T) with torch operators: (W (B, F, N, M) rows
    w^H, Y (B, N, F, T))."""
    B, M, F, T = X.shape
    N = mask.shape[1]
    Xt = X.permute(0, 2, 1, 3)  # (B, F, M, T)
    XH = Xt.conj().transpose(-1, -2)
    eye = torch.eye(M, dtype=X.dtype, device=X.device)
    rows = []
    for n in range(N):
        m = mask[:, n][:, :, None, :]  # (B, F, 1, T)
        u = 1.0 - m
        Ps = ((Xt * m) @ XH) / torch.clamp(m.sum(-1), min=EPS)[..., None]
        Pv = ((Xt * u) @ XH) / torch.clamp(u.sum(-1), min=EPS)[..., None]
        trace = Pv.diagonal(dim1=-2, dim2=-1).sum(-1).real
        Pv = Pv + (loading * trace / M)[..., None, None] * eye
        if kind == _lib.BEAMFORM_MWF:
            Pv = Ps + MU * Pv
        L = torch.linalg.cholesky(Pv)
        if kind == _lib.BEAMFORM_GEV_REFERENCE:
            Z = torch.linalg.solve_triangular(L, Ps, upper=False)
            C = torch.linalg.solve_triangular(L, Z.mH, upper=False).mH
            v = torch.linalg.eigh((C + C.mH) / 2)[1][..., -1:]
            w0 = torch.linalg.solve_triangular(L.mH, v, upper=True)[..., 0]
            a = (L @ v)[..., 0]
            w = w0 * a[..., :1].conj()
        else:
            A = torch.cholesky_solve(Ps, L)
            w = A[..., 0]
            if kind == _lib.BEAMFORM_MVDR:
                tr = A.diagonal(dim1=-2, dim2=-1).sum(-1).real
                w = w / torch.clamp(tr, min=EPS)[..., None]
        rows.append(w.conj())
    W = torch.stack(rows, dim=2)  # (B, F, N, M)
    Y = torch.einsum("bfnm,bmft->bnft", W, X)
    return W, Y


def cacgmm_iteration(X, N):
    """A callable running one CACGMM iteration on X, or None with the reason."""
    try:
        from ssspy_amd.bss.cacgmm import CACGMM

        m = CACGMM(n_sources=N, record_loss=False, permutation_alignment=False)
        m.call_on_device(X, n_iter=1)
        return m.update_once, None
    except Exception as e:  # (a shape it does not take, memory)
        return None, "{}: {}".format(type(e).__name__, e)


def shape_times(label, X, mask):
    B, M, F, T = X.shape
    N = mask.shape[1]
    route, lds = _ops.beamform_route(B, M, N, F, T)
    info = dv.zeros((2,), dv.i32, X.device)
    nbytes = B * F * (16 * M * T + 8 * N * T + 16 * N * T + 16 * N * M)
    kept = {}

    def kernel(kind, loading):
        def fn():
            kept["k"] = _ops.beamform_run(X, mask, None, kind, 0, loading, MU, info=info)[:2]
        return fn

    def chain(kind, loading):
        def fn():
            Ws, Ys = [], []
            for b0 in range(0, B, TORCH_CHUNK):
                W, Y = torch_chain(X[b0:b0 + TORCH_CHUNK], mask[b0:b0 + TORCH_CHUNK], kind, loading)
                Ws.append(W)
                Ys.append(Y)
            kept["t"] = (torch.cat(Ws), torch.cat(Ys))
        return fn

    em, why = cacgmm_iteration(X, N)
    for name, kind, loading in KINDS:
        entries = [(name + " kernel (" + ROUTE_NAMES[route] + ")", kernel(kind, loading)),
                   (name + " torch operators", chain(kind, loading))]
        if em is not None:
            entries.append(("CACGMM iteration", em))
        for _, fn in entries:
            fn()  # warm-up: first-use allocations, code loading
        agree = float((kept["k"][1] - kept["t"][1]).abs().max())
        ms = [[] for _ in entries]
        for _ in range(REGIONS):
            for k, (_, fn) in enumerate(entries):
                ms[k].append(timed(fn))
        med = [statistics.median(v) for v in ms]
        for k, ((entry, _), m, v) in enumerate(zip(entries, med, ms)):
            extra = ", {:.1f} % of the HBM peak on the algorithmic bytes".format(
                100 * nbytes / (m * 1e-3) / HBM_PEAK) if k == 0 else ""
            print("{:26s} {:26s} {:10.4f} ms  (x{:.3f} of the torch chain{}; regions {})".format(
                label, entry, m, m / med[1], extra, " ".join("{:.4f}".format(t) for t in v)),
                flush=True)
        print("{:26s} {}: max |Y kernel - Y torch| {:.2e}".format(label, name, agree), flush=True)
        kept.clear()
        torch.cuda.empty_cache()
    print("{:26s} LDS {} bytes / workgroup; failed solves {}{}".format(
        label, lds, int(info[0].item()),
        "" if why is None else "; CACGMM iteration not measured ({})".format(why)), flush=True)


def make(B, M, N, F, T, seed, dev):
    """Random steering vectors, sparse sources of RMS 1, 0.1 of noise, ideal ratio masks: the draw of
    tests/beamform_cases.py, made on the device."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)

    def cnormal(shape):
        return torch.complex(torch.randn(shape, generator=g, device=dev, dtype=torch.float64),
                             torch.randn(shape, generator=g, device=dev, dtype=torch.float64)) / 2 ** 0.5

    h = cnormal((B, F, N, M))
    s = cnormal((B, N, F, T)) * (torch.rand((B, N, F, T), generator=g, device=dev) < 0.5)
    X = torch.einsum("bfnm,bnft->bmft", h, s) + 0.1 * cnormal((B, M, F, T))
    power = (h.abs() ** 2).sum(-1).permute(0, 2, 1)[..., None] * s.abs() ** 2
    mask = power / (power.sum(1, keepdim=True) + M * 0.01)
    return X.contiguous(), mask.contiguous()


def main():
    dev = torch.device("cuda", 0)
    mixtures = [1, 32, 128]
    if "--mixtures" in sys.argv:
        at = sys.argv.index("--mixtures") + 1
        mixtures = [int(v) for v in sys.argv[at:] if v.isdigit()]
    shapes = [(4, 4, 1025, 512), (8, 2, 2049, 1024)]
    if "--small" in sys.argv:
        shapes, mixtures = [(4, 4, 33, 128), (8, 2, 17, 600)], [2]
    print("# mask-based beamformers: ms per call (covariances, filters and output), diagonal_loading "
          "{} (MWF 0), mu {}; HBM peak {:.1f} TB/s".format(LOADING, MU, HBM_PEAK / 1e12))
    for M, N, F, T in shapes:
        for B in mixtures:
            label = "m{} n{} f{} t{} x{}".format(M, N, F, T, B)
            X, mask = make(B, M, N, F, T, 1000 + M, dev)
            shape_times(label, X, mask)
            del X, mask
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
