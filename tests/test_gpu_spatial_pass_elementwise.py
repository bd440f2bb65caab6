"""Every ISS, IP2 and scale-restoration entry point alone against the extended-precision restatement
of tests/spatial_reference.py (the bar rules are in its module docstring: elementwise m u companion
for the plain sums, c g u |ref| per bin for solves and recurrences, c = 8 x the float64 restatement's
own g-normalised error on the same inputs, a unit phase per eigenvector row and nothing else gauged).

Branches (every case names the one it reaches):

* fused ISS1 (iss_fused.hip): sources in one reduction group up to 4, two groups of 4 at 5..8 with
  the last one padded at 5..7; frames per thread 1 / 2 / 4 / 8 for T <= 256 / 512 / 1024 / 2048 (8
  only up to 4 sources; beyond: UNSUPPORTED); bins per block ceil(B F / 1024), at most 8, 16 when
  r2_next is asked for, the last block ragged.
* ISS1 transform, ip1_source_solve, projection back, demix: compiled per N at 2..8
  (spatial_kernels.hip), run-time N at 9..16 (wide_n.hip).
* ISS2 transform: rows form (a bin on a lane group) at 2..8, run-time form at 9..16.
* IP2: one lane per bin at 2..4, eight lanes per bin at 5..8 (B F = 33: a partial group of a block),
  run-time N at 9..16.

Run as a script on the GPU to rewrite profiles/spatial_pass_elementwise.txt.
"""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pass_reference as pr  # noqa: E402
import spatial_reference as sr  # noqa: E402
from test_gpu_pass_elementwise import Out, _mods, check, up  # noqa: E402

pytestmark = pytest.mark.gpu

LD = pr.LD
MAXF, ADDF, NOF = (pr.FLOOR_MAX, pr.EPS), (pr.FLOOR_ADD, pr.EPS), (pr.FLOOR_NONE, 0.0)
FLOORS = (NOF, MAXF, ADDF)
BINS = [(1, 1), (1, 17), (5, 13), (3, 11)]  # B F = 1, 17, 65, 33


class HostFloor:
    """A flooring the kernels cannot run: _ops takes the deferred route (denominators to the host)."""

    def __init__(self, flooring):
        self.flooring = flooring

    def host(self, d):
        return pr.floor(np.asarray(d, dtype=np.float64), self.flooring)


def record(entry, route, err, c, extra=""):
    """A normwise result: err and the bar c in units of g u |ref|."""
    line = "{}\t{}\t{:.3f}\t{:.3f}\t{:.4f}\t{}".format(entry, route, err, c, err / c, extra)
    print(line)
    path = os.environ.get("SSSPY_PASS_PROFILE_RAW")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    assert err <= c, line


def pair_lists(N):
    from ssspy_amd.utils.select_pair import resolve_pairs, sequential_pair_selector

    return {"iss2": resolve_pairs(lambda n: sequential_pair_selector(n, stop=n, step=2), N),
            "seq": resolve_pairs(sequential_pair_selector, N)}


def form(N):
    return "per-N" if N <= 8 else "run-time N"


# ------------------------------------------------------------------------------- fused ISS1
def _fused_branch(N, T, bpb=1):
    groups = "1 group" if N <= 4 else ("2 groups" if N == 8 else "2 groups, last padded")
    fpt = 1 if T <= 256 else 2 if T <= 512 else 4 if T <= 1024 else 8
    return "N{} {} FPT{} bpb{}".format(N, groups, fpt, bpb)


def _run_fused(Y, w, kind, flooring, tracked, with_r2, ld0):
    _, dv, _, ops = _mods()
    B, N, F, T = Y.shape
    oY = Out(Y.shape, True, fill=Y)
    oR = Out((B, N, T)) if with_r2 else None
    oL = Out((B,), fill=ld0) if tracked else None
    ops.iss1_fused(oY.t, up(w), kind, flooring, r2_next=oR.t if oR else None,
                   logdet=oL.t if oL else None)
    return oY.get(), oR.get() if oR else None, oL.get() if oL else None


def _fused_case(B, N, F, T, floors, kinds=(sr.FRAME, sr.BIN_FRAME), bpb=(1, 1), seed=0):
    ld0 = np.linspace(-37.5, 11.25, B)
    for kind in kinds:
        Y, w = sr.gen_iss_inputs(seed + 31 * N + T + kind, B, N, F, T, kind)
        for flooring in floors:
            ref = sr.iss1_fused(Y, w, kind, flooring)
            assert float(ref["d"].min()) > 1e-300
            e64 = sr.rowwise(sr.iss1_fused(Y, w, kind, flooring, dtype=np.float64)["Y"], ref["Y"],
                             ref["comp"])
            c = sr.yardstick(e64)
            extra = "(c_f64 {:.3f}, g max {:.1f})".format(e64, float(ref["g"].max()))
            first = None
            for tracked in (False, True):
                for with_r2 in (False, True):
                    per_block = bpb[1] if with_r2 else bpb[0]
                    route = "{} kind{} floor{}".format(_fused_branch(N, T, per_block), kind, flooring[0])
                    name = "iss1_fused_tracked" if tracked else "iss1_fused"
                    gY, gR, gL = _run_fused(Y, w, kind, flooring, tracked, with_r2, ld0)
                    assert np.all(np.isfinite(gY))
                    record(name + "_Y", route, sr.rowwise(gY, ref["Y"], ref["comp"]), c, extra)
                    if with_r2:
                        r2, bar = sr.frame_power_of(gY)
                        check(name + "_r2_next", route, gR, r2, bar)
                    if tracked:
                        nblk = -(-F // per_block)
                        val, bar = sr.iss1_logdet(ref, ld0, c, T, nblk)
                        check(name + "_logdet", route, gL, val, bar)
                    if tracked and with_r2:
                        first = (gY, gR, gL)
            again = _run_fused(Y, w, kind, flooring, True, True, ld0)
            for a, b in zip(first, again):
                assert np.array_equal(a, b), "two runs differ"


FUSED_NT = [(N, T) for N in (2, 3, 4, 5, 7, 8) for T in (1, 63, 255, 256, 257, 512, 513, 1024, 1025, 2048)
            if T <= 1024 or N <= 4]


@pytest.mark.parametrize("N,T", FUSED_NT)
def test_iss1_fused(N, T):
    """Untracked and tracked, with and without r2_next, FRAME and BIN_FRAME weights, the three floors;
    B = 2, F = 3 (one bin per block).  The first bin of the first mixture is 1e-6 of the others, so its
    denominators are floored under MAX.  T < N (T = 1) leaves a rank-deficient slab: from the second
    sweep on the denominators are the residue of an exact cancellation -- zero in exact arithmetic,
    the excluded band -- unless a floor holds them up, so that size runs under MAX and ADD only.
    logdet comes in non-zero; a tracked run with frame powers is repeated and must match bit for bit."""
    _fused_case(2, N, 3, T, FLOORS if T >= N else (MAXF, ADDF))


@pytest.mark.parametrize("N,T", [(2, 2049), (3, 2049), (4, 2049), (5, 1025), (7, 1025), (8, 1025)])
def test_iss1_fused_above_the_limit_is_unsupported(N, T):
    _, dv, _, ops = _mods()
    assert ops.iss1_fused_max_frames(N) == T - 1
    Y, w = sr.gen_iss_inputs(N, 1, N, 2, T, sr.FRAME)
    for tracked in (False, True):
        oY = Out(Y.shape, True, fill=Y)
        oL = Out((1,), fill=np.array([2.5]))
        with pytest.raises(NotImplementedError):
            ops.iss1_fused(oY.t, up(w), sr.FRAME, MAXF, logdet=oL.t if tracked else None)
        assert np.array_equal(oY.get(), Y) and np.array_equal(oL.get(), np.array([2.5]))


@pytest.mark.parametrize("F,bpb", [(1040, (2, 2)), (1025, (2, 2)), (15361, (8, 16))])
def test_iss1_fused_bins_per_block(F, bpb):
    """N = 2, T = 8, one mixture.  1040 bins: two per block; 1025: two per block and a last block of
    one; 15361 (just above 15 x 1024): 16 per block with r2_next, the cap of 8 without, both ragged."""
    assert F % bpb[0] == (0 if F == 1040 else 1) and F % bpb[1] == (0 if F == 1040 else 1)
    _fused_case(1, 2, F, 8, (MAXF,), bpb=bpb, seed=F)


# ------------------------------------------------------------------------------- ISS transforms
def _iss_stats(seed, B, N, F, T):
    Y, w = sr.gen_iss_inputs(seed, B, N, F, T, sr.BIN_FRAME)
    return Y, w, sr._f64(sr.iss_statistics(Y, w, sr.BIN_FRAME))


@pytest.mark.parametrize("B,F", BINS)
@pytest.mark.parametrize("N", [2, 3, 4, 5, 8, 9, 16])
def test_iss1_transform(N, B, F):
    """G of the N steps on the statistics of a real Y and real weights, the three floors; up to 8
    sources separate(Y, G) is also held against the fused kernel's Y within the sum of both bars."""
    _, dv, _, ops = _mods()
    T = 4 * N
    Y, w, Vc = _iss_stats(700 + N + F, B, N, F, T)
    route = "{} N{} BF{}".format(form(N), N, B * F)
    for flooring in FLOORS:
        G, g = sr.iss1_transform(Vc, flooring)
        e64 = sr.normwise(sr.iss1_transform(Vc, flooring, dtype=np.float64)[0], G, g, (-2, -1))
        c = sr.yardstick(e64)
        o = Out(G.shape, True)
        ops.iss1_transform(up(Vc), flooring, out=o.t)
        got = o.get()
        assert np.all(np.isfinite(got))
        record("iss1_transform", route + " floor{}".format(flooring[0]),
               sr.normwise(got, G, g, (-2, -1)), c,
               "(c_f64 {:.3f}, g max {:.1f})".format(e64, float(g.max())))
        if N > 8:
            continue
        # Y' = G Y by the kernels against the fused sweep on the same Y
        fused = sr.iss1_fused(Y, w, sr.BIN_FRAME, flooring)
        cf = sr.yardstick(sr.normwise(sr.iss1_fused(Y, w, sr.BIN_FRAME, flooring,
                                                    dtype=np.float64)["Y"], fused["Y"], fused["g"], -1))
        oY = Out(Y.shape, True, fill=Y)
        ops.iss1_fused(oY.t, up(w), sr.BIN_FRAME, flooring)
        oS = Out(Y.shape, True)
        ops.separate(up(Y), o.t, out=oS.t)
        _, sep_bar = pr.separate(Y, got)
        nrm = lambda a: np.sqrt((np.abs(a) ** 2).sum(axis=-1))  # noqa: E731
        bar_f = cf * fused["g"] * pr.U * nrm(fused["Y"])                                   # (B,N,F)
        normY = np.sqrt((np.abs(Y) ** 2).sum(axis=(1, 3)))                                 # (B,F)
        normG = np.sqrt((np.abs(G) ** 2).sum(axis=(-2, -1)))
        bar_t = (c * g * pr.U * normG * normY)[:, None, :] + nrm(sep_bar)
        ratio = float(np.max(nrm(oS.get().astype(np.clongdouble) - oY.get()) / (bar_f + bar_t)))
        record("iss1_transform_vs_fused", route + " floor{}".format(flooring[0]), ratio, 1.0)


@pytest.mark.parametrize("B,F", BINS)
@pytest.mark.parametrize("N", [2, 3, 4, 5, 8, 9, 16])
def test_iss2_transform(N, B, F):
    """The in-kernel floors and the deferred form (one pair per call, accumulate 0 then 1, the rows
    divided by the floored denominators with scale_filter_row) against the same reference; the pair
    lists of utils/select_pair.py: ISS2's default (every second pair) and the full sequential list,
    which wraps round at an odd N."""
    _, dv, _, ops = _mods()
    T = 4 * N
    _, _, Vc = _iss_stats(800 + N + F, B, N, F, T)
    for lname, pairs in pair_lists(N).items():
        rows = sorted({r for p in pairs for r in p})
        route = "{} N{} BF{} {}".format("rows" if N <= 8 else "run-time N", N, B * F, lname)
        for flooring in FLOORS:
            G, g, _ = sr.iss2_transform(Vc, pairs, flooring)
            G64 = sr.iss2_transform(Vc, pairs, flooring, dtype=np.float64)[0]
            e64 = sr.normwise(sr.align_phase(G64, G, rows), G, g, (-2, -1))
            c = sr.yardstick(e64)
            extra = "(c_f64 {:.3f}, g max {:.1f})".format(e64, float(g.max()))
            for name, fl in (("iss2_transform", flooring), ("iss2_transform_deferred", HostFloor(flooring))):
                info = dv.zeros((1,), dv.i32)
                o = Out(G.shape, True)
                ops.iss2_transform(up(Vc), pairs, fl, info=info, out=o.t)
                got = o.get()
                assert np.all(np.isfinite(got)) and int(info.item()) == 0
                record(name, route + " floor{}".format(flooring[0]),
                       sr.normwise(sr.align_phase(got, G, rows), G, g, (-2, -1)), c, extra)


# ------------------------------------------------------------------------------- IP1 / IP2
def _ip2_inputs(seed, B, F, N, pairs, pair_only):
    """Inputs whose every bin keeps kappa(W U) <= 1e4 and a relative eigen-gap >= 0.1 over the pairs
    walked: bins that miss either are redrawn (a property of the inputs, computed by the reference)."""
    W, Uc = sr.gen_ip2_inputs(seed, B, F, N, n_sets=2 if pair_only else None, log2_cond=8)
    for attempt in range(1, 40):
        parts = {}
        sr.update_by_ip2(W, Uc, pairs, NOF, pair_only, parts=parts)
        bad = (parts["kappa"] > 1e4) | (parts["gap"] < 0.1)
        if not bad.any():
            return W, Uc, parts
        W2, U2 = sr.gen_ip2_inputs(seed + 1000 * attempt, B, F, N, n_sets=2 if pair_only else None,
                                   log2_cond=8)
        W[bad], Uc[bad] = W2[bad], U2[bad]
    raise AssertionError("no well-separated inputs found")


def _floor_scale(Uc):
    """The covariance of the pair's first member times 1e26 in the first bin: P^H U P goes with 1 / U,
    so that member's sqrt(q) = sqrt(lamb) ends below eps = 1e-10 (floored under MAX)."""
    Uc = Uc.copy()
    Uc[0, 0, 0] *= 1e26
    return Uc


@pytest.mark.parametrize("B,F", BINS)
@pytest.mark.parametrize("pair_only", [0, 1])
@pytest.mark.parametrize("N", [2, 3, 4, 5, 6, 8, 9, 16])
def test_update_by_ip2(N, pair_only, B, F):
    """One pair and the full sequential list (pair_only: one pair, its own two covariances), the three
    floors in the kernel and deferred (update_by_ip2_deferred + scale_filter_row)."""
    _, dv, _, ops = _mods()
    lanes = "1 lane" if N <= 4 else ("8 lanes" if N <= 8 else "run-time N")
    plist = [[(N - 1, 0)]] if pair_only else [[(0, 1)], pair_lists(N)["seq"]]
    for pairs in plist:
        W, Uc, parts = _ip2_inputs(900 + 7 * N + F + pair_only, B, F, N, pairs, pair_only)
        route = "{} N{} BF{} pair_only{} pairs{}".format(lanes, N, B * F, pair_only, len(pairs))
        for flooring in FLOORS:
            Uf = _floor_scale(Uc) if (flooring[0] != pr.FLOOR_NONE and len(pairs) == 1) else Uc
            ref, g, _ = sr.update_by_ip2(W, Uf, pairs, flooring, pair_only)
            f64 = sr.update_by_ip2(W, Uf, pairs, flooring, pair_only, dtype=np.float64)[0]
            e64 = sr.normwise(sr.align_phase(f64, ref), ref, g[..., None], -1)
            c = sr.yardstick(e64)
            extra = "(c_f64 {:.3f}, kappa max {:.1f}, gap min {:.3f})".format(
                e64, float(parts["kappa"].max()), float(parts["gap"].min()))
            for name, fl in (("update_by_ip2", flooring), ("update_by_ip2_deferred", HostFloor(flooring))):
                info = dv.zeros((1,), dv.i32)
                o = Out(W.shape, True, fill=W)
                ops.update_by_ip2(o.t, up(Uf), pairs, fl, info=info, pair_only=bool(pair_only))
                got = o.get()
                assert np.all(np.isfinite(got)) and int(info.item()) == 0
                record(name, route + " floor{}".format(flooring[0]),
                       sr.normwise(sr.align_phase(got, ref), ref, g[..., None], -1), c, extra)


@pytest.mark.parametrize("N", [3, 6, 9])
def test_update_by_ip2_singular_bin(N):
    """One bin whose filter has a zero row (W U singular whatever U): info goes up by exactly one and
    every other bin stays within its bar."""
    _, dv, _, ops = _mods()
    B, F = 3, 11
    pairs = pair_lists(N)["seq"]
    W, Uc, _ = _ip2_inputs(950 + N, B, F, N, pairs, 0)
    ref, g, _ = sr.update_by_ip2(W, Uc, pairs, MAXF)
    f64 = sr.update_by_ip2(W, Uc, pairs, MAXF, dtype=np.float64)[0]
    c = sr.yardstick(sr.normwise(sr.align_phase(f64, ref), ref, g[..., None], -1))
    Ws = W.copy()
    Ws[1, 5, N - 1, :] = 0
    info = dv.zeros((1,), dv.i32)
    o = Out(W.shape, True, fill=Ws)
    ops.update_by_ip2(o.t, up(Uc), pairs, MAXF, info=info)
    got = o.get()
    assert int(info.item()) == 1
    keep = np.ones((B, F), bool)
    keep[1, 5] = False
    assert np.all(np.isfinite(got[keep]))
    record("update_by_ip2_singular_bin", "N{}".format(N),
           sr.normwise(sr.align_phase(got[keep], ref[keep]), ref[keep], g[keep][:, None], -1), c)


@pytest.mark.parametrize("B,N", [(2, 2), (2, 4), (2, 6), (2, 8), (2, 9), (1, 16)])
def test_ip1_source_solve_and_scale_filter_row(B, N):
    """update_by_ip1 through a host floor: ip1_source_solve then scale_filter_row per source must give
    the sweep of update_by_ip1 (the IP1 bar of test_gpu_pass_elementwise.py), and the first source's
    unnormalised row and denominator their own restatement."""
    _, dv, lib, ops = _mods()
    F = 17
    W, Uc = pr.gen_ip1_inputs(60 + N + B, B, F, N)
    ref, kappa = pr.update_by_ip1(W, Uc, MAXF)
    c_np = pr.ip1_row_error(pr.update_by_ip1_float64(W, Uc, MAXF), ref, kappa)
    info = dv.zeros((1,), dv.i32)
    o = Out(W.shape, True, fill=W)
    ops.update_by_ip1(o.t, up(Uc), HostFloor(MAXF), info)
    record("ip1_source_solve+scale_filter_row", "{} B{} N{}".format(form(N), B, N),
           pr.ip1_row_error(o.get(), ref, kappa), 8 * c_np,
           "(c_np {:.3f}, kappa max {:.1f})".format(c_np, float(kappa.max())))
    assert int(info.item()) == 0
    # the two calls on their own
    n = N - 1
    Wr, d, k = sr.ip1_source_solve(W, Uc, n)
    W64, d64, _ = sr.ip1_source_solve(W, Uc, n, dtype=np.float64)
    e64 = max(sr.normwise(W64, Wr, k[..., None], -1), sr.normwise(d64[..., None], d[..., None], k, -1))
    o, od = Out(W.shape, True, fill=W), Out((B, F))
    lib.check(lib.load().ssspy_ip1_source_solve(dv.ptr(o.t), dv.ptr(up(Uc)), dv.ptr(od.t), n, B, F, N,
                                               dv.ptr(info), dv.stream_handle()), "ip1_source_solve")
    got, gd = o.get(), od.get()
    record("ip1_source_solve", "{} B{} N{}".format(form(N), B, N),
           max(sr.normwise(got, Wr, k[..., None], -1), sr.normwise(gd[..., None], d[..., None], k, -1)),
           sr.yardstick(e64), "(c_f64 {:.3f}, kappa max {:.1f})".format(e64, float(k.max())))
    dd = np.exp2(np.random.default_rng(N).uniform(-30, 30, (B, F)))
    out, bar = sr.scale_filter_row(got, dd, n)
    o = Out(W.shape, True, fill=got)
    lib.check(lib.load().ssspy_scale_filter_row(dv.ptr(o.t), dv.ptr(up(dd)), n, B, F, N,
                                               dv.stream_handle()), "scale_filter_row")
    res = o.get()
    rows = np.arange(N) != n
    assert np.array_equal(res[:, :, rows], got[:, :, rows])
    check("scale_filter_row", "B{} N{}".format(B, N), res[:, :, n], out[:, :, n], bar[:, :, n])


# ------------------------------------------------------------------------------- scale restoration
def _ref_ids(N):
    return sorted({0, 1, N - 1})


@pytest.mark.parametrize("N", [2, 3, 4, 8, 9, 16])
def test_projection_back(N):
    """projection_back_filter with and without scale_out, projection_back_scale against it on
    consistent data (Y = W X: the least-squares scale is row ref of W^-1) within both bars, a singular
    bin counted once in info.  The filters are Q1 diag(s) Q2 (kappa <= 256 that is no row scaling)."""
    _, dv, _, ops = _mods()
    B, F, T = 2, 17, 6 * N
    W = sr.gen_conditioned(1100 + N, B, F, N, 2)
    rng = np.random.default_rng(1100 + N)
    X = rng.standard_normal((B, N, F, T)) + 1j * rng.standard_normal((B, N, F, T))
    Y = sr._f64(pr.separate(X, W)[0])
    XY, YY = (sr._f64(pr.cross_covariance(a, b)[0]) for a, b in ((X, Y), (Y, Y)))
    for ref_id in _ref_ids(N):
        route = "{} N{} ref{}".format(form(N), N, ref_id)
        Wn, s, k = sr.projection_back_filter(W, ref_id)
        W64, s64, _ = sr.projection_back_filter(W, ref_id, dtype=np.float64)
        e64 = max(sr.normwise(s64, s, k, -1), sr.normwise(W64, Wn, k, (-2, -1)))
        c = sr.yardstick(e64)
        extra = "(c_f64 {:.3f}, kappa max {:.1f})".format(e64, float(k.max()))
        info = dv.zeros((1,), dv.i32)
        o = Out(W.shape, True, fill=W)
        ops.projection_back_filter(o.t, ref_id, info=info)
        record("projection_back_filter", route, sr.normwise(o.get(), Wn, k, (-2, -1)), c, extra)
        o, og = Out(W.shape, True, fill=W), Out(W.shape, True)
        ops.projection_back_filter(o.t, ref_id, info=info, scale_out=og.t)
        gs = og.get()
        record("projection_back_filter_scale_out", route,
               max(sr.normwise(o.get(), Wn, k, (-2, -1)),
                   sr.normwise(np.einsum("bfnn->bfn", gs), s, k, -1)), c, extra)
        off = ~np.eye(N, dtype=bool)
        assert np.all(gs[:, :, off] == 0)
        s2, k2 = sr.projection_back_scale(XY, YY, ref_id)
        e64b = sr.normwise(sr.projection_back_scale(XY, YY, ref_id, dtype=np.float64)[0], s2, k2, -1)
        c2 = sr.yardstick(e64b)
        og2 = Out(W.shape, True)
        ops.projection_back_scale(up(XY), up(YY), ref_id, info=info, out=og2.t)
        gs2 = og2.get()
        assert np.all(gs2[:, :, off] == 0)
        d2 = np.einsum("bfnn->bfn", gs2)
        record("projection_back_scale", route, sr.normwise(d2, s2, k2, -1), c2,
               "(c_f64 {:.3f}, kappa max {:.1f})".format(e64b, float(k2.max())))
        # the two routes on consistent data: |s_filter - s_scale| within both bars, each around its
        # own reference, plus what separates the references (the rounding of Y, XY, YY: the second
        # reference's own distance from the first)
        nrm = lambda a: np.sqrt((np.abs(a) ** 2).sum(axis=-1))  # noqa: E731
        both = pr.U * (c * k * nrm(s) + c2 * k2 * nrm(s2)) + nrm(s2 - s)
        record("projection_back_scale_vs_filter", route,
               float(np.max(nrm(d2.astype(np.clongdouble) - np.einsum("bfnn->bfn", gs)) / both)), 1.0)
        assert int(info.item()) == 0
    Ws = W.copy()
    Ws[1, 3, 0, :] = 0
    info = dv.zeros((1,), dv.i32)
    ops.projection_back_filter(Out(W.shape, True, fill=Ws).t, 0, info=info)
    assert int(info.item()) == 1
    YYs = YY.copy()
    YYs[0, 2, N - 1, :] = 0
    YYs[0, 2, :, N - 1] = 0
    ops.projection_back_scale(up(XY), up(YYs), 0, info=info, out=Out(W.shape, True).t)
    assert int(info.item()) == 2


@pytest.mark.parametrize("N", [2, 3, 4, 8, 9, 16])
def test_mdp_scale_and_scale_basis(N):
    _, dv, _, ops = _mods()
    B, F, T, K = 2, 17, 33, 5
    X, W = pr.gen_spectrogram(1200 + N, B, N, F, T) * 2.0 ** -8, pr.gen_filters(1200 + N, B, F, N, 2)
    Y = sr._f64(pr.separate(X, W)[0])
    YX, YY = (sr._f64(pr.cross_covariance(a, b)[0]) for a, b in ((Y, X), (Y, Y)))
    basis = pr.gen_nmf(1200 + N, B, N, F, T, K)[0]
    for ref_id in _ref_ids(N):
        G, bar = sr.mdp_scale(YX, YY, ref_id)
        o = Out(G.shape, True)
        ops.mdp_scale(up(YX), up(YY), ref_id, out=o.t)
        got = o.get()
        check("mdp_scale", "N{} ref{}".format(N, ref_id), got, G, bar)
        for domain in (1.0, 2.0):
            out, bar = sr.ilrma_scale_basis(basis, got, domain)
            ob = Out(basis.shape, fill=basis)
            ops.ilrma_scale_basis(ob.t, o.t, domain)
            check("ilrma_scale_basis", "N{} domain{}".format(N, domain), ob.get(), out, bar)


@pytest.mark.parametrize("N", [2, 3, 4, 8, 9, 16])
def test_demix_from_covariance(N):
    """YX = W XX of a known W, XX the covariance of x = A z with a mixing A = Q1 diag(s) Q2, s over
    2^-4..2^4 (kappa(XX) up to 1e6, none of it a diagonal scaling, which kappa_2 would overstate): the
    kernel's W against the restatement's, which itself is the known W within the same bar; a singular
    XX counted in info."""
    _, dv, _, ops = _mods()
    B, F, T = 2, 17, 8 * N
    rng = np.random.default_rng(1300 + N)
    Z = rng.standard_normal((B, N, F, T)) + 1j * rng.standard_normal((B, N, F, T))
    X = sr._f64(pr.separate(Z, sr.gen_conditioned(1300 + N, B, F, N, 4))[0])
    W = pr.gen_filters(1300 + N, B, F, N, 2)
    XXl = pr.cross_covariance(X, X)[0]
    XX = sr._f64(XXl)
    YX = sr._f64(np.einsum("bfac,bfcd->bfad", W.astype(np.clongdouble), XX.astype(np.clongdouble)))
    Wd, k = sr.demix_from_covariance(YX, XX)
    assert 1e3 < k.max() <= 1e6
    e64 = sr.normwise(sr.demix_from_covariance(YX, XX, dtype=np.float64)[0], Wd, k, (-2, -1))
    c = sr.yardstick(e64)
    assert sr.normwise(W, Wd, k, (-2, -1)) <= c  # the known W, up to the rounding of YX
    info = dv.zeros((1,), dv.i32)
    o = Out(W.shape, True)
    ops.demix_from_covariance(up(YX), up(XX), info=info, out=o.t)
    record("demix_from_covariance", "{} N{}".format(form(N), N), sr.normwise(o.get(), Wd, k, (-2, -1)),
           c, "(c_f64 {:.3f}, kappa max {:.1f})".format(e64, float(k.max())))
    assert int(info.item()) == 0
    XXs = XX.copy()
    XXs[1, 4, 0, :] = 0
    XXs[1, 4, :, 0] = 0
    ops.demix_from_covariance(up(YX), up(XXs), info=info, out=Out(W.shape, True).t)
    assert int(info.item()) == 1


# ------------------------------------------------------------------------------- profile
def _write_profile(raw, path):
    worst = {}
    for line in open(raw):
        f = line.rstrip("\n").split("\t")
        key = (f[0], f[1])
        if key not in worst or float(f[4]) > float(worst[key][4]):
            worst[key] = f
    with open(path, "w") as out:
        out.write("# largest measured error of every entry point and route, tests/test_gpu_spatial_pass_"
                  "elementwise.py on an MI355X\n# elementwise entries: error and bar in u = 2^-53 of the "
                  "reference value at the worst element; normwise entries (c_f64 given): error and bar "
                  "c = 8 c_f64\n# in units of g u |ref| per bin, c_f64 the float64 restatement's own "
                  "error in the same units; ratio = error / bar\n")
        for key in sorted(worst):
            f = worst[key]
            out.write("{:36s} {:58s} err {:>10s}  bar {:>10s}  ratio {}{}\n".format(
                f[0], f[1], f[2], f[3], f[4], "  " + f[5] if len(f) > 5 and f[5] else ""))


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles")
    raw = os.path.join(out_dir, "spatial_pass_elementwise.raw")
    if os.path.exists(raw):
        os.remove(raw)
    os.environ["SSSPY_PASS_PROFILE_RAW"] = raw
    rc = pytest.main([os.path.abspath(__file__), "-m", "gpu", "-q", "--maxfail=40", "--durations=8"]
                     + sys.argv[2:])
    if os.path.exists(raw):
        _write_profile(raw, os.path.join(out_dir, "spatial_pass_elementwise.txt"))
        os.remove(raw)
    sys.exit(int(rc))
