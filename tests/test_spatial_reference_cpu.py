"""The restatement of tests/spatial_reference.py checked on the CPU: (1) its float64 run meets its own
bars, (2) it agrees with oracle/spatial.py -- the project's restatement of the reference functions,
itself pinned to the reference by the committed fixtures -- on small inputs, (3) every deliberate
mistake (`mutant`) breaks at least one bar.  No GPU."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pass_reference as pr  # noqa: E402
import spatial_reference as sr  # noqa: E402
from oracle import spatial as osp  # noqa: E402

LD = pr.LD
MAXF, ADDF, NOF = (pr.FLOOR_MAX, pr.EPS), (pr.FLOOR_ADD, pr.EPS), (pr.FLOOR_NONE, 0.0)
OFLOOR = {pr.FLOOR_MAX: ("max", pr.EPS), pr.FLOOR_ADD: ("add", pr.EPS), pr.FLOOR_NONE: ("none", 0.0)}


def elementwise(got, ref, bar):
    err = np.abs(np.asarray(got).astype(ref.dtype) - ref)
    bar = np.asarray(bar, dtype=LD)
    assert np.all(err[bar <= 0] == 0)
    return float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1), 0)))


def pairs_of(N):
    from ssspy_amd.utils.select_pair import (combination_pair_selector, resolve_pairs,
                                             sequential_pair_selector)

    return {"seq": resolve_pairs(sequential_pair_selector, N),
            "iss2": resolve_pairs(lambda n: sequential_pair_selector(n, stop=n, step=2), N),
            "comb": resolve_pairs(combination_pair_selector, N)}


# ------------------------------------------------------------------ (1) float64 against its own bars
@pytest.mark.parametrize("kind", [sr.FRAME, sr.BIN_FRAME])
@pytest.mark.parametrize("flooring", [NOF, MAXF, ADDF])
@pytest.mark.parametrize("N,T", [(2, 17), (3, 65), (5, 40), (8, 33)])
def test_fused_iss1_float64_meets_its_bars(N, T, flooring, kind):
    B, F = 2, 3
    Y, w = sr.gen_iss_inputs(N * 100 + T, B, N, F, T, kind)
    ref = sr.iss1_fused(Y, w, kind, flooring)
    f64 = sr.iss1_fused(Y, w, kind, flooring, dtype=np.float64)
    e = sr.normwise(f64["Y"], ref["Y"], ref["g"], -1)
    c = sr.yardstick(e)
    print("iss1_fused N{} T{}: float64 error {:.3f} g u, g max {:.1f}".format(N, T, e, ref["g"].max()))
    assert e <= c and e < 64, "the growth factor does not explain the float64 error"
    # plain sums: frame powers of a given Y, the log-determinant increment
    r2, bar = sr.frame_power_of(f64["Y"])
    r64, _ = sr.frame_power_of(f64["Y"], dtype=np.float64)
    print("  r2_next error / bar {:.3f}".format(elementwise(r64, r2, bar)))
    assert elementwise(r64, r2, bar) <= 1
    ld0 = np.array([3.5, -20.25])
    val, lbar = sr.iss1_logdet(ref, ld0, c, T, F)
    v64, _ = sr.iss1_logdet(f64, ld0, c, T, F, dtype=np.float64)
    print("  logdet error / bar {:.3f}".format(elementwise(v64, val, lbar)))
    assert elementwise(v64, val, lbar) <= 1


@pytest.mark.parametrize("N", [2, 3, 4, 5, 8, 9])
def test_transforms_float64_meet_their_bars(N):
    B, F, T = 1, 5, 6 * N
    Y, w = sr.gen_iss_inputs(200 + N, B, N, F, T, sr.BIN_FRAME, tiny_bin=False)
    Vc = sr._f64(sr.iss_statistics(Y, w, sr.BIN_FRAME))
    G, g = sr.iss1_transform(Vc, MAXF)
    e = sr.normwise(sr.iss1_transform(Vc, MAXF, dtype=np.float64)[0], G, g, (-2, -1))
    print("iss1_transform N{}: float64 error {:.3f} g u, g max {:.1f}".format(N, e, g.max()))
    assert e < 64
    # the transform applied to Y is the fused sweep: within the sum of both bars
    fused = sr.iss1_fused(Y, w, sr.BIN_FRAME, MAXF)
    Yt, _ = pr.separate(Y, sr._f64(G))
    assert sr.normwise(Yt, fused["Y"], fused["g"] * g.T[:, None, :], -1) < 64 * N
    for name, pairs in pairs_of(N).items():
        G2, g2, _ = sr.iss2_transform(Vc, pairs, MAXF)
        G64 = sr.iss2_transform(Vc, pairs, MAXF, dtype=np.float64)[0]
        rows = sorted({r for p in pairs for r in p})
        e = sr.normwise(sr.align_phase(G64, G2, rows), G2, g2, (-2, -1))
        print("iss2_transform N{} {}: float64 error {:.3f} g u, g max {:.1f}".format(
            N, name, e, g2.max()))
        assert e < 64


@pytest.mark.parametrize("N", [2, 3, 5, 9])
@pytest.mark.parametrize("pair_only", [0, 1])
def test_ip2_float64_meets_its_bars(N, pair_only):
    B, F = 1, 9
    W, Uc = sr.gen_ip2_inputs(300 + N, B, F, N, n_sets=2 if pair_only else None, log2_cond=8)
    plist = [[(N - 1, 0)]] if pair_only else [[(0, 1)], pairs_of(N)["seq"]]
    for pairs in plist:
        ref, g, _ = sr.update_by_ip2(W, Uc, pairs, MAXF, pair_only)
        f64, _, _ = sr.update_by_ip2(W, Uc, pairs, MAXF, pair_only, dtype=np.float64)
        e = sr.normwise(sr.align_phase(f64, ref), ref, g[..., None], -1)
        print("update_by_ip2 N{} pair_only{} {} pair(s): float64 error {:.3f} g u, g max {:.1f}".format(
            N, pair_only, len(pairs), e, g.max()))
        assert e < 64


@pytest.mark.parametrize("N", [2, 4, 9])
def test_scale_restoration_float64_meets_its_bars(N):
    B, F, T = 1, 7, 5 * N
    W = pr.gen_filters(400 + N, B, F, N, 2)
    for ref_id in (0, N - 1):
        Wn, s, k = sr.projection_back_filter(W, ref_id)
        W64, s64, _ = sr.projection_back_filter(W, ref_id, dtype=np.float64)
        assert sr.normwise(s64, s, k, -1) < 64 and sr.normwise(W64, Wn, k, (-2, -1)) < 64
    X = pr.gen_spectrogram(401 + N, B, N, F, T) * 2.0 ** -10
    Y, _ = pr.separate(X, W)
    Y = sr._f64(Y)
    XY, YY, YX, XX = (sr._f64(pr.cross_covariance(a, b)[0]) for a, b in ((X, Y), (Y, Y), (Y, X), (X, X)))
    s, k = sr.projection_back_scale(XY, YY, 0)
    assert sr.normwise(sr.projection_back_scale(XY, YY, 0, dtype=np.float64)[0], s, k, -1) < 64
    Wd, k = sr.demix_from_covariance(YX, XX)
    assert sr.normwise(sr.demix_from_covariance(YX, XX, dtype=np.float64)[0], Wd, k, (-2, -1)) < 64
    G, bar = sr.mdp_scale(YX, YY, 0)
    assert elementwise(sr.mdp_scale(YX, YY, 0, dtype=np.float64)[0], G, bar) <= 1
    basis = pr.gen_nmf(402, B, N, F, T, 3)[0]
    for domain in (1.0, 2.0):
        out, bar = sr.ilrma_scale_basis(basis, sr._f64(G), domain)
        o64, _ = sr.ilrma_scale_basis(basis, sr._f64(G), domain, dtype=np.float64)
        assert elementwise(o64, out, bar) <= 1
    d = np.exp2(np.random.default_rng(N).uniform(-20, 20, (B, F)))
    out, bar = sr.scale_filter_row(W, d, N - 1)
    assert elementwise(sr.scale_filter_row(W, d, N - 1, dtype=np.float64)[0], out, bar) <= 1


# ------------------------------------------------------------------ (2) against the oracle
@pytest.mark.parametrize("flooring", [NOF, MAXF, ADDF])
@pytest.mark.parametrize("N", [2, 3, 5])
def test_restatement_equals_the_oracle(N, flooring):
    """oracle/spatial.py follows the reference line by line in float64 (one mixture); the extended
    run must agree to float64 accuracy: 1e-9 relative in norm is far above the rounding of these
    well-conditioned inputs and far below any of the mistakes of part (3)."""
    F, T = 4, 7 * N
    of = OFLOOR[flooring[0]]
    Y, w = sr.gen_iss_inputs(500 + N, 1, N, F, T, sr.BIN_FRAME)

    def close(a, b):
        a, b = sr._f64(a), np.asarray(b)
        assert np.linalg.norm(a - b) <= 1e-9 * np.linalg.norm(b)

    close(sr.iss1_fused(Y, w, sr.BIN_FRAME, flooring)["Y"][0], osp.update_by_iss1(Y[0], w[0], of))
    Vc = sr._f64(sr.iss_statistics(Y, w, sr.BIN_FRAME))
    close(pr.separate(Y, sr._f64(sr.iss1_transform(Vc, flooring)[0]))[0][0],
          osp.update_by_iss1(Y[0], w[0], of))
    for pairs in pairs_of(N).values():
        G = sr.iss2_transform(Vc, pairs, flooring)[0]
        Yo = osp.update_by_iss2(Y[0], w[0], of, pairs)
        Yg = sr._f64(pr.separate(Y, sr._f64(G))[0][0])
        close(sr.align_phase(Yg, Yo.astype(np.clongdouble)), Yo)  # (a phase per source and bin)
        W, Uc = sr.gen_ip2_inputs(510 + N, 1, F, N)
        Wo = osp.update_by_ip2(W[0], Uc[0], of, pairs)
        Wr = sr.update_by_ip2(W, Uc, pairs, flooring)[0]
        close(sr.align_phase(Wr, Wo[None].astype(np.clongdouble)), Wo[None])
    W, Uc = sr.gen_ip2_inputs(520 + N, 1, F, N)
    Wo = osp.update_by_ip1(W[0], Uc[0], of)
    Wr = W.copy()
    for n in range(N):
        Wr, d, _ = sr.ip1_source_solve(Wr, Uc, n)
        Wr = sr._f64(sr.scale_filter_row(sr._f64(Wr), sr._f64(pr.floor(d, flooring)), n)[0])
    close(Wr[0], Wo)
    close(sr.projection_back_filter(W, N - 1)[0][0], osp.projection_back_filter(W[0], N - 1))
    X = pr.gen_spectrogram(530 + N, 1, N, F, T) * 2.0 ** -10
    Yd = sr._f64(pr.separate(X, W)[0])
    XY, YY, YX, XX = (sr._f64(pr.cross_covariance(a, b)[0]) for a, b in ((X, Yd), (Yd, Yd), (Yd, X), (X, X)))
    for ref_id in (0, N - 1):
        s = sr.projection_back_scale(XY, YY, ref_id)[0]
        close(pr.separate(Yd, sr._f64(sr.diag_of(s)))[0][0], osp.projection_back_output(Yd[0], X[0], ref_id))
        Gm = sr.mdp_scale(YX, YY, ref_id)[0]
        close(pr.separate(Yd, sr._f64(Gm))[0][0], osp.minimal_distortion_output(Yd[0], X[0], ref_id))
    close(sr.demix_from_covariance(YX, XX)[0][0], osp.demix_from_output(Yd[0], X[0]))


# ------------------------------------------------------------------ (3) mutants
def _fused_case(flooring=MAXF, kind=sr.BIN_FRAME):
    N, T = 5, 257
    Y, w = sr.gen_iss_inputs(600, 2, N, 3, T, kind)
    ref = sr.iss1_fused(Y, w, kind, flooring)
    c = sr.yardstick(sr.normwise(sr.iss1_fused(Y, w, kind, flooring, dtype=np.float64)["Y"], ref["Y"],
                                 ref["g"], -1))
    return Y, w, ref, c, T


@pytest.mark.parametrize("mutant", ["no_conj", "weight_n", "one_minus_inv", "drop_last_frame",
                                    "drop_last_bin"])
def test_fused_iss1_mutants_are_caught(mutant):
    Y, w, ref, c, _ = _fused_case()
    bad = sr.iss1_fused(Y, w, sr.BIN_FRAME, MAXF, mutant=mutant)
    e = sr.normwise(bad["Y"], ref["Y"], ref["g"], -1)
    print("{}: {:.3g} g u against c = {:.3f}".format(mutant, e, c))
    assert e > c


@pytest.mark.parametrize("mutant", ["logdet_sign", "logdet_half"])
def test_logdet_mutants_are_caught(mutant):
    _, _, ref, c, T = _fused_case()
    ld0 = np.array([1.5, -2.5])
    val, bar = sr.iss1_logdet(ref, ld0, c, T, 3)
    bad, _ = sr.iss1_logdet(ref, ld0, c, T, 3, mutant=mutant)
    assert elementwise(bad, val, bar) > 1
    # overwriting instead of adding: the incoming value is part of the result
    assert elementwise(val - ld0, val, bar) > 1


@pytest.mark.parametrize("mutant", ["no_conj", "weight_n", "one_minus_inv"])
def test_iss1_transform_mutants_are_caught(mutant):
    N = 4
    Y, w = sr.gen_iss_inputs(610, 1, N, 5, 24, sr.BIN_FRAME, tiny_bin=False)
    Vc = sr._f64(sr.iss_statistics(Y, w, sr.BIN_FRAME))
    G, g = sr.iss1_transform(Vc, MAXF)
    c = sr.yardstick(sr.normwise(sr.iss1_transform(Vc, MAXF, dtype=np.float64)[0], G, g, (-2, -1)))
    assert sr.normwise(sr.iss1_transform(Vc, MAXF, mutant=mutant)[0], G, g, (-2, -1)) > c


@pytest.mark.parametrize("mutant,flooring,pair_only,pairs",
                         [("floor_q", ADDF, 0, [(0, 1)]), ("floor_q", MAXF, 0, [(0, 1)]),
                          ("swap_eigenvectors", MAXF, 0, [(0, 1), (1, 2)]),
                          ("pair_only_by_source", MAXF, 1, [(1, 2)])])
def test_ip2_mutants_are_caught(mutant, flooring, pair_only, pairs):
    N, B, F = 3, 1, 6
    W, Uc = sr.gen_ip2_inputs(620, B, F, N, n_sets=2 if pair_only else None)
    if mutant == "floor_q":
        Uc[:, 0, 0] *= 1e26  # P^H U P goes with 1 / U: lamb = 1e-26-ish in the first bin, sqrt(q) below eps
    ref, g, _ = sr.update_by_ip2(W, Uc, pairs, flooring, pair_only)
    f64 = sr.update_by_ip2(W, Uc, pairs, flooring, pair_only, dtype=np.float64)[0]
    c = sr.yardstick(sr.normwise(sr.align_phase(f64, ref), ref, g[..., None], -1))
    bad = sr.update_by_ip2(W, Uc, pairs, flooring, pair_only, mutant=mutant)[0]
    e = sr.normwise(sr.align_phase(bad, ref), ref, g[..., None], -1)
    print("{}: {:.3g} g u against c = {:.3f}".format(mutant, e, c))
    assert e > c


def test_scale_restoration_mutants_are_caught():
    N, B, F = 3, 1, 5
    W = pr.gen_filters(630, B, F, N, 2)
    Wn, s, k = sr.projection_back_filter(W, 1)
    c = sr.yardstick(sr.normwise(sr.projection_back_filter(W, 1, dtype=np.float64)[1], s, k, -1))
    assert sr.normwise(sr.projection_back_filter(W, 1, mutant="pb_column")[1], s, k, -1) > c
    X = pr.gen_spectrogram(631, B, N, F, 12) * 2.0 ** -10
    Y = sr._f64(pr.separate(X, W)[0])
    YX, YY = sr._f64(pr.cross_covariance(Y, X)[0]), sr._f64(pr.cross_covariance(Y, Y)[0])
    G, bar = sr.mdp_scale(YX, YY, 1)
    assert elementwise(sr.mdp_scale(YX, YY, 1, mutant="mdp_no_conj")[0], G, bar) > 1
