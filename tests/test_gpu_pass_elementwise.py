"""Every ILRMA / AuxIVA hot-path entry point alone, element by element, against the extended-precision
restatement of tests/pass_reference.py.

The bars are those the reference functions derive (see the module docstring of pass_reference.py for
the rules): each is ``m u companion`` per element, u = 2^-53, nothing fitted to a measurement and no
element left out.  In short, for the passes here:

* basis pass: num and den are sums of T terms, each term carrying its own budget -- R = T V: K + 1;
  1 / R by rcp_nr: + 2; Gauss a = P / R^2: P's budget + 2 (K + 1) + 3; the t and GGD factors as
  `_mm_terms` spells out, a power through exp2(e log2 x) counting (2 |e log2 x| + 4) -- so
  rel(num) = T + 1 + weighted mean of the term budgets, likewise den with K + 3; the update is
  old (num / den)^expo: expo (rel num + rel den + 2) + 3 (+ 1 under the ADD floor).  At K = 16,
  T = 64, Gauss, no filter: 0.5 (65 + 2 + 37 + 65 + 19 + 2) + 3 = 98 u.
* activation pass: the same with sums of F terms.
* with a filter P = |W x|^2 loses what y = W x cancels: 6 N u S |y| + 2 u P, S = sum |w| |x|; the
  term budget then holds 6 N S / |y| of that element (data dependent, a few hundred u at worst for
  the unitary-times-diagonal filters generated here).
* covariances: (T + 6) u A_ac, A_ac = (1/T) sum_j w |x_a| |x_c|, plus the weights' budgets.
* losses are absolute: (n + budget) u on the data sum, ((n + 4) max(1, sum |log R|) + n (K + 1)) u
  on the log part, n = N F T.
* IP1 is a solve: per bin ||w - w_ref|| <= c kappa u ||w_ref||, kappa = max_n kappa_2(W U_n) from
  the extended-precision inverse, c = 8 x the largest kappa-normalised error np.linalg.solve makes in
  float64 on the same inputs (both numbers are printed and go to the profile).

Routes.  Each ILRMA case asserts ssspy_ilrma_route for its shape.  The shared and IVA operators have
no such query; their launchers branch on the source count alone -- per-N kernels at 2..4, the
matrix-core covariance of wide_cov.hip at 5..8 sources (weighted_covariance), the per-N kernels at
5..8 elsewhere, the run-time-N kernels of wide_n.hip at 9..16 -- and ssspy_iva_frame_power on
(T, B): a thread per frame when ceil(T / 256) B >= 128 (B = 128 here), four waves sharing the bins
below, with bin chunks folded whenever 1024 / (ceil(T / 64) B) > 1 (every small case).  The cases
name the branch they reach.  Frame splits of the throughput basis pass are chosen by the tail plan,
which ssspy_ilrma_route reports: the cases assert unsplit only, split only, and both in one launch.

Run as a script on the GPU to rewrite profiles/pass_elementwise.txt.
"""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pass_reference as pr  # noqa: E402

pytestmark = pytest.mark.gpu

LD = pr.LD
MAXF, ADDF, NOF = (pr.FLOOR_MAX, pr.EPS), (pr.FLOOR_ADD, pr.EPS), (pr.FLOOR_NONE, 0.0)
ROUTE_NAMES = ["latency", "throughput", "grouped", "generic", "wide_basis", "runtime_n"]
LAT, THR, GRP, GEN, WIDE, RTN = range(6)
G2 = ((pr.GAUSS, 0.0), 2.0)  # (model, domain)
K17_CHUNKED = (90, 4, 65, 16)  # (B, N, F, T): 450 bin tiles, 180 activation blocks per chunk
MODELS = [((pr.GAUSS, 0.0), 2.0), ((pr.GAUSS | pr.ME, 0.0), 2.0), ((pr.GAUSS, 0.0), 1.0),
          ((pr.GAUSS, 0.0), 1.3), ((pr.TMODEL, 3.0), 2.0), ((pr.GGD, 1.0), 2.0),
          ((pr.GGD, 0.5), 2.0), ((pr.GGD, 1.2), 2.0)]


# ------------------------------------------------------------------------------- device plumbing
def _mods():
    import torch

    from ssspy_amd import _device as dv
    from ssspy_amd import _lib, _ops

    return torch, dv, _lib, _ops


def up(a):
    """Upload with a NaN band behind the data in the same allocation."""
    torch, dv, _, _ = _mods()
    a = np.ascontiguousarray(a)
    flat, n = pr.with_nan_band(a)
    t = dv.to_device(flat)
    v = t[:n]
    if np.iscomplexobj(a):
        v = v.view(torch.complex128)
    v = v.view(a.shape)
    v._keep = t
    return v


class Out:
    """An output (or in-place) tensor between two sentinel bands."""

    def __init__(self, shape, cplx=False, fill=None):
        torch, dv, _, _ = _mods()
        self.shape, self.cplx = tuple(shape), cplx
        self.n = int(np.prod(shape)) * (2 if cplx else 1)
        self.buf = dv.to_device(pr.sentinel_buffer(self.n, fill))
        v = self.buf[pr.BAND:pr.BAND + self.n]
        self.t = (v.view(torch.complex128) if cplx else v).view(self.shape)

    def get(self):
        _, dv, _, _ops = _mods()
        host = np.array(dv.to_host(self.buf))
        assert pr.bands_intact(host), "a kernel wrote outside its output"
        _ops.check_workspace_canaries()
        pay = host[pr.BAND:pr.BAND + self.n]
        return (pay.view(np.complex128) if self.cplx else pay).reshape(self.shape)


def check(entry, route, got, ref, bar):
    """Elementwise over the whole output: |got - ref| <= bar, every element finite."""
    got = np.asarray(got)
    assert np.all(np.isfinite(got)), "{} [{}]: non-finite output".format(entry, route)
    ref, bar = np.asarray(ref), np.asarray(bar, dtype=LD)
    err = np.abs(got.astype(ref.dtype) - ref)
    assert np.all(bar > 0) or np.all(err[bar <= 0] == 0)
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1), 0)
    k = np.unravel_index(np.argmax(ratio), ratio.shape) if ratio.ndim else ()
    scale = pr.U * max(float(np.abs(ref[k])), 1e-300)
    line = "{}\t{}\t{:.2f}\t{:.2f}\t{:.4f}".format(entry, route, float(err[k]) / scale,
                                                   float(bar[k]) / scale, float(ratio[k]))
    print(line)
    path = os.environ.get("SSSPY_PASS_PROFILE_RAW")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    assert float(ratio[k]) <= 1.0, "{} [{}]: error / bar = {:.3f} at {}".format(
        entry, route, float(ratio[k]), k)


# ------------------------------------------------------------------------------- shared operators
@pytest.mark.parametrize("N", [2, 3, 4, 5, 8, 9, 16])
def test_separate_and_compose(N):
    """separate (out of place and in place), compose_filters.  Per-N kernels to 8 sources, the
    run-time-N kernels of wide_n.hip at 9 and 16.  T = 65: a second 64-frame block of one frame.
    At 9 and 16 sources also T = 257 and 300: k_separate_rt puts 256 threads along the frames, so
    these take a second trip of its frame loop (of one frame, and of 44)."""
    _, dv, _, ops = _mods()
    B, F = 2, 17
    W = pr.gen_filters(10 + N, B, F, N)
    for T in (65,) + ((257, 300) if N > 8 else ()):
        tag = "N={}".format(N) if T == 65 else "N={},T={}".format(N, T)
        X = pr.gen_spectrogram(10 + N + (0 if T == 65 else T), B, N, F, T)
        Y, bar = pr.separate(X, W)
        o = Out(X.shape, True)
        ops.separate(up(X), up(W), out=o.t)
        check("separate", tag, o.get(), Y, bar)
        o = Out(X.shape, True, fill=X)
        ops.separate(o.t, up(W), out=o.t)
        check("separate_inplace", tag, o.get(), Y, bar)
    G = pr.gen_filters(40 + N, B, F, N, 2)
    ref, bar = pr.compose_filters(G, W)
    o = Out(W.shape, True)
    ops.compose_filters(up(G), up(W), o.t)
    check("compose_filters", "N={}".format(N), o.get(), ref, bar)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("N,T", [(2, 17), (3, 64), (4, 65), (5, 40), (8, 16), (9, 17), (16, 33),
                                 (9, 65), (16, 97)])
def test_weighted_covariance(N, T, kind):
    """UNIT / FRAME / BIN_FRAME with S = 1 and S = N: per-N kernels (2..4), wide_cov.hip (5..8,
    falling back to the per-N kernel where it declines the shape), wide_n.hip (9, 16).  (9, 65) and
    (16, 97) walk three and four 32-frame LDS tiles of k_cov_rt, the last of 1 frame."""
    _, dv, _, ops = _mods()
    B, F = 2, 17
    X = pr.gen_spectrogram(20 + N, B, N, F, T)
    for S in ((1,) if kind == 0 else (1, N)):  # (UNIT is one weight set by definition)
        w = None if kind == 0 else pr.gen_weights(21 + N, (B, S, T) if kind == 1 else (B, S, F, T))
        ref, bar = pr.weighted_covariance(X, w, kind, S)
        o = Out((B, F, S, N, N), True)
        ops.weighted_covariance(up(X), None if w is None else up(w), kind, S, out=o.t)
        nt = "N={},T={}".format(N, T) if (N, T) in ((9, 65), (16, 97)) else "N={}".format(N)
        check("weighted_covariance_kind{}".format(kind), "{} S={}".format(nt, S), o.get(), ref, bar)


WIDE_COV_T = (1, 7, 8, 9, 15, 17, 63, 64, 65, 71, 129)
KIND_NAMES = ["unit", "frame", "bin_frame"]


def _wide_cov_weights(seed, kind, B, S, F, T):
    return None if kind == 0 else pr.gen_weights(seed, (B, S, T) if kind == 1 else (B, S, F, T))


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("N", [6, 7, 8])
def test_wide_cov_frames_sets_and_channels(N, kind):
    """k_wide_cov of wide_cov.hip alone (6..8 channels, at most 8 weight sets, a mixture below 4 GiB:
    wide_weighted_cov_ok takes every shape here).  B F = 10 items are three workgroups, the last with
    two live waves.  The frames walk in slabs of 8 through a ring of 8 slabs and 4 weight pairs:
    T = 1..9 one or two slabs (every refill clamped), 15 and 17 a tail of 7 and of 1, 63..65 the
    eighth slab short, full, and a second trip of the ring that holds one frame, 71 and 129 a ninth
    and a seventeenth slab of 7 and of 1 (three trips; odd and even numbers of slab pairs; the weight
    patch's two halves in turn).  S = 1, 3, N are the instances launch<1>, <3>, <6..8>; N = 6 and 7
    leave tile rows to the descriptor's range check."""
    _, dv, _, ops = _mods()
    B, F = 2, 5
    for T in WIDE_COV_T:
        X = pr.gen_spectrogram(200 + 10 * N + T, B, N, F, T)
        for S in ((1,) if kind == 0 else (1, 3, N)):
            w = _wide_cov_weights(201 + N + T + S, kind, B, S, F, T)
            ref, bar = pr.weighted_covariance(X, w, kind, S)
            o = Out((B, F, S, N, N), True)
            ops.weighted_covariance(up(X), None if w is None else up(w), kind, S, out=o.t)
            check("wide_cov_" + KIND_NAMES[kind], "N={},S={} T={}".format(N, S, T), o.get(), ref, bar)


def _narrow_spectrogram(seed, B, N, F, T):
    """unit-variance columns with magnitudes over 1/2..2: every frame carries weight in every entry
    of its covariance, so a frame that went missing is a gross error in all of them."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((B, N, F, T)) + 1j * rng.standard_normal((B, N, F, T))) \
        * np.exp2(rng.uniform(-1, 1, (B, N, F, T)))
    return X.astype(np.complex128)


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("T", [9, 65])
def test_wide_cov_nonfinite_neighbour(T, kind):
    """The tail slab of a row of 9 or 65 frames is loaded whole: 7 frames of it are the first frames
    of the row behind -- the same channel's next bin for the samples; the next set (FRAME) or the next
    bin of the set (BIN_FRAME) for the weights.  One sample and one weight there are Inf.  The bins and
    sets in front of them must come out finite and within the bar (a masked weight alone would leave
    0 * Inf), the poisoned bin and set themselves non-finite (so the Inf did reach the device)."""
    _, dv, _, ops = _mods()
    B, N, F = 2, 8, 5
    X = pr.gen_spectrogram(260 + T, B, N, F, T)
    for S in (3, N):
        w = _wide_cov_weights(261 + T + S, kind, B, S, F, T)
        ref, bar = pr.weighted_covariance(X, w, kind, S)  # (of the clean inputs: what is checked
        Xp, wp = X.copy(), w.copy()                        #  does not depend on the poisoned ones)
        Xp[0, 3, 2, 2] = np.inf   # read by the tail of (mixture 0, channel 3, bin 1)
        dirty = np.zeros((B, F, S), bool)
        dirty[0, 2, :] = True
        if kind == 1:
            wp[0, 1, 1] = np.inf  # read by the tail of set 0, every bin
            dirty[0, :, 1] = True
        else:
            wp[0, 1, 4, 1] = np.inf  # read by the tail of (set 1, bin 3)
            wp[0, 1, 0, 1] = np.inf  # read by the tail of (set 0, bin 4), across the sets
            dirty[0, 4, 1] = dirty[0, 0, 1] = True
        o = Out((B, F, S, N, N), True)
        ops.weighted_covariance(up(Xp), up(wp), kind, S, out=o.t)
        got = o.get()
        assert not np.any(np.isfinite(got[dirty][:, 3, 3])), "the Inf did not reach its own bin / set"
        check("wide_cov_" + KIND_NAMES[kind] + "_inf_neighbour", "N={},S={},T={}".format(N, S, T),
              got[~dirty], ref[~dirty], bar[~dirty])


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("T", [9, 65])
def test_wide_cov_last_weight(T, kind):
    """T odd: the last frame's weight of a mixture's last set is the first half of a 16-byte load
    whose second half lies past the mixture's weights (past the descriptor; mixture 1's weights also
    start 8 bytes off a 16-byte boundary, S T and S F T being odd).  That weight is 2^20 times the
    others, on samples of even magnitude: were the load dropped as a whole, every entry of the last
    set would be off by about its own size."""
    _, dv, _, ops = _mods()
    B, N, F, S = 2, 8, 5, 3
    X = _narrow_spectrogram(270 + T, B, N, F, T)
    rng = np.random.default_rng(271 + T + kind)
    w = np.exp2(rng.uniform(-1, 1, (B, S, T) if kind == 1 else (B, S, F, T)))
    w.reshape(B, -1)[:, -1] *= 2.0 ** 20
    ref, bar = pr.weighted_covariance(X, w, kind, S)
    # what that one frame contributes to the entries it reaches: at least 1e6 bars, in every one
    short = pr.weighted_covariance(X[..., :-1], w[..., :-1], kind, S)[0] * LD(T - 1) / LD(T)
    sel = (slice(None), -1 if kind == 2 else slice(None), -1)
    assert np.all(np.abs(ref - short)[sel] > 1e6 * bar[sel])
    o = Out((B, F, S, N, N), True)
    ops.weighted_covariance(up(X), up(w), kind, S, out=o.t)
    check("wide_cov_" + KIND_NAMES[kind] + "_last_weight", "N={},S={},T={}".format(N, S, T), o.get(),
          ref, bar)


@pytest.mark.parametrize("N", [2, 3, 4, 6, 9, 16])
def test_cross_covariance_and_congruence(N):
    """At 9 and 16 sources also T = 65 and 97: three and four 32-frame LDS tiles of k_cov_rt with
    both operands staged, the last tile of one frame."""
    _, dv, _, ops = _mods()
    B, F, T = 2, 17, 33
    for T2 in {9: (65,), 16: (97,)}.get(N, ()):
        X, Z = pr.gen_spectrogram(30 + N + T2, B, N, F, T2), pr.gen_spectrogram(31 + N + T2, B, N, F, T2)
        ref, bar = pr.cross_covariance(X, Z)
        o = Out((B, F, N, N), True)
        ops.cross_covariance(up(X), up(Z), out=o.t)
        check("cross_covariance", "N={},T={}".format(N, T2), o.get(), ref, bar)
    X, Z = pr.gen_spectrogram(30 + N, B, N, F, T), pr.gen_spectrogram(31 + N, B, N, F, T)
    ref, bar = pr.cross_covariance(X, Z)
    o = Out((B, F, N, N), True)
    ops.cross_covariance(up(X), up(Z), out=o.t)
    check("cross_covariance", "N={}".format(N), o.get(), ref, bar)
    G = pr.gen_filters(32 + N, B, F, N, 4)
    C1 = np.asarray(pr.cross_covariance(X, X)[0], dtype=np.complex128)
    CN = np.asarray(pr.weighted_covariance(X, pr.gen_weights(33, (B, N, T)), 1, N)[0],
                    dtype=np.complex128)
    for C, tag in ((C1, "S=1"), (CN, "S=N")):
        ref, bar = pr.covariance_congruence(C, G)
        o = Out(C.shape, True)
        ops.covariance_congruence(up(C), up(G), o.t)
        check("covariance_congruence", "N={} {}".format(N, tag), o.get(), ref, bar)


@pytest.mark.parametrize("N", [2, 3, 4, 7, 9, 16])
def test_sum_logdet(N):
    _, dv, _, ops = _mods()
    B, F = 3, 65
    W = pr.gen_filters(50 + N, B, F, N)
    ref, bar = pr.sum_logdet(W)
    o = Out((B,))
    ops.sum_logdet(up(W), out=o.t)
    check("sum_logdet", "N={}".format(N), o.get(), ref, bar)


@pytest.mark.parametrize("total,nslots", [(1, 1), (5, 2), (300, 17), (70, 260)])
def test_fold_scalar_slots(total, nslots):
    _, dv, _, ops = _mods()
    rng = np.random.default_rng(total + nslots)
    slots = rng.standard_normal((nslots, total)) * np.exp2(rng.uniform(-20, 20, (nslots, total)))
    ref, bar = pr.fold_scalar_slots(slots)
    o = Out((total,))
    ops.fold_scalar_slots(up(slots), total, nslots, o.t)
    check("fold_scalar_slots", "{}x{}".format(nslots, total), o.get(), ref, bar)


# ------------------------------------------------------------------------------- ILRMA passes
def _ilrma_passes(B, N, F, T, K, route, model=G2[0], domain=2.0, flooring=MAXF, chunks=None,
                  floor_inputs=False, seed=0, split=None, own_line=False):
    """basis, activation, loss, covariance and ISS weights of one shape, with and without a filter.
    own_line: the case keeps a line of its own per entry point in the profile (shape, model and floor
    join the route in the key) instead of counting towards its route's worst case."""
    _, dv, _, ops = _mods()
    got_route, got_chunks, plan = ops.ilrma_route(B, N, F, T, K, domain, model)
    assert got_route == route, "shape reaches {} instead of {}".format(
        ROUTE_NAMES[got_route], ROUTE_NAMES[route])
    print("route asserted: {} for B{} N{} F{} T{} K{} model {} domain {}".format(
        ROUTE_NAMES[route], B, N, F, T, K, model, domain))
    if chunks == "one":
        assert got_chunks == 1
    elif chunks == "many":
        assert got_chunks > 1
    # frame splits of the basis pass: (unsplit items, split items, chunks per split item)
    if split == "none":
        assert plan[0] > 0 and plan[1] == 0 and plan[2] == 1, plan
    elif split == "all":
        assert plan[0] == 0 and plan[1] > 0 and plan[2] > 1, plan
    elif split == "mixed":
        assert plan[0] > 0 and plan[1] > 0 and plan[2] > 1, plan
    tag = "{} B{} N{} F{} T{} K{}".format(ROUTE_NAMES[route], B, N, F, T, K)
    fast = route in (LAT, THR, GRP, RTN)
    seed = seed or (B * 7 + N * 5 + F * 3 + T * 2 + K)
    X, W = pr.gen_spectrogram(seed, B, N, F, T), pr.gen_filters(seed, B, F, N)
    if floor_inputs:
        basis, act = pr.gen_floor_nmf(seed, B, N, F, T, K)
        X = X * np.exp2(-44)  # |x|^2 / R small enough that a third to a half of the updates end below eps
    else:
        basis, act = pr.gen_nmf(seed, B, N, F, T, K)
    ws, wsb = ops.ilrma_workspace(B, N, F, T, K, dv.device())
    kind = model[0] & 0xff
    mname = "m{}p{}d{}f{}".format(model[0], model[1], domain, flooring[0])
    label = tag + " " + mname
    if own_line:
        label = "{}[B{},N{},F{},T{},K{},{}{}]".format(ROUTE_NAMES[route], B, N, F, T, K, mname,
                                                     ",floor_inputs" if floor_inputs else "")
    Xd, Wd, bd, ad = up(X), up(W), up(basis), up(act)
    for Wh, Wdev, wt in ((W, Wd, "W"), (None, None, "noW")):
        ref, bar = pr.ilrma_update_basis(X, Wh, basis, act, domain, model, flooring, fast_pow=fast)
        if floor_inputs and flooring[0] == pr.FLOOR_MAX:
            fl = float(np.mean(ref == LD(pr.EPS)))
            assert 0.05 < fl < 0.95, "floored share {}".format(fl)
        o = Out(basis.shape, fill=basis)
        ops.ilrma_update_basis(Xd, Wdev, o.t, ad, domain, flooring, ws, wsb, model=model)
        check("ilrma_update_basis_" + wt, label, o.get(), ref, bar)
        ref, bar = pr.ilrma_update_activation(X, Wh, basis, act, domain, model, flooring,
                                              fast_pow=fast)
        o = Out(act.shape, fill=act)
        ops.ilrma_update_activation(Xd, Wdev, bd, o.t, domain, flooring, ws, wsb, model=model)
        check("ilrma_update_activation_" + wt, label, o.get(), ref, bar)
        if not floor_inputs:
            ref, bar = pr.ilrma_loss_data(X, Wh, basis, act, domain, model, fast_pow=fast)
            o = Out((B,))
            ops.ilrma_loss_data(Xd, Wdev, bd, ad, domain, out=o.t, model=model)
            check("ilrma_loss_data_" + wt, label, o.get(), ref, bar)
    # covariance: the filter is read by the heavy-tailed models only
    Wh, Wdev = (None, None) if kind == pr.GAUSS else (W, Wd)
    ref, bar = pr.ilrma_weighted_covariance(X, Wh, basis, act, domain, model, flooring,
                                            fast_pow=fast)
    o = Out((B, F, N, N, N), True)
    ops.ilrma_weighted_covariance(Xd, bd, ad, domain, ws, wsb, out=o.t, W=Wdev, model=model,
                                  flooring=flooring)
    check("ilrma_weighted_covariance", label, o.get(), ref, bar)
    ref, bar = pr.ilrma_iss_weight(X, basis, act, domain, model, flooring)
    o = Out((B, N, F, T))
    ops.ilrma_iss_weight(bd, ad, domain, out=o.t, Y=Xd, model=model, flooring=flooring)
    check("ilrma_iss_weight", label, o.get(), ref, bar)
    Ypow = np.abs(X) ** 2
    ref, bar = pr.ilrma_iss_weight(None, basis, act, domain, model, flooring, Ypow=Ypow)
    o = Out((B, N, F, T))
    ops.ilrma_iss_weight(bd, ad, domain, out=o.t, model=model, flooring=flooring, Ypow=up(Ypow))
    check("ilrma_iss_weight_power", label, o.get(), ref, bar)


@pytest.mark.parametrize("N", [2, 3, 4])
@pytest.mark.parametrize("B,route", [(175, LAT), (176, THR)])
def test_ilrma_latency_throughput_boundary(B, route, N):
    """F = 17 is two bin tiles: 175 mixtures are 350 tiles (latency kernels), 176 leave them."""
    _ilrma_passes(B, N, 17, 17, 7, route)


@pytest.mark.parametrize("K,T", [(16, 16), (16, 64), (17, 16), (32, 40), (12, 40), (16, 40)])
def test_ilrma_throughput_k_tiles_and_full_tiles(K, T):
    """K = 16 with T % 16 == 0 takes the full-tile instances; T = 40 or K = 12 must not; 17 and 32
    are two k tiles (basis out of place).  The 176 basis items are all split in two frame chunks at
    T = 40 and 64 (three and four frame tiles) and unsplit at one frame tile or two k tiles.  Up to 16 bases the activation pass runs in chunks at this
    batch (176 blocks per chunk); two k tiles double the blocks and the plan keeps one chunk, folded
    all the same (the in-place finish is for n_basis <= 16)."""
    _ilrma_passes(176, 4, 17, T, K, THR, chunks="many" if K <= 16 else "one",
                  split="all" if (T > 16 and K <= 16) else "none")


def test_ilrma_two_k_tiles_chunked_activation():
    """K = 17 with an activation pass of several chunks (the fold above 16 bases)."""
    _ilrma_passes(*K17_CHUNKED, 17, THR, chunks="many")


@pytest.mark.parametrize("N,T,K", [(2, 16, 16), (2, 20, 12)])
def test_ilrma_activation_finished_in_place(N, T, K):
    """blocks0 = B ceil(T / 64) ceil(K / 16) = 2048: one chunk, the update applied in place (the
    full-tile and the masked instance)."""
    _ilrma_passes(2048, N, 17, T, K, THR, chunks="one")


@pytest.mark.parametrize("F", [65, 33, 17, 80, 64])
def test_ilrma_edge_groups(F):
    """The bin-edge items of test_gpu_edge_items.py at 272 mixtures and two frame tiles: two bin groups
    (F = 65, 80) are 544 basis items, 512 unsplit and 32 split in two; one bin group is 272 unsplit
    items."""
    _ilrma_passes(272, 2, F, 32, 16, THR, split="mixed" if F > 64 else "none")


def test_ilrma_edge_group_four_sources_masked():
    _ilrma_passes(272, 4, 65, 24, 12, THR, split="mixed")


@pytest.mark.parametrize("B,N", [(2, 8), (2, 6), (1, 5), (2, 5), (3, 5), (3, 7), (2, 7), (1, 7)])
def test_ilrma_grouped_sources(B, N):
    """N = 8 (groups of 4), 6 (3); 5 and 7 with B N % 4 = 1, 2, 3: the closing 3 + 2, 2, 3 groups."""
    if N in (5, 7):
        assert (B * N) % 4 == {(1, 5): 1, (2, 5): 2, (3, 5): 3, (3, 7): 1, (2, 7): 2, (1, 7): 3}[(B, N)]
    _ilrma_passes(B, N, 17, 17, 7, GRP)


@pytest.mark.parametrize("K", [33, 40])
def test_ilrma_wide_basis(K):
    _ilrma_passes(2, 3, 17, 17, K, WIDE)


@pytest.mark.parametrize("K", [33, 64, 65])
def test_ilrma_wide_basis_edge_tiles(K):
    """k_gemm_f64 past one workgroup tile.  F = 100, T = 97: two 64 x 64 tiles each way, the edge
    tiles with 36 and 33 live rows / columns -- all four waves and both 16-row sub-tiles of each hold
    data next to masked lanes, blockIdx.x and .y reach 1.  The depth Kd is K for R = T V (33: two
    full stages and one of 1; 64: four full stages, no remainder; 65: four and one of 1), T = 97 for
    the basis products (seven stages, the A side kd-contiguous, the B side outer-contiguous) and
    F = 100 for the activation products (seven stages, both sides outer-contiguous; K is the row
    count there: one tile of 33 rows, one full tile, a second tile of one row).  B N = 3 sources:
    the numerator / denominator pairs of the dual launches sit at odd and even g >> 1."""
    _ilrma_passes(1, 3, 100, 97, K, WIDE, own_line=True)


@pytest.mark.parametrize("F,T", [(64, 65), (65, 64)])
def test_ilrma_wide_basis_tile_boundaries(F, T):
    """Exactly one full tile one way, one tile and a single row / column the other."""
    _ilrma_passes(1, 2, F, T, 33, WIDE, own_line=True)


@pytest.mark.parametrize("model,domain", MODELS)
def test_ilrma_wide_basis_models(model, domain):
    """Every model through the epilogues of k_gemm_f64 (EPI_AB, EPI_PHI, EPI_LOSS) and k_mu_update;
    F = 40, T = 36: waves 0..3 hold 32 x 32, 32 x 4, 8 x 32 and 8 x 4 live entries."""
    _ilrma_passes(1, 3, 40, 36, 33, WIDE, model=model, domain=domain, own_line=True)


@pytest.mark.parametrize("flooring", [NOF, MAXF, ADDF])
@pytest.mark.parametrize("model,domain", [MODELS[0], MODELS[7]])
def test_ilrma_wide_basis_floors(model, domain, flooring):
    """k_mu_update's floor with updated values on both sides of eps (test_pass_reference_cpu.py checks
    the floored share of these inputs with the reference alone)."""
    _ilrma_passes(1, 3, 40, 36, 33, WIDE, model=model, domain=domain, flooring=flooring,
                  floor_inputs=True, own_line=True)


@pytest.mark.parametrize("N", [9, 16])
def test_ilrma_runtime_source_count(N):
    _ilrma_passes(1, N, 17, 17, 7, RTN)


@pytest.mark.parametrize("B,N,F,T,K", [(1, 9, 70, 67, 7), (1, 9, 70, 67, 40), (1, 16, 3, 300, 7),
                                       (2, 9, 3, 257, 7)])
def test_ilrma_runtime_source_count_tiles_and_frames(B, N, F, T, K):
    """F = 70, T = 67: edge tiles of 6 and 3 rows / columns.  At K = 7 the NMF passes of 9 = 3 x 3 and
    16 = 4 x 4 sources are walked in groups by the tuned kernels (source_group) and k_gemm_f64 runs for
    the loss alone (EPI_LOSS, Kd = 7: a single short stage); K = 40 (both reasons for the route at
    once) puts every pass on the dense products, three stages deep.  T = 300 and 257 at F = 3: the
    frame loops of wide_n.hip (256 threads along frames: separate, its power form in front of the
    filtered passes) take a second trip, k_cov_rt ten and nine frame tiles."""
    _ilrma_passes(B, N, F, T, K, RTN, own_line=True)


@pytest.mark.parametrize("N", [2, 3, 4, 5, 6, 7, 8])
def test_ilrma_generic_kernels(N):
    """The t model at domain 1 is off the tuned path: the per-N kernels of ilrma_kernels.hip."""
    _ilrma_passes(2, N, 17, 17, 7, GEN, model=(pr.TMODEL, 3.0), domain=1.0)


@pytest.mark.parametrize("B,route", [(2, LAT), (180, THR)])
@pytest.mark.parametrize("model,domain", MODELS)
def test_ilrma_models(model, domain, B, route):
    """Every model of the tuned path (FM_GAUSS with and without ME, FM_GAUSS1, FM_GAUSSP, FM_T,
    FM_GGD with its two square-root shortcuts and the exp2 / log2 form)."""
    _ilrma_passes(B, 3, 17, 40, 12, route, model=model, domain=domain)


@pytest.mark.parametrize("B,route", [(2, LAT), (180, THR)])
@pytest.mark.parametrize("flooring", [NOF, MAXF, ADDF])
@pytest.mark.parametrize("model,domain", [MODELS[0], MODELS[7]])
def test_ilrma_floors(model, domain, flooring, B, route):
    """Updated values on both sides of eps = 1e-10 (a share of them floored, a few exactly at it)."""
    _ilrma_passes(B, 3, 17, 40, 12, route, model=model, domain=domain, flooring=flooring,
                  floor_inputs=True)


@pytest.mark.parametrize("B,route", [(2, LAT), (400, THR)])
@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("F", [1, 15, 16, 17])
def test_ilrma_tiny_shapes(F, K, B, route):
    for T in (1, 2, 15, 16, 17, 64, 65):
        _ilrma_passes(B, 2, F, T, K, route, seed=1000 + F * 70 + T)


@pytest.mark.parametrize("N", [2, 4, 6, 9])
@pytest.mark.parametrize("flooring", [MAXF, ADDF])
def test_ilrma_normalize(N, flooring):
    """normalize_filter, normalize_output (power computed, frame power given, tracked log-det)."""
    _, dv, _, ops = _mods()
    B, F, T, K, domain = 2, 17, 33, 7, 2.0 if N != 4 else 1.0
    X, W = pr.gen_spectrogram(70 + N, B, N, F, T), pr.gen_filters(70 + N, B, F, N, 4)
    basis, _ = pr.gen_nmf(70 + N, B, N, F, T, K)
    C = np.asarray(pr.cross_covariance(X, X)[0], dtype=np.complex128)
    ws, wsb = ops.ilrma_workspace(B, N, F, T, K, dv.device())
    Wn, barW, bn, barb, _, _ = pr.ilrma_normalize_filter(W, C, basis, domain, flooring)
    oW, ob = Out(W.shape, True, fill=W), Out(basis.shape, fill=basis)
    ops.ilrma_normalize_filter(oW.t, up(C), ob.t, domain, flooring, ws, wsb)
    check("ilrma_normalize_filter_W", "N={}".format(N), oW.get(), Wn, barW)
    check("ilrma_normalize_filter_basis", "N={}".format(N), ob.get(), bn, barb)
    fp = np.asarray(pr.iva_frame_power(X)[0], dtype=np.float64)
    ld0 = np.random.default_rng(N).standard_normal(B) * 50
    for tag, kw, rkw in (("", {}, {}), ("_frame_power", {"frame_power": up(fp)}, {"frame_power": fp}),
                         ("_tracked", {}, {"logdet": ld0})):
        res = pr.ilrma_normalize_output(X, basis, domain, flooring, **rkw)
        oY, ob = Out(X.shape, True, fill=X), Out(basis.shape, fill=basis)
        if tag == "_tracked":
            ol = Out((B,), fill=ld0)
            kw = {"logdet": ol.t}
        ops.ilrma_normalize_output(oY.t, ob.t, domain, flooring, ws, wsb, **kw)
        check("ilrma_normalize_output" + tag + "_Y", "N={}".format(N), oY.get(), res[0], res[1])
        check("ilrma_normalize_output" + tag + "_basis", "N={}".format(N), ob.get(), res[2], res[3])
        if tag == "_tracked":
            check("ilrma_normalize_output_tracked_logdet", "N={}".format(N), ol.get(), res[4], res[5])


@pytest.mark.parametrize("B,N", [(2, 2), (2, 3), (2, 4), (40, 4), (2, 5), (2, 6), (2, 7), (2, 8), (2, 9),
                                 (1, 16)])
def test_update_by_ip1(B, N):
    """update_by_ip1 and update_by_ip1_logdet (shares folded with fold_scalar_slots): normwise per
    bin, c = 8 x what np.linalg.solve makes of the same inputs (see the module docstring)."""
    _, dv, _, ops = _mods()
    F = 17
    W, Uc = pr.gen_ip1_inputs(80 + N + B, B, F, N)
    ref, kappa = pr.update_by_ip1(W, Uc, MAXF)
    assert kappa.max() <= 1e3
    c_np = pr.ip1_row_error(pr.update_by_ip1_float64(W, Uc, MAXF), ref, kappa)
    c = 8 * c_np
    info = dv.zeros((1,), dv.i32)
    o = Out(W.shape, True, fill=W)
    ops.update_by_ip1(o.t, up(Uc), MAXF, info)
    e1 = pr.ip1_row_error(o.get(), ref, kappa)
    slots = ops.update_by_ip1_logdet_slots(B, F, N)
    o2 = Out(W.shape, True, fill=W)
    shares = Out((slots, B), fill=np.zeros((slots, B)))
    ops.update_by_ip1_logdet(o2.t, up(Uc), MAXF, info, shares.t, B)
    e2 = pr.ip1_row_error(o2.get(), ref, kappa)
    shares.get()
    ld = Out((B,))
    ops.fold_scalar_slots(shares.t, B, slots, ld.t)
    for name, e in (("update_by_ip1", e1), ("update_by_ip1_logdet", e2)):
        line = "{}\tB={} N={}\t{:.2f}\t{:.2f}\t{:.4f}\t(c_np {:.3f}, kappa max {:.1f})".format(
            name, B, N, e, c, e / c, c_np, float(kappa.max()))
        print(line)
        if os.environ.get("SSSPY_PASS_PROFILE_RAW"):
            with open(os.environ["SSSPY_PASS_PROFILE_RAW"], "a") as f:
                f.write(line + "\n")
        assert e <= c, line
    assert int(info.item()) == 0
    lref, lbar = pr.sum_logdet(W)
    check("update_by_ip1_logdet_value", "B={} N={}".format(B, N), ld.get(), lref,
          lbar + slots * pr.U * np.abs(lref))


FUSED = [(2, 3, 12, LAT, G2[0], 2.0), (180, 3, 12, THR, G2[0], 2.0), (180, 4, 16, THR, G2[0], 2.0),
         (180, 2, 32, THR, G2[0], 2.0), (2, 4, 12, LAT, (pr.GGD, 1.2), 2.0),
         (180, 3, 12, THR, (pr.GAUSS, 0.0), 1.0), (2, 6, 7, GRP, G2[0], 2.0), (2, 3, 33, WIDE, G2[0], 2.0),
         (1, 9, 7, RTN, G2[0], 2.0), (2, 3, 12, GEN, (pr.TMODEL, 3.0), 1.0)]


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("B,N,K,route,model,domain", FUSED)
def test_ilrma_ip1_update_fused(B, N, K, route, model, domain, normalize):
    """One fused ilrma_ip1_update against the composition of the references: basis, activation WITH
    THE NEW BASIS (its bar carries the new basis's own error: basis_rel_u), covariance, IP1,
    normalisation; and the _loss_slots variant wherever ilrma_deferred_loss_slots() > 0, its data and
    log-det shares folded with fold_scalar_slots and compared with the loss of the state AT ENTRY.

    Bars.  normalize = False: basis and activation elementwise, as in their own passes.  W comes from
    solves: per bin and row ||w - w_ref|| <= c kappa u ||w_ref||, kappa = max_n kappa_2(W U_n) of the
    extended-precision sweep, c = 8 x the kappa-normalised error of the SAME composition evaluated in
    float64 NumPy with np.linalg.solve (the issue's recipe; the composition, not the bare sweep,
    because the covariances the sweep starts from are themselves rounded).  normalize = True:
    psi_n^2 = mean_i q_in, q_in = w_in^H C_i w_in, moves with the rows: |dq_in| <= 2 e_i ||C_i|| ||w_in||^2,
    e_i = c kappa_i u, plus the quadratic form's own (6 N + 2) u sum |w||c||w| and the mean's
    (F + 1) u; the square root halves it and adds 2 u: rel(psi).  Rows of W then carry
    (c kappa + rel(psi) + 3) u normwise, the basis rel(basis) + p rel(psi) + 5 u elementwise; the
    activation is not scaled."""
    _, dv, _, ops = _mods()
    F, T = 17, 40 if N <= 6 else 64
    got_route = ops.ilrma_route(B, N, F, T, K, domain, model)[0]
    assert got_route == route, ROUTE_NAMES[got_route]
    tag = "{} B{} N{} K{} m{}p{}d{} norm{}".format(ROUTE_NAMES[route], B, N, K, model[0], model[1],
                                                   domain, int(normalize))
    fast = route in (LAT, THR, GRP, RTN)
    X, W, basis, act, C = pr.gen_fused_inputs(300 + B + N + K, B, N, F, T, K)
    ref = pr.ilrma_ip1_update(X, C, W, basis, act, domain, model, normalize, MAXF, fast_pow=fast)
    f64 = pr.ilrma_ip1_update(X, C, W, basis, act, domain, model, normalize, MAXF, dtype=np.float64,
                              fast_pow=fast)
    kappa = ref["kappa"]
    assert kappa.max() <= 1e3
    c_np = pr.ip1_row_error(f64["W"], ref["W"], kappa)
    c = 8 * c_np
    row_extra = 0.0
    bar_basis = ref["bar_basis"]
    if normalize:
        raw = pr.ilrma_ip1_update(X, C, W, basis, act, domain, model, False, MAXF, fast_pow=fast)
        Wr = raw["W"]
        q = np.einsum("bink,bikl,binl->bin", Wr, C.astype(np.clongdouble), Wr.conj()).real
        qa = np.einsum("bink,bikl,binl->bin", np.abs(Wr), np.abs(C).astype(LD), np.abs(Wr))
        normC = np.linalg.norm(C, 2, axis=(2, 3))                                  # (B, F)
        w2 = (np.abs(Wr) ** 2).sum(axis=-1)                                        # (B, F, N)
        dq = 2 * c * (kappa * normC)[:, :, None] * w2 + (6 * N + 2) * qa           # in u
        rel_psi = 0.5 * (dq.mean(axis=1) / q.mean(axis=1) + F + 1) + 2             # (B, N)
        row_extra = float(rel_psi.max()) + 3
        bar_basis = ref["basis"] * pr.U * (raw["bar_basis"] / (pr.U * raw["basis"])
                                           + (LD(domain) * rel_psi + 5)[:, :, None, None])

    def run(with_slots):
        ws, wsb = ops.ilrma_workspace(B, N, F, T, K, dv.device())
        oW, ob = Out(W.shape, True, fill=W), Out(basis.shape, fill=basis)
        oa, oU = Out(act.shape, fill=act), Out((B, F, N, N, N), True)
        info = dv.zeros((1,), dv.i32)
        args = (up(X), up(C), oW.t, ob.t, oa.t, oU.t, domain, normalize, MAXF, ws, wsb, info)
        name = "ilrma_ip1_update"
        if with_slots:
            name = "ilrma_ip1_update_loss_slots"
            ns = ops.ilrma_deferred_loss_slots(B, N, F, T, K, domain, model)
            nl = ops.ilrma_deferred_logdet_slots(B, N, F, T, K, domain, model)
            sl = Out((ns, B), fill=np.zeros((ns, B)))
            ll = Out((nl, B), fill=np.zeros((nl, B)))
            ops.ilrma_ip1_update_loss_slots(*args, sl.t, B, ll.t, model=model)
            sl.get(), ll.get()
            od, ol = Out((B,)), Out((B,))
            ops.fold_scalar_slots(sl.t, B, ns, od.t)
            ops.fold_scalar_slots(ll.t, B, nl, ol.t)
            lref, lbar = pr.ilrma_loss_data(X, W, basis, act, domain, model, fast_pow=fast)
            check(name + "_loss_data", tag, od.get(), lref, lbar + ns * pr.U * np.abs(lref))
            dref, dbar = pr.sum_logdet(W)
            check(name + "_logdet", tag, ol.get(), dref, dbar + nl * pr.U * np.abs(dref))
        else:
            ops.ilrma_ip1_update(*args, model=model)
        check(name + "_basis", tag, ob.get(), ref["basis"], bar_basis)
        check(name + "_activation", tag, oa.get(), ref["activation"], ref["bar_activation"])
        e = pr.ip1_row_error(oW.get(), ref["W"], kappa)
        lim = c + row_extra / float(kappa.min())
        line = "{}_W\t{}\t{:.2f}\t{:.2f}\t{:.4f}\t(c_np {:.3f}, kappa max {:.1f})".format(
            name, tag, e, lim, e / lim, c_np, float(kappa.max()))
        print(line)
        if os.environ.get("SSSPY_PASS_PROFILE_RAW"):
            with open(os.environ["SSSPY_PASS_PROFILE_RAW"], "a") as f:
                f.write(line + "\n")
        assert e <= lim, line
        assert int(info.item()) == 0

    run(False)
    if ops.ilrma_deferred_loss_slots(B, N, F, T, K, domain, model) > 0:
        run(True)
    else:
        assert not ops.ilrma_deferred_loss_supported(N, F, T, K, domain, model)


# ------------------------------------------------------------------------------- AuxIVA passes
@pytest.mark.parametrize("B,N,F,T", [(1, 2, 17, 65), (2, 3, 1, 1), (2, 4, 33, 17), (128, 2, 17, 16),
                                     (3, 6, 16, 64), (2, 8, 15, 2), (1, 9, 17, 15), (1, 16, 17, 33),
                                     (1, 9, 17, 257), (1, 9, 17, 300), (1, 16, 17, 257),
                                     (1, 16, 17, 300)])
def test_iva_frame_power(B, N, F, T):
    """iva_frame_power with and without a filter, separate_frame_power (to 8 sources).  B = 128 takes
    the thread-per-frame kernel, the others the four-wave form with folded bin chunks; 9 and 16
    sources the run-time-N kernel, a thread per frame in blocks of 256: T = 257 and 300 are a second
    frame block of 1 and of 44 threads."""
    _, dv, _, ops = _mods()
    X, W = pr.gen_spectrogram(90 + N, B, N, F, T), pr.gen_filters(90 + N, B, F, N)
    # (the cases of a second frame block keep profile lines of their own)
    tag = ("B{},N{},F{},T{}" if T > 256 else "B{} N{} F{} T{}").format(B, N, F, T)
    for Wh, wt in ((None, "noW"), (W, "W")):
        ref, bar = pr.iva_frame_power(X, Wh)
        o = Out((B, N, T))
        ops.iva_frame_power(up(X), None if Wh is None else up(W), out=o.t)
        check("iva_frame_power_" + wt, tag, o.get(), ref, bar)
    if N <= 8:
        Y, barY = pr.separate(X, W)
        ref, bar = pr.iva_frame_power(X, W)
        oY, o = Out(X.shape, True, fill=X), Out((B, N, T))
        ops.separate_frame_power(oY.t, up(W), r2=o.t)
        check("separate_frame_power_Y", tag, oY.get(), Y, barY)
        check("separate_frame_power_r2", tag, o.get(), ref, bar)


@pytest.mark.parametrize("flooring", [NOF, MAXF, ADDF])
@pytest.mark.parametrize("contrast", [0, 1, 2])
def test_iva_weight_and_loss(contrast, flooring):
    """LAPLACE / GAUSS / GAUSS_FIXED; 2 r on both sides of eps and exactly at it; T = 300: a second
    block of 44.  The loss for LAPLACE and GAUSS."""
    _, dv, _, ops = _mods()
    B, N, T, F = 2, 3, 300, 17
    rng = np.random.default_rng(95 + contrast)
    r2 = np.exp2(rng.uniform(-40, 40, (B, N, T)))
    r2[0, 0, :100] = (pr.EPS / 2) ** 2 * np.exp2(rng.uniform(-6, 6, 100))
    r2[0, 1, :8] = (pr.EPS / 2) ** 2
    var = np.exp2(rng.uniform(-12, 12, (B, N, T)))
    w, bar, v, vbar = pr.iva_weight(r2, var, F, contrast, flooring)
    if flooring[0] == pr.FLOOR_MAX:
        assert 0.01 < np.mean(2 * np.sqrt(r2) < pr.EPS) < 0.5
    ow, ov = Out((B, N, T)), Out((B, N, T), fill=var)
    ops.iva_weight(up(r2), F, contrast, flooring, weight=ow.t, variance=None if contrast == 0 else ov.t)
    tag = "contrast{} floor{}".format(contrast, flooring[0])
    check("iva_weight", tag, ow.get(), w, bar)
    if contrast == 1:
        check("iva_weight_variance", tag, ov.get(), v, vbar)
    elif contrast == 2:
        assert np.array_equal(ov.get(), var)
    if contrast < 2 and flooring[0] == pr.FLOOR_NONE:
        ref, lbar = pr.iva_loss_data(r2, var, F, contrast)
        o = Out((B,))
        ops.iva_loss_data(up(r2), None if contrast == 0 else up(var), F, contrast, out=o.t)
        check("iva_loss_data", tag, o.get(), ref, lbar)


# ------------------------------------------------------------------------------- profile
def _write_profile(raw, path):
    worst = {}
    for line in open(raw):
        f = line.rstrip("\n").split("\t")
        key = (f[0], f[1].split(" ")[0])
        if key not in worst or float(f[4]) > float(worst[key][4]):
            worst[key] = f
    with open(path, "w") as out:
        out.write("# largest measured error of every entry point and route, tests/test_gpu_pass_"
                  "elementwise.py on an MI355X\n# entry point, route: worst case; error and bar in "
                  "units of u = 2^-53 of the reference value at the worst element; ratio = error / bar\n")
        for key in sorted(worst):
            f = worst[key]
            out.write("{:44s} {:52s} err {:>10s} u  bar {:>10s} u  ratio {}{}\n".format(
                f[0], f[1], f[2], f[3], f[4], "  " + f[5] if len(f) > 5 else ""))


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles")
    raw = os.path.join(out_dir, "pass_elementwise.raw")
    if os.path.exists(raw):
        os.remove(raw)
    os.environ["SSSPY_PASS_PROFILE_RAW"] = raw
    rc = pytest.main([os.path.abspath(__file__), "-m", "gpu", "-q", "--maxfail=15", "--durations=8"]
                     + sys.argv[2:])
    if os.path.exists(raw):
        _write_profile(raw, os.path.join(out_dir, "pass_elementwise.txt"))
        os.remove(raw)
    sys.exit(int(rc))
