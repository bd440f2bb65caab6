"""The extended-precision pass reference (tests/pass_reference.py) checked without a GPU: it agrees
with the float64 oracle within its own bars, the bars are attainable by a plain float64 NumPy
evaluation of the same formulas on the generators' inputs (no element left out), and the generators
have the properties the GPU tests rely on."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pass_reference as pr  # noqa: E402

LD = pr.LD
MAXF, ADDF, NOF = (pr.FLOOR_MAX, pr.EPS), (pr.FLOOR_ADD, pr.EPS), (pr.FLOOR_NONE, 0.0)
MODELS = [((pr.GAUSS, 0.0), 2.0), ((pr.GAUSS | pr.ME, 0.0), 2.0), ((pr.GAUSS, 0.0), 1.0),
          ((pr.GAUSS, 0.0), 1.3), ((pr.TMODEL, 3.0), 2.0), ((pr.GGD, 1.0), 2.0),
          ((pr.GGD, 0.5), 2.0), ((pr.GGD, 1.2), 2.0), ((pr.TMODEL, 3.0), 1.0)]


def inside(got, ref, bar):
    err = np.abs(np.asarray(got).astype(np.asarray(ref).dtype) - ref)
    assert np.all(np.isfinite(np.asarray(got, dtype=np.complex128)))
    worst = float(np.max(err / bar))
    assert worst <= 1.0, worst
    return worst


def _inputs(seed, B, N, F, T, K):
    X, W = pr.gen_spectrogram(seed, B, N, F, T), pr.gen_filters(seed, B, F, N)
    basis, act = pr.gen_nmf(seed, B, N, F, T, K)
    return X, W, basis, act


# ------------------------------------------------------------------------------- against the oracle
def _oracle(model, domain, X, W, basis, act, flooring=("max", pr.EPS)):
    from oracle.ilrma import GaussILRMAOracle

    kind = model[0] & 0xff
    name = {pr.GAUSS: ("gauss", None), pr.TMODEL: ("t", model[1]), pr.GGD: ("ggd", model[1])}[kind]
    o = GaussILRMAOracle(n_basis=basis.shape[-1], domain=domain, flooring=flooring, model=name,
                         source_algorithm="ME" if model[0] & pr.ME else "MM",
                         spatial_algorithm="IP" if W is not None else "ISS")
    o.reset(X, basis=basis, activation=act, demix_filter=W)
    return o


@pytest.mark.parametrize("with_filter", [True, False])
@pytest.mark.parametrize("model,domain", MODELS)
def test_ilrma_reference_matches_oracle(model, domain, with_filter):
    from oracle import spatial as sp

    N, F, T, K = 3, 17, 40, 12
    X, W, basis, act = _inputs(5, 1, N, F, T, K)
    Wb = W if with_filter else None
    o = _oracle(model, domain, X[0], W[0] if with_filter else None, basis[0], act[0])
    ref, bar = pr.ilrma_update_basis(X, Wb, basis, act, domain, model, MAXF, fast_pow=False)
    o.update_basis()
    inside(o.basis, ref[0], bar[0])
    o.basis = basis[0].copy()
    ref, bar = pr.ilrma_update_activation(X, Wb, basis, act, domain, model, MAXF, fast_pow=False)
    o.update_activation()
    inside(o.activation, ref[0], bar[0])
    o.activation = act[0].copy()
    ref, bar = pr.ilrma_loss_data(X, Wb, basis, act, domain, model, fast_pow=False)
    if with_filter:
        ld, lbar = pr.sum_logdet(W)
        inside(o.compute_loss(), ref[0] - 2 * ld[0], bar[0] + 2 * lbar[0])
    Y = o._current_output()
    P = (np.abs(Y) ** 2)[None].astype(LD)
    v, vu = pr.ilrma_weight(P, pr.power(X, Wb)[1] / (pr.U * pr.power(X, Wb)[0]), basis, act, domain,
                            model, MAXF, fast_pow=False)
    inside(o._spatial_weight(Y), v[0], pr.U * v[0] * vu[0])
    if with_filter:
        Uo = sp.weighted_covariance(X[0], o._spatial_weight(Y))
        ref, bar = pr.ilrma_weighted_covariance(X, W, basis, act, domain, model, MAXF, fast_pow=False)
        inside(Uo, ref[0], bar[0])


@pytest.mark.parametrize("N", [2, 4, 9])
def test_shared_reference_matches_oracle(N):
    from oracle import spatial as sp

    F, T = 17, 33
    X, W = pr.gen_spectrogram(6 + N, 1, N, F, T), pr.gen_filters(6 + N, 1, F, N)
    Y, bar = pr.separate(X, W)
    inside(sp.separate(X[0], W[0]), Y[0], bar[0])
    w = pr.gen_weights(7, (1, N, F, T))
    ref, bar = pr.weighted_covariance(X, w, 2, N)
    inside(sp.weighted_covariance(X[0], w[0]), ref[0], bar[0])
    ref, bar = pr.weighted_covariance(X, w[:, :, 0], 1, N)
    inside(sp.weighted_covariance(X[0], w[0, :, 0]), ref[0], bar[0])
    ld, lbar = pr.sum_logdet(W)
    inside(np.sum(np.linalg.slogdet(W[0])[1]), ld[0], lbar[0])
    W1, Uc = pr.gen_ip1_inputs(8 + N, 1, F, N)
    ref, kappa = pr.update_by_ip1(W1, Uc, MAXF)
    got = sp.update_by_ip1(W1[0], Uc[0], ("max", pr.EPS))
    c_np = pr.ip1_row_error(pr.update_by_ip1_float64(W1, Uc, MAXF), ref, kappa)
    assert pr.ip1_row_error(got[None], ref, kappa) <= 8 * c_np


# ------------------------------------------------------------------------------- attainable bars
SHAPES = [(3, 3, 17, 40, 12), (2, 2, 1, 1, 1), (2, 2, 15, 2, 7), (2, 2, 16, 65, 7), (2, 4, 17, 64, 16),
          (2, 4, 65, 40, 12), (2, 3, 17, 17, 33), (1, 8, 17, 17, 7), (1, 16, 17, 17, 7),
          (1, 3, 40, 36, 33)]


# the large-batch legs of the GPU file run the Gauss model at domain 2 only; so do they here
BIG_SHAPES = [(176, 4, 17, 40, 32), (176, 4, 17, 64, 16), (272, 2, 80, 32, 16), (272, 4, 65, 24, 12),
              (2048, 2, 17, 20, 12), (400, 2, 17, 65, 7), (90, 4, 65, 16, 17), (2, 3, 17, 17, 40)]


@pytest.mark.parametrize("B,N,F,T,K", SHAPES + BIG_SHAPES)
def test_float64_stays_inside_the_ilrma_bars(B, N, F, T, K):
    """Every model, with and without a filter, exp2(e log2 x) powers included (fast_pow), at the
    distinct (N, F, T, K) of the GPU file (its remaining cases repeat these with another batch size or
    seed).  The size check m < 1024 is asserted for the positive-sum passes proper: basis and activation
    without a filter.  With a filter the budget of an element holds 6 N S / |y|, which depends on how
    much y = W x cancels in that element and has no bound a priori (a few hundred u at 2..4 sources,
    several thousand at 16 on these inputs): those cases are exempt from the size check, not from the
    bar."""
    X, W, basis, act = _inputs(B * 7 + N * 5 + F * 3 + T * 2 + K, B, N, F, T, K)
    worst_m = 0.0
    for model, domain in (MODELS if B <= 3 else MODELS[:1]):
        for Wb in (W, None):
            for fn in (pr.ilrma_update_basis, pr.ilrma_update_activation,
                       pr.ilrma_weighted_covariance):
                ref, bar = fn(X, Wb, basis, act, domain, model, MAXF)
                inside(fn(X, Wb, basis, act, domain, model, MAXF, dtype=np.float64)[0], ref, bar)
                if Wb is None and fn is not pr.ilrma_weighted_covariance:
                    worst_m = max(worst_m, float(np.max(bar / (pr.U * ref))))
            ref, bar = pr.ilrma_loss_data(X, Wb, basis, act, domain, model)
            inside(pr.ilrma_loss_data(X, Wb, basis, act, domain, model, dtype=np.float64)[0], ref, bar)
        ref, bar = pr.ilrma_iss_weight(X, basis, act, domain, model, MAXF)
        inside(pr.ilrma_iss_weight(X, basis, act, domain, model, MAXF, dtype=np.float64)[0], ref, bar)
    # the size check of the positive-sum passes: m below 1024 at every shape used
    assert worst_m < 1024, worst_m


@pytest.mark.parametrize("flooring", [NOF, MAXF, ADDF])
@pytest.mark.parametrize("model,domain", [MODELS[0], MODELS[7]])
def test_float64_stays_inside_the_bars_at_the_floor(model, domain, flooring):
    B, N, F, T, K = 2, 3, 17, 40, 12
    X = pr.gen_spectrogram(9, B, N, F, T) * np.exp2(-44)
    W = pr.gen_filters(9, B, F, N)
    basis, act = pr.gen_floor_nmf(9, B, N, F, T, K)
    assert np.mean(basis == pr.EPS) > 0.1 and np.mean(basis < pr.EPS) > 0.2 \
        and np.mean(basis > pr.EPS) > 0.2
    for Wb in (W, None):
        for fn in (pr.ilrma_update_basis, pr.ilrma_update_activation):
            ref, bar = fn(X, Wb, basis, act, domain, model, flooring)
            inside(fn(X, Wb, basis, act, domain, model, flooring, dtype=np.float64)[0], ref, bar)
            if flooring[0] == pr.FLOOR_MAX:
                assert 0.05 < float(np.mean(ref == LD(pr.EPS))) < 0.95


# the edge-tile, tile-boundary and long-frame shapes of the dense-product routes (n_basis >= 33, or 9..16
# sources): the GPU file runs the Gauss model at domain 2 there; so do they here
DENSE_SHAPES = [(1, 3, 100, 97, 33), (1, 3, 100, 97, 64), (1, 3, 100, 97, 65), (1, 2, 64, 65, 33),
                (1, 2, 65, 64, 33), (1, 9, 70, 67, 7), (1, 9, 70, 67, 40), (1, 16, 3, 300, 7),
                (2, 9, 3, 257, 7)]


@pytest.mark.parametrize("B,N,F,T,K", DENSE_SHAPES)
def test_float64_stays_inside_the_ilrma_bars_at_the_dense_shapes(B, N, F, T, K):
    X, W, basis, act = _inputs(B * 7 + N * 5 + F * 3 + T * 2 + K, B, N, F, T, K)
    model, domain = MODELS[0]
    for Wb in (W, None):
        for fn in (pr.ilrma_update_basis, pr.ilrma_update_activation, pr.ilrma_weighted_covariance):
            ref, bar = fn(X, Wb, basis, act, domain, model, MAXF)
            inside(fn(X, Wb, basis, act, domain, model, MAXF, dtype=np.float64)[0], ref, bar)
        ref, bar = pr.ilrma_loss_data(X, Wb, basis, act, domain, model)
        inside(pr.ilrma_loss_data(X, Wb, basis, act, domain, model, dtype=np.float64)[0], ref, bar)
    ref, bar = pr.ilrma_iss_weight(X, basis, act, domain, model, MAXF)
    inside(pr.ilrma_iss_weight(X, basis, act, domain, model, MAXF, dtype=np.float64)[0], ref, bar)


@pytest.mark.parametrize("flooring", [NOF, MAXF, ADDF])
@pytest.mark.parametrize("model,domain", [MODELS[0], MODELS[7]])
def test_floor_inputs_straddle_eps_at_33_bases(model, domain, flooring):
    """The floor case of the dense-product route, (B, N, F, T, K) = (1, 3, 40, 36, 33) from the seed the
    GPU file derives for it: with the reference alone, between 5 % and 95 % of the updated basis ends
    at the MAX floor (the condition the GPU case asserts), with and without a filter, and float64
    stays inside the bars on both sides of eps."""
    B, N, F, T, K = 1, 3, 40, 36, 33
    seed = B * 7 + N * 5 + F * 3 + T * 2 + K
    X = pr.gen_spectrogram(seed, B, N, F, T) * np.exp2(-44)
    W = pr.gen_filters(seed, B, F, N)
    basis, act = pr.gen_floor_nmf(seed, B, N, F, T, K)
    for Wb in (W, None):
        for fn in (pr.ilrma_update_basis, pr.ilrma_update_activation):
            for fast in (False, True):
                ref, bar = fn(X, Wb, basis, act, domain, model, flooring, fast_pow=fast)
                inside(fn(X, Wb, basis, act, domain, model, flooring, dtype=np.float64,
                          fast_pow=fast)[0], ref, bar)
            if flooring[0] == pr.FLOOR_MAX:
                assert 0.05 < float(np.mean(ref == LD(pr.EPS))) < 0.95


@pytest.mark.parametrize("N", [6, 7, 8])
def test_float64_stays_inside_the_covariance_bars_at_any_set_count(N):
    """weighted_covariance with 1 < S < N weight sets and the frame counts of the matrix-core
    covariance cases (T = 1 .. 129), every kind: the (T + 6) u bar holds for float64 NumPy."""
    B, F = 2, 5
    for T in (1, 7, 8, 9, 15, 17, 63, 64, 65, 71, 129):
        X = pr.gen_spectrogram(200 + 10 * N + T, B, N, F, T)
        for kind in (0, 1, 2):
            for S in ((1,) if kind == 0 else (1, 3, N)):
                w = None if kind == 0 else pr.gen_weights(
                    201 + N + T + S, (B, S, T) if kind == 1 else (B, S, F, T))
                ref, bar = pr.weighted_covariance(X, w, kind, S)
                assert ref.shape == (B, F, S, N, N)
                inside(pr.weighted_covariance(X, w, kind, S, dtype=np.float64)[0], ref, bar)


@pytest.mark.parametrize("N", [2, 4, 6, 9, 16])
def test_float64_stays_inside_the_shared_and_iva_bars(N):
    B, F, T, K = 2, 17, 33, 7
    X, W, basis, _ = _inputs(40 + N, B, N, F, T, K)
    f64 = np.float64
    for fn, args in ((pr.separate, (X, W)), (pr.cross_covariance, (X, X)),
                     (pr.compose_filters, (W, W)), (pr.iva_frame_power, (X, W)),
                     (pr.iva_frame_power, (X, None)),
                     (pr.weighted_covariance, (X, pr.gen_weights(1, (B, N, T)), 1, N)),
                     (pr.weighted_covariance, (X, None, 0, 1))):
        ref, bar = fn(*args)
        inside(fn(*args, dtype=f64)[0], ref, bar)
    C = np.asarray(pr.cross_covariance(X, X)[0], dtype=np.complex128)
    ref, bar = pr.covariance_congruence(C, W)
    inside(pr.covariance_congruence(C, W, dtype=f64)[0], ref, bar)
    ref, bar = pr.sum_logdet(W)
    inside(pr.sum_logdet(W, dtype=f64)[0], ref, bar)
    for flooring in (MAXF, ADDF):
        a, b = pr.ilrma_normalize_filter(W, C, basis, 2.0, flooring), \
            pr.ilrma_normalize_filter(W, C, basis, 2.0, flooring, dtype=f64)
        inside(b[0], a[0], a[1])
        inside(b[2], a[2], a[3])
        ld = np.linspace(-40, 40, B)
        a, b = pr.ilrma_normalize_output(X, basis, 1.0, flooring, logdet=ld), \
            pr.ilrma_normalize_output(X, basis, 1.0, flooring, dtype=f64, logdet=ld)
        for k in (0, 2, 4):
            inside(b[k], a[k], a[k + 1])
    rng = np.random.default_rng(N)
    r2, var = np.exp2(rng.uniform(-40, 40, (B, N, T))), np.exp2(rng.uniform(-12, 12, (B, N, T)))
    r2[0, 0, :8] = (pr.EPS / 2) ** 2
    for contrast in (0, 1, 2):
        for flooring in (NOF, MAXF, ADDF):
            a, b = pr.iva_weight(r2, var, F, contrast, flooring), \
                pr.iva_weight(r2, var, F, contrast, flooring, dtype=f64)
            inside(b[0], a[0], a[1])
        if contrast < 2:
            ref, bar = pr.iva_loss_data(r2, var, F, contrast)
            inside(pr.iva_loss_data(r2, var, F, contrast, dtype=f64)[0], ref, bar)
    slots = rng.standard_normal((17, 30)) * np.exp2(rng.uniform(-20, 20, (17, 30)))
    ref, bar = pr.fold_scalar_slots(slots)
    inside(pr.fold_scalar_slots(slots, dtype=f64)[0], ref, bar)


@pytest.mark.parametrize("N,K,model,domain", [(3, 12, MODELS[0][0], 2.0), (4, 12, MODELS[7][0], 2.0),
                                              (6, 7, MODELS[0][0], 2.0), (9, 7, MODELS[0][0], 2.0),
                                              (3, 33, MODELS[0][0], 2.0), (3, 12, MODELS[8][0], 1.0)])
def test_fused_composition_in_float64(N, K, model, domain):
    """The composed update in float64 stays inside the elementwise bars of basis and activation, and
    its inputs are well conditioned."""
    F, T = 17, 40 if N <= 6 else 64
    X, W, basis, act, C = pr.gen_fused_inputs(300 + 2 + N + K, 2, N, F, T, K)
    ref = pr.ilrma_ip1_update(X, C, W, basis, act, domain, model, False, MAXF)
    got = pr.ilrma_ip1_update(X, C, W, basis, act, domain, model, False, MAXF, dtype=np.float64)
    assert ref["kappa"].max() <= 1e3
    inside(got["basis"], ref["basis"], ref["bar_basis"])
    inside(got["activation"], ref["activation"], ref["bar_activation"])
    assert pr.ip1_row_error(got["W"], ref["W"], ref["kappa"]) < 50


# ------------------------------------------------------------------------------- generators
def test_generators_are_deterministic_and_in_range():
    X = pr.gen_spectrogram(3, 2, 3, 17, 40)
    assert np.array_equal(X, pr.gen_spectrogram(3, 2, 3, 17, 40))
    mag = np.abs(X)
    assert mag.min() >= 2.0 ** -20 and mag.max() <= 2.0 ** 20
    assert np.mean(mag < 2.0 ** -10) > 0.15 and np.mean(mag > 2.0 ** 10) > 0.15  # small entries exist
    basis, act = pr.gen_nmf(3, 2, 3, 17, 40, 12)
    for a in (basis, act):
        assert a.min() >= 2.0 ** -12 and a.max() <= 2.0 ** 12 and np.mean(a < 2.0 ** -6) > 0.15
    W = pr.gen_filters(3, 2, 17, 4)
    rows = np.linalg.norm(W, axis=-1)
    Q = W / rows[..., None]
    assert np.allclose(Q @ Q.conj().swapaxes(-1, -2), np.eye(4), atol=1e-12)
    assert rows.min() >= 2.0 ** -8 and rows.max() <= 2.0 ** 8


@pytest.mark.parametrize("N", [2, 3, 4, 6, 8, 9, 16])
def test_ip1_inputs_are_well_conditioned(N):
    W, Uc = pr.gen_ip1_inputs(80 + N + 2, 2, 17, N)
    _, kappa = pr.update_by_ip1(W, Uc, MAXF)
    assert kappa.max() <= 1e3


def test_guard_bands():
    a = np.arange(12.0).reshape(3, 4) + 1j
    flat, n = pr.with_nan_band(a)
    assert n == 24 and flat.size == n + pr.BAND and np.all(np.isnan(flat[n:]))
    assert np.array_equal(flat[:n].view(np.complex128).reshape(3, 4), a)
    buf = pr.sentinel_buffer(24, fill=a)
    assert buf.size == 24 + 2 * pr.BAND and pr.bands_intact(buf)
    assert np.array_equal(buf[pr.BAND:pr.BAND + 24].view(np.complex128).reshape(3, 4), a)
    for k in (0, pr.BAND - 1, pr.BAND + 24, buf.size - 1):
        bad = buf.copy()
        bad[k] = 0.0
        assert not pr.bands_intact(bad)
