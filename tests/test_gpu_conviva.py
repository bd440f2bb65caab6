"""ConvIVA on the device against the NumPy restatement (tests/conviva_numpy.py): end to end within
bars taken from the restatement's own sensitivity (profiles/conviva_sensitivity.txt), the statistics
kernel alone against extended precision within bars derived from the operation counts, taps = 0
against AuxIVA-IP1 on the device, the loss, routes, launches, batches and repeat runs bit for bit,
containers, apply and the failure path."""

import functools

import numpy as np
import pytest

import conviva_cases
import conviva_numpy
import wpd_numpy

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
N_ITER = conviva_cases.N_ITER

# profiles/conviva_sensitivity.txt (benchmarks/tools/conviva_sensitivity.py): 1000 x how far the
# restatement itself moves under a 1e-15 relative perturbation of the input, per shape and contrast:
# (output, convolutional_filter, loss (relative))
BARS = {
    (2, 1, 1, 2, 24, 1): ((4.4e-12, 1.0e-12, 1.0e-12), (5.2e-12, 2.2e-12, 3.6e-12)),
    (3, 4, 3, 2, 97, 2): ((8.9e-12, 1.5e-12, 1.2e-12), (5.9e-10, 2.5e-10, 6.1e-12)),
    (4, 10, 3, 3, 257, 1): ((1.2e-11, 4.9e-12, 1.3e-12), (1.7e-11, 1.0e-11, 1.3e-12)),
    (8, 7, 2, 3, 300, 1): ((1.2e-11, 7.4e-12, 2.3e-12), (8.9e-11, 6.5e-11, 8.7e-12)),
    (2, 16, 3, 2, 1700, 1): ((1.2e-11, 1.7e-12, 1.0e-12), (1.2e-11, 2.9e-12, 1.6e-12)),
    (4, 0, 1, 3, 33, 1): ((6.6e-12, 2.3e-12, 1.0e-12), (7.4e-12, 3.8e-12, 1.0e-12)),
}
# (2, 3, 1): L = 6 and block 3 of the stacked vector is zero in each of 3 frames
SINGULAR_CASE = (2, 3, 1, 3, 3, 1)


def _cls(contrast):
    from ssspy_amd.bss import ConvGaussIVA, ConvLaplaceIVA

    return {"laplace": ConvLaplaceIVA, "gauss": ConvGaussIVA}[contrast]


def _method(case, contrast, **kwargs):
    return _cls(contrast)(taps=case[1], delay=case[2], **kwargs)


@functools.lru_cache(maxsize=None)
def _data(case):
    X = conviva_cases.make_mixture(case)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _reference(case, contrast):
    return conviva_numpy.run(_data(case), case[1], case[2], n_iter=N_ITER, contrast=contrast)


def _run(case, contrast, X=None, n_iter=N_ITER, **kwargs):
    m = _method(case, contrast, **kwargs)
    Y = m(_data(case) if X is None else X, n_iter=n_iter)
    return Y, np.array(m.convolutional_filter), [np.array(v) for v in m.loss or ()]


@functools.lru_cache(maxsize=None)
def _device_run(case, contrast):
    return _run(case, contrast)


def _rel(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64) - 1).max()


def _same_bits(a, b):
    (Ya, Wa, la), (Yb, Wb, lb) = a, b
    assert np.array_equal(Ya, Yb)
    assert np.array_equal(Wa, Wb)
    assert len(la) == len(lb) and all(np.array_equal(x, y) for x, y in zip(la, lb))


# ---- parity with the restatement
@pytest.mark.parametrize("contrast", conviva_cases.CONTRASTS)
@pytest.mark.parametrize("case", conviva_cases.CASES, ids=conviva_cases.case_id)
def test_parity_with_restatement(case, contrast):
    ref = _reference(case, contrast)
    Y, W, loss = _device_run(case, contrast)
    out_bar, filter_bar, loss_bar = BARS[case][conviva_cases.CONTRASTS.index(contrast)]
    M, K, _, F, T, B = case
    lead = (B,) if B > 1 else ()
    assert ref["failed"] == 0
    assert Y.shape == lead + (M, F, T) and Y.dtype == np.complex128
    assert W.shape == lead + (F, M, K + 1, M)
    assert len(loss) == N_ITER + 1
    figures = (np.abs(Y - ref["output"]).max(), np.abs(W - ref["convolutional_filter"]).max(),
               _rel(loss, ref["loss"]))
    print("conviva parity {} {}: output {:.2e} (bar {:.1e}), filter {:.2e} (bar {:.1e}), loss {:.2e} "
          "(bar {:.1e})".format(case, contrast, figures[0], out_bar, figures[1], filter_bar,
                                figures[2], loss_bar))
    assert figures[0] <= out_bar
    assert figures[1] <= filter_bar
    assert figures[2] <= loss_bar


def test_filters_of_a_call():
    """demix_filter is block 0 of the convolutional filter; prediction_filter is G of the last
    iteration in WPE's layout, within the filter bar of the shape."""
    case = conviva_cases.CASES[1]
    M, K, D, F, T, B = case
    ref = _reference(case, "laplace")
    m = _method(case, "laplace")
    m(_data(case), n_iter=N_ITER)
    W = np.array(m.convolutional_filter)
    assert np.array_equal(m.demix_filter, W[..., 0, :])
    G = m.prediction_filter
    assert G.shape == (B, F, M, K, M, M)
    assert np.abs(G - ref["prediction_filter"]).max() <= BARS[case][0][1]
    assert repr(m) == ("ConvLaplaceIVA(taps=4, delay=3, diagonal_loading=0.0, scale_restoration=True, "
                       "record_loss=True, reference_id=0)")


def test_route_of_every_shape():
    """Every shape but the one with 1700 frames keeps the slab in LDS; all within 160 KiB."""
    from ssspy_amd import _lib, _ops

    for case in conviva_cases.CASES:
        M, K, _, F, T, B = case
        route, lds = _ops.conviva_route(B, M, F, T, K)
        expected = _lib.CONVIVA_ROUTE_STREAMING if T == 1700 else _lib.CONVIVA_ROUTE_RESIDENT
        assert route == expected, case
        assert 0 < lds <= 160 * 1024
    with pytest.raises(ValueError):
        _ops.conviva_route(1, 8, 3, 100, 8)  # (taps + 1) M = 72
    with pytest.raises(ValueError):
        _ops.conviva_route(1, 1, 3, 100, 2)  # one channel


def test_launch_function_checks_its_arguments():
    from ssspy_amd import _device as dv
    from ssspy_amd import _ops

    info = dv.zeros((2,), dv.i32)
    for M, K, D, error in ((8, 8, 1, NotImplementedError), (9, 0, 1, NotImplementedError),
                           (1, 2, 1, NotImplementedError), (2, 1, 0, ValueError)):
        X = dv.zeros((1, M, 2, 16), dv.c128)
        phi = dv.zeros((1, M, 16), dv.f64)
        with pytest.raises(error):
            _ops.conviva_statistics(X, phi, K, D, 0.0, info)


# ---- the statistics kernel alone, against extended precision
def _extended_statistics(case, seed, loading):
    """Rb, G and Sigma of every (mixture, bin, source) from random positive weights in longdouble,
    and the magnitudes the error bars are made of."""
    M, K, D, F, T, B = case
    L, Lb = K * M, (K + 1) * M
    X = np.asarray(_data(case)).reshape(B, M, F, T)
    rng = np.random.default_rng(seed)
    phi = rng.uniform(0.2, 5.0, (B, M, T))
    out = {"X": X, "phi": phi}
    for key, shape in (("Rb", (B, F, M, Lb, Lb)), ("G", (B, F, M, L, M)), ("Sigma", (B, F, M, M, M))):
        out[key] = np.zeros(shape, dtype=np.clongdouble)
        out["d" + key] = np.zeros(shape, dtype=np.longdouble)
    ld = np.longdouble
    for b in range(B):
        for f in range(F):
            xb = wpd_numpy.stack(X[b, :, f, :].astype(np.clongdouble), K, D)
            for n in range(M):
                w = phi[b, n].astype(ld)
                Sigma, G, st = conviva_numpy.statistics(xb, w, M, loading, True)
                Rb = st["Rb"]
                # Rb: (1 / T) times a sum of T terms phi a conj(b): c T eps sum |terms| with c = 8 for the
                # scaling and the complex product, plus the scaling by 1 / T; the loading adds its
                # share of the errors of the diagonal and the L additions of the trace
                dRb = 8 * T * EPS * ((np.abs(xb) * w) @ np.abs(xb).T) / T + 4 * EPS * np.abs(Rb)
                if L:
                    tr = np.trace(np.abs(Rb[M:, M:])).real
                    dRb[M:, M:] += np.eye(L) * ld(loading) * (
                        np.trace(dRb[M:, M:]) / L + (L + 4) * EPS * tr / L)
                    # G = R^-1 P: the perturbations dR and dP pass through |R^-1|, and the solve by
                    # Cholesky is backward stable, |dR'| <= 8 (3 L + 1) eps |U|^T |U| (Higham, th. 10.4,
                    # with 8 real operations per complex multiply-add)
                    Rinv = np.abs(wpe_solve_identity(st["U"]))
                    Uabs = np.abs(st["U"])
                    dR = dRb[M:, M:] + 8 * (3 * L + 1) * EPS * (Uabs.T @ Uabs)
                    dG = Rinv @ (dRb[M:, :M] + dR @ np.abs(G)) + 4 * EPS * np.abs(G)
                    # Sigma = C - P^H G: the L products and sums, and what dP and dG move
                    P = np.abs(Rb[M:, :M])
                    dSigma = dRb[:M, :M] + dRb[M:, :M].T @ np.abs(G) + P.T @ dG \
                        + 8 * (L + 2) * EPS * (np.abs(Rb[:M, :M]) + P.T @ np.abs(G))
                    out["G"][b, f, n], out["dG"][b, f, n] = G, dG
                else:
                    dSigma = dRb
                out["Rb"][b, f, n], out["dRb"][b, f, n] = Rb, dRb
                out["Sigma"][b, f, n], out["dSigma"][b, f, n] = Sigma, dSigma
    return out


def wpe_solve_identity(U):
    """R^-1 from its Cholesky factor, in U's dtype."""
    import wpe_numpy

    return wpe_numpy.solve_cholesky(U, np.eye(U.shape[0], dtype=U.dtype))


@pytest.mark.parametrize("loading", (0.0, 1e-3))
@pytest.mark.parametrize("case", conviva_cases.SMALL, ids=conviva_cases.case_id)
def test_statistics_elementwise(case, loading):
    """Rb, G, Sigma and the Cholesky factor of ssspy_conviva_statistics, every entry, from random
    positive weights: pins the zero history of the first D + K - 1 frames and the tile edges."""
    from ssspy_amd import _device as dv
    from ssspy_amd import _ops

    M, K, D, F, T, B = case
    L = K * M
    ext = _extended_statistics(case, seed=5, loading=loading)
    Xd = dv.to_device(ext["X"], dtype=np.complex128)
    pd = dv.to_device(ext["phi"], dtype=np.float64)
    info = dv.zeros((2,), dv.i32)
    Sigma, G, failed, Rb, U = _ops.conviva_statistics(Xd, pd, K, D, loading, info,
                                                      want_statistics=True)
    assert info.tolist() == [0, 0] and not failed.any().item()
    Sigma, G, Rb, U = (dv.to_host(t) for t in (Sigma, G, Rb, U))
    for name, got in (("Rb", Rb), ("G", G), ("Sigma", Sigma)):
        err = np.abs(got - ext[name])
        worst = float((err / ext["d" + name]).max()) if err.size else 0.0
        print("conviva statistics {} loading {} {}: max error / bar {:.3f}".format(
            case, loading, name, worst))
        assert np.all(err <= ext["d" + name]), name
    assert np.array_equal(Rb, np.conj(np.swapaxes(Rb, -1, -2)))
    assert np.array_equal(Sigma, np.conj(np.swapaxes(Sigma, -1, -2)))
    assert np.all(np.diagonal(Sigma, axis1=-2, axis2=-1).imag == 0)
    # the factor: upper triangular, real positive diagonal, and U^H U = R up to the backward error of
    # a Cholesky factorisation, |U^H U - R| <= gamma_{L+1} |U|^T |U| (Higham, th. 10.3), with 8 real
    # operations per complex multiply-add
    assert np.all(np.tril(U, -1) == 0)
    diag = np.diagonal(U, axis1=-2, axis2=-1)
    assert np.all(diag.imag == 0) and np.all(diag.real > 0)
    Ue, Re = U.astype(np.clongdouble), Rb[..., M:, M:].astype(np.clongdouble)
    residual = np.abs(np.conj(np.swapaxes(Ue, -1, -2)) @ Ue - Re)
    bar = 8 * (L + 1) * EPS * (np.swapaxes(np.abs(Ue), -1, -2) @ np.abs(Ue))
    print("conviva statistics {} factor: max residual / bar {:.3f}".format(
        case, float((residual / bar).max())))
    assert np.all(residual <= bar)


def test_compose_forms_the_convolutional_filter():
    """W = conj([q; -G q]) from random Q and G: L products and sums per entry."""
    from ssspy_amd import _device as dv
    from ssspy_amd import _ops

    B, F, M, K = 2, 3, 3, 4
    L = K * M
    rng = np.random.default_rng(3)
    Q = rng.standard_normal((B, F, M, M)) + 1j * rng.standard_normal((B, F, M, M))
    G = rng.standard_normal((B, F, M, L, M)) + 1j * rng.standard_normal((B, F, M, L, M))
    failed = np.zeros((B, F, M), dtype=np.int32)
    failed[1, 2, 1] = 3
    W = dv.to_device(np.full((B, F, M, L + M), 7.0 + 0j), dtype=np.complex128)
    _ops.conviva_compose(dv.to_device(Q), dv.to_device(G), W, K, dv.to_device(failed))
    W = dv.to_host(W)
    want = np.concatenate([Q, -np.einsum("bfnlm,bfnm->bfnl", np.conj(G), Q)], axis=-1)
    bar = 4 * (M + 2) * EPS * np.concatenate(
        [np.abs(Q), np.einsum("bfnlm,bfnm->bfnl", np.abs(G), np.abs(Q))], axis=-1)
    keep = failed.astype(bool)
    assert np.all(W[keep] == 7.0)
    assert np.all(np.abs(W - want)[~keep] <= bar[~keep])


# ---- taps = 0 is AuxIVA-IP1
@pytest.mark.parametrize("contrast", conviva_cases.CONTRASTS)
def test_taps_zero_against_auxiva_ip1_on_the_device(contrast):
    """With taps = 0 Sigma is the weighted covariance of AuxIVA and the sweep is the same kernel, but
    the covariance is summed by another kernel in another order (frames in order in one thread here,
    tiles folded there): not bitwise, within the filter bar of the shape."""
    from ssspy_amd.bss.iva import AuxGaussIVA, AuxLaplaceIVA

    case = conviva_cases.CASES[5]
    assert case[1] == 0
    X = _data(case)
    Y, W, loss = _device_run(case, contrast)
    aux = {"laplace": AuxLaplaceIVA, "gauss": AuxGaussIVA}[contrast](spatial_algorithm="IP")
    Ya = aux(X, n_iter=N_ITER)
    bar = BARS[case][conviva_cases.CONTRASTS.index(contrast)][1]
    figures = (np.abs(Y - Ya).max(), np.abs(W[..., 0, :] - np.array(aux.demix_filter)).max(),
               _rel(loss, aux.loss))
    print("conviva taps = 0 against AuxIVA {}: output {:.2e}, filter {:.2e}, loss {:.2e} (bar {:.1e})"
          .format(contrast, *figures, bar))
    assert max(figures) <= bar


# ---- the loss
@pytest.mark.parametrize("contrast", conviva_cases.CONTRASTS)
@pytest.mark.parametrize("case", conviva_cases.CASES, ids=conviva_cases.case_id)
def test_loss_is_non_increasing_on_the_device(case, contrast):
    """(the 3 iterations of the parity run: the Gauss model on few bins overfits beyond that)"""
    _, _, loss = _device_run(case, contrast)
    loss = np.asarray(loss)
    print("conviva loss {} {}: {}".format(case, contrast, loss.tolist()))
    assert len(loss) == N_ITER + 1 and np.all(np.isfinite(loss))
    assert np.all(loss[1:] <= loss[:-1] + 1e-12 * np.abs(loss[:-1]))


def test_apply_after_projection_back_is_the_output():
    case = conviva_cases.CASES[1]
    m = _method(case, "laplace", record_loss=False, reference_id=1)
    Y = m(_data(case), n_iter=2)
    assert np.array_equal(m.apply(_data(case)), Y)
    assert np.array_equal(np.asarray(m.output), Y)


# ---- bit for bit: launches, routes, batches, repeat runs
@pytest.mark.parametrize("contrast", conviva_cases.CONTRASTS)
@pytest.mark.parametrize("case", (conviva_cases.CASES[1], conviva_cases.CASES[4]),
                         ids=conviva_cases.case_id)
def test_one_sequence_against_update_once_with_callbacks(case, contrast):
    seen = []
    run = _run(case, contrast, callbacks=lambda method: seen.append(len(method.loss)))
    assert seen == [1, 2, 3, 4]
    _same_bits(_device_run(case, contrast), run)


@pytest.mark.parametrize("case", (conviva_cases.CASES[0], conviva_cases.CASES[2],
                                  conviva_cases.CASES[5]), ids=conviva_cases.case_id)
def test_slab_in_lds_against_reread(case):
    from ssspy_amd import _routes

    with _routes.override(conviva_resident=False):
        streamed = _run(case, "laplace")
    _same_bits(_device_run(case, "laplace"), streamed)


def test_batch_equals_single_runs_and_runs_repeat():
    case = conviva_cases.CASES[1]
    X = _data(case)
    for contrast in conviva_cases.CONTRASTS:
        Y, W, loss = _device_run(case, contrast)
        for b in range(case[5]):
            _same_bits((Y[b], W[b], [v[b] for v in loss]), _run(case, contrast, X=X[b]))
        _same_bits(_device_run(case, contrast), _run(case, contrast))


# ---- containers
def test_device_tensor_in_device_tensor_out():
    import torch

    case = conviva_cases.CASES[0]
    Xd = torch.from_numpy(np.array(_data(case))).to("cuda")
    m = _method(case, "gauss")
    Yd = m(Xd, n_iter=N_ITER)
    assert isinstance(Yd, torch.Tensor) and Yd.is_cuda and Yd.dtype == torch.complex128
    Y, W, loss = _device_run(case, "gauss")
    assert tuple(Yd.shape) == Y.shape
    assert np.array_equal(Yd.cpu().numpy(), Y)
    assert np.array_equal(np.array(m.convolutional_filter), W)
    Ad = m.apply(Xd)
    assert isinstance(Ad, torch.Tensor) and np.array_equal(Ad.cpu().numpy(), Y)
    with pytest.raises(ValueError):
        _method(case, "gauss")(Xd.to(torch.complex64))


def test_injected_filter_continues_a_run():
    case = conviva_cases.CASES[1]
    X = _data(case)
    first = _method(case, "laplace", scale_restoration=False)
    first(X, n_iter=2)
    given = np.array(first.convolutional_filter)
    kept = given.copy()
    second = _method(case, "laplace", scale_restoration=False)
    Y = second(X, n_iter=1, convolutional_filter=given)
    assert np.array_equal(given, kept)  # (copied, not overwritten)
    Y3, W3, loss3 = _run(case, "laplace", scale_restoration=False)
    assert np.array_equal(Y, Y3) and np.array_equal(np.array(second.convolutional_filter), W3)
    assert all(np.array_equal(a, b) for a, b in zip(first.loss + second.loss[1:], loss3))
    assert np.array_equal(second.loss[0], first.loss[-1])
    with pytest.raises(ValueError):
        _method(case, "laplace")(X, n_iter=1, convolutional_filter=given[..., :1, :])


def test_apply_on_another_spectrogram():
    case = conviva_cases.CASES[1]
    M, K, D, F, T, B = case
    m = _method(case, "laplace", record_loss=False)
    m(_data(case), n_iter=2)
    other = conviva_cases.make_mixture((M, K, D, F, 61, B), seed=4)
    got = m.apply(other)
    W = np.array(m.convolutional_filter).reshape(B, F, M, (K + 1) * M)
    assert got.shape == (B, M, F, 61)
    for b in range(B):
        for f in range(F):
            xb = wpd_numpy.stack(other[b, :, f, :], K, D)
            want = W[b, f] @ xb
            bar = 4 * ((K + 1) * M + 2) * EPS * (np.abs(W[b, f]) @ np.abs(xb))
            assert np.all(np.abs(got[b, :, f, :] - want) <= bar)
    with pytest.raises(ValueError):
        m.apply(other[:, :2])


# ---- the failure path: an ordinary error return
def test_too_few_frames_without_loading_is_singular():
    """T = 3 < L = 6 and the last block of the stacked vector is zero in every frame: without loading
    every (bin, source) meets a pivot that is not positive."""
    case = SINGULAR_CASE
    M, K, D, F, T, B = case
    X = conviva_cases.make_mixture(case)
    for contrast in conviva_cases.CONTRASTS:
        for callbacks, record_loss in ((None, True), (None, False), (lambda method: None, True)):
            m = _method(case, contrast, callbacks=callbacks, record_loss=record_loss)
            # (a triple counts once, however many launches the call makes)
            with pytest.raises(np.linalg.LinAlgError,
                               match=r"of 6 of 6 \(mixture, bin, source\)"):
                m(X, n_iter=3)
            out = np.asarray(m.output)
            assert np.all(np.isfinite(out))
            assert np.array_equal(out, X)  # (every row kept: the start filter)
    ref = conviva_numpy.run(X, K, D, n_iter=3)
    assert ref["failed"] == F * M
    Y = _method(case, "laplace", diagonal_loading=1e-6)(X, n_iter=2)
    assert np.all(np.isfinite(Y))
