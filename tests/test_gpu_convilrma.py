"""ConvILRMA on the device against the NumPy restatement (tests/convilrma_numpy.py): end to end within
bars taken from the restatement's own sensitivity (profiles/convilrma_sensitivity.txt), the statistics
kernel with the weights formed in the kernel against extended precision within bars derived from the
operation counts, taps = 0 against GaussILRMA-IP1 on the device, routes, launches, batches and repeat
runs bit for bit, the normalisation, containers, apply, injection and the failure path."""

import functools

import numpy as np
import pytest

import convilrma_cases
import convilrma_numpy
import conviva_numpy
import wpd_numpy
import wpe_numpy

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
N_ITER = convilrma_cases.N_ITER

# profiles/convilrma_sensitivity.txt (benchmarks/tools/convilrma_sensitivity.py): 1000 x how far the
# restatement itself moves under a 1e-15 relative perturbation of the input, per shape:
# (output, convolutional_filter, basis (relative), activation (relative), loss (relative))
BARS = {
    (2, 1, 1, 2, 24, 1, 1, 2): (1.5e-11, 6.0e-12, 6.0e-12, 2.7e-12, 2.4e-12),
    (3, 4, 3, 2, 97, 2, 3, 2): (6.1e-12, 1.6e-12, 1.4e-12, 2.9e-12, 1.3e-12),
    (4, 10, 3, 3, 257, 1, 4, 1): (1.0e-11, 6.4e-12, 1.4e-12, 1.7e-12, 1.2e-12),
    (8, 7, 2, 3, 300, 1, 2, 2): (1.2e-11, 5.5e-12, 1.5e-12, 4.8e-12, 4.2e-12),
    (2, 16, 3, 2, 1700, 1, 2, 2): (1.2e-11, 2.0e-12, 1.0e-12, 3.7e-12, 1.0e-12),
    (4, 0, 1, 3, 33, 1, 32, 2): (5.6e-12, 2.0e-12, 1.4e-12, 3.6e-12, 1.0e-12),
}
# (2, 3, 1): L = 6 and block 3 of the stacked vector is zero in each of 3 frames
SINGULAR_CASE = (2, 3, 1, 3, 3, 1)


def _method(case, **kwargs):
    from ssspy_amd.bss import ConvGaussILRMA

    kwargs.setdefault("domain", case[7])
    return ConvGaussILRMA(case[6], taps=case[1], delay=case[2], **kwargs)


@functools.lru_cache(maxsize=None)
def _data(case):
    X = convilrma_cases.make_mixture(case)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _factors(case):
    basis, activation = convilrma_cases.make_factors(case)
    basis.setflags(write=False)
    activation.setflags(write=False)
    return basis, activation


@functools.lru_cache(maxsize=None)
def _reference(case, normalization=True, scale_restoration=True):
    basis, activation = _factors(case)
    return convilrma_numpy.run(_data(case), case[1], case[2], domain=case[7], n_iter=N_ITER,
                               basis=basis, activation=activation, normalization=normalization,
                               scale_restoration=scale_restoration)


def _run(case, X=None, factors=None, n_iter=N_ITER, **kwargs):
    """(output, convolutional_filter, basis, activation, loss) of one call from the case's factors."""
    m = _method(case, **kwargs)
    basis, activation = _factors(case) if factors is None else factors
    Y = m(_data(case) if X is None else X, n_iter=n_iter, basis=basis, activation=activation)
    return (Y, np.array(m.convolutional_filter), np.array(m.basis), np.array(m.activation),
            [np.array(v) for v in m.loss or ()])


@functools.lru_cache(maxsize=None)
def _device_run(case):
    return _run(case)


def _rel(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64) - 1).max()


def _same_bits(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    assert len(a[4]) == len(b[4]) and all(np.array_equal(x, y) for x, y in zip(a[4], b[4]))


def _figures(run, ref):
    Y, W, basis, activation, loss = run
    return (np.abs(Y - ref["output"]).max(), np.abs(W - ref["convolutional_filter"]).max(),
            np.abs(basis - ref["basis"]).max() / np.abs(ref["basis"]).max(),
            np.abs(activation - ref["activation"]).max() / np.abs(ref["activation"]).max(),
            _rel(loss, ref["loss"]))


# ---- parity with the restatement
@pytest.mark.parametrize("case", convilrma_cases.CASES, ids=convilrma_cases.case_id)
def test_parity_with_restatement(case):
    ref = _reference(case)
    run = _device_run(case)
    M, K, _, F, T, B, Kb, _ = case
    lead = (B,) if B > 1 else ()
    assert ref["failed"] == 0
    assert run[0].shape == lead + (M, F, T) and run[0].dtype == np.complex128
    assert run[1].shape == lead + (F, M, K + 1, M)
    assert run[2].shape == lead + (M, F, Kb) and run[3].shape == lead + (M, Kb, T)
    assert len(run[4]) == N_ITER + 1
    figures = _figures(run, ref)
    print("convilrma parity {}: ".format(case) + ", ".join(
        "{} {:.2e} (bar {:.1e})".format(name, got, bar) for name, got, bar in zip(
            ("output", "filter", "basis", "activation", "loss"), figures, BARS[case])))
    for got, bar in zip(figures, BARS[case]):
        assert got <= bar


@pytest.mark.parametrize("case", convilrma_cases.CASES, ids=convilrma_cases.case_id)
def test_loss_is_non_increasing_on_the_device(case):
    loss = np.asarray(_device_run(case)[4])
    print("convilrma loss {}: {}".format(case, loss.tolist()))
    assert len(loss) == N_ITER + 1 and np.all(np.isfinite(loss))
    assert np.all(loss[1:] <= loss[:-1] + 1e-12 * np.abs(loss[:-1]))


def test_route_of_every_shape():
    """The conviva_resident route governs this kernel too: every shape but the one with 1700 frames
    keeps the slab in LDS."""
    from ssspy_amd import _lib, _ops

    for case in convilrma_cases.CASES:
        M, K, _, F, T, B = case[:6]
        route, lds = _ops.conviva_route(B, M, F, T, K)
        expected = _lib.CONVIVA_ROUTE_STREAMING if T == 1700 else _lib.CONVIVA_ROUTE_RESIDENT
        assert route == expected, case
        assert 0 < lds + 8 * case[6] <= 160 * 1024


def test_launch_function_checks_its_arguments():
    from ssspy_amd import _device as dv
    from ssspy_amd import _ops

    info = dv.zeros((2,), dv.i32)
    for M, K, D, Kb, p, error in ((8, 8, 1, 2, 2, NotImplementedError),
                                  (9, 0, 1, 2, 2, NotImplementedError),
                                  (1, 2, 1, 2, 2, NotImplementedError),
                                  (2, 1, 1, 33, 2, NotImplementedError),
                                  (2, 1, 0, 2, 2, ValueError), (2, 1, 1, 2, 0, ValueError),
                                  (2, 1, 1, 2, 2.5, ValueError)):
        X = dv.zeros((1, M, 2, 16), dv.c128)
        basis = dv.zeros((1, M, 2, Kb), dv.f64) + 1.0
        activation = dv.zeros((1, M, Kb, 16), dv.f64) + 1.0
        with pytest.raises(error):
            _ops.conviva_statistics_nmf(X, basis, activation, p, K, D, 0.0, info)


# ---- the statistics kernel alone, against extended precision
def _extended_statistics(case, loading, domain):
    """phi, Rb, G and Sigma of every (mixture, bin, source) from fixed random factors in longdouble,
    and the magnitudes the error bars are made of (those of the ConvIVA statistics test, with the
    rounding of the weights in front)."""
    M, K, D, F, T, B, Kb, _ = case
    L, Lb = K * M, (K + 1) * M
    ld = np.longdouble
    X = np.asarray(_data(case)).reshape(B, M, F, T)
    rng = np.random.default_rng(11)
    basis = rng.uniform(0.2, 2.0, (B, M, F, Kb))
    activation = rng.uniform(0.2, 2.0, (B, M, Kb, T))
    phi = np.stack([convilrma_numpy.weights(basis[b].astype(ld), activation[b].astype(ld), domain)
                    for b in range(B)])
    # the weights: Kb products and Kb - 1 sums of positive terms (Kb eps relative with or without
    # fused multiply-adds), then one division, or pow with an error of its own (bounded in the test
    # below by 8 eps: (Kb + 8) eps)
    phi_eps = (Kb + 2) * EPS if domain == 2 else (Kb + 8) * EPS
    out = {"X": X, "basis": basis, "activation": activation, "phi": phi}
    for key, shape in (("Rb", (B, F, M, Lb, Lb)), ("G", (B, F, M, L, M)), ("Sigma", (B, F, M, M, M))):
        out[key] = np.zeros(shape, dtype=np.clongdouble)
        out["d" + key] = np.zeros(shape, dtype=ld)
    for b in range(B):
        for f in range(F):
            xb = wpd_numpy.stack(X[b, :, f, :].astype(np.clongdouble), K, D)
            for n in range(M):
                w = phi[b, n, f]
                Sigma, G, st = conviva_numpy.statistics(xb, w, M, loading, True)
                Rb = st["Rb"]
                # Rb: (1 / T) times a sum of T terms phi a conj(b): c T eps sum |terms| with c = 8 for
                # the scaling and the complex product, the relative error of the weights on every
                # term, plus the scaling by 1 / T; the loading adds its share of the errors of the
                # diagonal and the L additions of the trace
                dRb = (8 * T * EPS + phi_eps) * ((np.abs(xb) * w) @ np.abs(xb).T) / T \
                    + 4 * EPS * np.abs(Rb)
                if L:
                    tr = np.trace(np.abs(Rb[M:, M:])).real
                    dRb[M:, M:] += np.eye(L) * ld(loading) * (
                        np.trace(dRb[M:, M:]) / L + (L + 4) * EPS * tr / L)
                    # G = R^-1 P: the perturbations dR and dP pass through |R^-1|, and the solve by
                    # Cholesky is backward stable, |dR'| <= 8 (3 L + 1) eps |U|^T |U| (Higham, th. 10.4)
                    Rinv = np.abs(wpe_numpy.solve_cholesky(st["U"], np.eye(L, dtype=st["U"].dtype)))
                    Uabs = np.abs(st["U"])
                    dR = dRb[M:, M:] + 8 * (3 * L + 1) * EPS * (Uabs.T @ Uabs)
                    dG = Rinv @ (dRb[M:, :M] + dR @ np.abs(G)) + 4 * EPS * np.abs(G)
                    P = np.abs(Rb[M:, :M])
                    dSigma = dRb[:M, :M] + dRb[M:, :M].T @ np.abs(G) + P.T @ dG \
                        + 8 * (L + 2) * EPS * (np.abs(Rb[:M, :M]) + P.T @ np.abs(G))
                    out["G"][b, f, n], out["dG"][b, f, n] = G, dG
                else:
                    dSigma = dRb
                out["Rb"][b, f, n], out["dRb"][b, f, n] = Rb, dRb
                out["Sigma"][b, f, n], out["dSigma"][b, f, n] = Sigma, dSigma
    return out


@pytest.mark.parametrize("domain, loading", ((2, 0.0), (2, 1e-3), (1, 0.0)))
@pytest.mark.parametrize("case", convilrma_cases.SMALL, ids=convilrma_cases.case_id)
def test_statistics_elementwise(case, domain, loading):
    """phi, Rb, G, Sigma and the Cholesky factor of ssspy_conviva_statistics_nmf, every entry, from
    fixed random factors."""
    from ssspy_amd import _device as dv
    from ssspy_amd import _ops

    M, K, D, F, T, B, Kb, _ = case
    L = K * M
    ext = _extended_statistics(case, loading, domain)
    Xd = dv.to_device(ext["X"], dtype=np.complex128)
    info = dv.zeros((2,), dv.i32)
    Sigma, G, failed, Rb, U, phi = _ops.conviva_statistics_nmf(
        Xd, dv.to_device(ext["basis"]), dv.to_device(ext["activation"]), domain, K, D, loading, info,
        want_statistics=True)
    assert info.tolist() == [0, 0] and not failed.any().item()
    Sigma, G, Rb, U, phi = (dv.to_host(t) for t in (Sigma, G, Rb, U, phi))
    excess = float((np.abs(phi / ext["phi"] - 1) / EPS).max())
    print("convilrma statistics {} domain {}: phi off by {:.2f} eps (Kb = {})".format(
        case, domain, excess, Kb))
    assert excess <= (Kb + 2 if domain == 2 else Kb + 8)
    for name, got in (("Rb", Rb), ("G", G), ("Sigma", Sigma)):
        err = np.abs(got - ext[name])
        worst = float((err / ext["d" + name]).max()) if err.size else 0.0
        print("convilrma statistics {} domain {} loading {} {}: max error / bar {:.3f}".format(
            case, domain, loading, name, worst))
        assert np.all(err <= ext["d" + name]), name
    assert np.array_equal(Rb, np.conj(np.swapaxes(Rb, -1, -2)))
    assert np.array_equal(Sigma, np.conj(np.swapaxes(Sigma, -1, -2)))
    assert np.all(np.diagonal(Sigma, axis1=-2, axis2=-1).imag == 0)
    # the factor: U^H U = R up to the backward error of a Cholesky factorisation (Higham, th. 10.3)
    assert np.all(np.tril(U, -1) == 0)
    diag = np.diagonal(U, axis1=-2, axis2=-1)
    assert np.all(diag.imag == 0) and np.all(diag.real > 0)
    Ue, Re = U.astype(np.clongdouble), Rb[..., M:, M:].astype(np.clongdouble)
    residual = np.abs(np.conj(np.swapaxes(Ue, -1, -2)) @ Ue - Re)
    bar = 8 * (L + 1) * EPS * (np.swapaxes(np.abs(Ue), -1, -2) @ np.abs(Ue))
    assert np.all(residual <= bar)


def test_statistics_same_bits_on_both_routes_and_in_a_batch():
    from ssspy_amd import _device as dv
    from ssspy_amd import _ops, _routes

    case = convilrma_cases.CASES[1]
    K, D = case[1], case[2]
    ext = _extended_statistics(case, 0.0, 2)
    Xd = dv.to_device(ext["X"], dtype=np.complex128)
    Td, Vd = dv.to_device(ext["basis"]), dv.to_device(ext["activation"])
    info = dv.zeros((2,), dv.i32)

    def stats(X, T, V):
        out = _ops.conviva_statistics_nmf(X, T, V, 2, K, D, 0.0, info, want_statistics=True)
        return [dv.to_host(t) for t in out]

    whole = stats(Xd, Td, Vd)
    with _routes.override(conviva_resident=False):
        streamed = stats(Xd, Td, Vd)
    for a, b in zip(whole, streamed):
        assert np.array_equal(a, b)
    for b in range(case[5]):
        alone = stats(Xd[b:b + 1].contiguous(), Td[b:b + 1].contiguous(), Vd[b:b + 1].contiguous())
        for a, c in zip(whole, alone):
            assert np.array_equal(a[b:b + 1], c)


def test_a_zero_model_takes_the_failure_path():
    """s_t = 0 gives phi = inf: R is not finite and the pivot check fails the triple."""
    from ssspy_amd import _device as dv
    from ssspy_amd import _ops

    case = convilrma_cases.CASES[0]
    M, K, D, F, T, B, Kb, _ = case
    X = dv.to_device(np.asarray(_data(case)).reshape(B, M, F, T), dtype=np.complex128)
    basis = np.ones((B, M, F, Kb))
    basis[0, 1, 0] = 0.0
    info = dv.zeros((2,), dv.i32)
    _, _, failed = _ops.conviva_statistics_nmf(X, dv.to_device(basis),
                                               dv.to_device(np.ones((B, M, Kb, T))), 2, K, D, 0.0,
                                               info)
    want = np.zeros((B, F, M), dtype=np.int32)
    want[0, 0, 1] = 3
    assert np.array_equal(dv.to_host(failed), want) and info.tolist() == [1, 0]


# ---- taps = 0 is GaussILRMA-IP1
def test_taps_zero_against_gauss_ilrma_ip1_on_the_device():
    """With taps = 0 Sigma is the weighted covariance of GaussILRMA and the sweep, the NMF updates and
    the loss are the same kernels, but the covariance is summed by another kernel in another order and
    GaussILRMA updates the factors from W x where this class reads Y: not bitwise, within the bars of
    the shape."""
    from ssspy_amd.bss.ilrma import GaussILRMA

    case = convilrma_cases.CASES[5]
    assert case[1] == 0
    basis, activation = _factors(case)
    run = _device_run(case)
    ilrma = GaussILRMA(case[6], spatial_algorithm="IP1", domain=case[7])
    Y = ilrma(_data(case), n_iter=N_ITER, basis=basis, activation=activation)
    figures = (np.abs(run[0] - Y).max(),
               np.abs(run[1][..., 0, :] - np.array(ilrma.demix_filter)).max(),
               np.abs(run[2] - ilrma.basis).max() / np.abs(ilrma.basis).max(),
               np.abs(run[3] - ilrma.activation).max() / np.abs(ilrma.activation).max(),
               _rel(run[4], ilrma.loss))
    print("convilrma taps = 0 against GaussILRMA-IP1: " + ", ".join(
        "{:.2e} (bar {:.1e})".format(got, bar) for got, bar in zip(figures, BARS[case])))
    for got, bar in zip(figures, BARS[case]):
        assert got <= bar


# ---- the normalisation
@pytest.mark.parametrize("case", (convilrma_cases.CASES[1], convilrma_cases.CASES[2]),
                         ids=convilrma_cases.case_id)
def test_normalisation_sets_unit_power_and_leaves_the_loss(case):
    normed = _run(case, normalization=True, scale_restoration=False)
    plain = _run(case, normalization=False, scale_restoration=False)
    power = np.mean(np.abs(normed[0]) ** 2, axis=(-2, -1))
    rel = _rel(normed[4], plain[4])
    print("convilrma normalisation {}: |mean |y|^2 - 1| {:.2e}, loss {:.2e} (bar {:.1e})".format(
        case, np.abs(power - 1).max(), rel, BARS[case][4]))
    assert np.abs(power - 1).max() <= 1e-12
    assert rel <= BARS[case][4]
    ref = _reference(case, True, False)
    for got, bar in zip(_figures(normed, ref), BARS[case]):
        assert got <= bar


def test_output_is_the_filter_on_the_mixture_after_normalisation():
    """Y and the rows of W take the same psi: apply(input) is the output to the rounding of one
    division per entry on top of the Lb products and sums of the apply."""
    case = convilrma_cases.CASES[1]
    M, K, D, F, T, B, _, _ = case
    m = _method(case, scale_restoration=False, record_loss=False)
    basis, activation = _factors(case)
    Y = m(_data(case), n_iter=2, basis=basis, activation=activation)
    W = np.array(m.convolutional_filter).reshape(B, F, M, (K + 1) * M)
    X = _data(case)
    for b in range(B):
        for f in range(F):
            xb = wpd_numpy.stack(X[b, :, f, :], K, D)
            bar = 4 * ((K + 1) * M + 4) * EPS * (np.abs(W[b, f]) @ np.abs(xb))
            assert np.all(np.abs(Y[b, :, f, :] - W[b, f] @ xb) <= bar)
    assert np.array_equal(np.asarray(m.output), Y)


def test_apply_after_projection_back_is_the_output():
    case = convilrma_cases.CASES[1]
    m = _method(case, record_loss=False, reference_id=1)
    basis, activation = _factors(case)
    Y = m(_data(case), n_iter=2, basis=basis, activation=activation)
    assert np.array_equal(m.apply(_data(case)), Y)
    assert np.array_equal(np.asarray(m.output), Y)
    assert np.array_equal(m.demix_filter, np.array(m.convolutional_filter)[..., 0, :])
    assert m.prediction_filter.shape == (case[5], case[3], case[0], case[1], case[0], case[0])
    assert repr(m) == ("ConvGaussILRMA(n_basis=3, taps=4, delay=3, domain=2, diagonal_loading=0.0, "
                       "normalization=True, scale_restoration=True, record_loss=False, reference_id=1)")


# ---- bit for bit: launches, routes, batches, repeat runs
@pytest.mark.parametrize("case", (convilrma_cases.CASES[1], convilrma_cases.CASES[4]),
                         ids=convilrma_cases.case_id)
def test_one_sequence_against_update_once_with_callbacks(case):
    seen = []
    run = _run(case, callbacks=lambda method: seen.append(len(method.loss)))
    assert seen == [1, 2, 3, 4]
    _same_bits(_device_run(case), run)


@pytest.mark.parametrize("case", (convilrma_cases.CASES[0], convilrma_cases.CASES[2],
                                  convilrma_cases.CASES[5]), ids=convilrma_cases.case_id)
def test_slab_in_lds_against_reread(case):
    from ssspy_amd import _routes

    with _routes.override(conviva_resident=False):
        streamed = _run(case)
    _same_bits(_device_run(case), streamed)


def test_batch_equals_single_runs_and_runs_repeat():
    case = convilrma_cases.CASES[1]
    X = _data(case)
    basis, activation = _factors(case)
    run = _device_run(case)
    for b in range(case[5]):
        single = _run(case, X=X[b], factors=(basis[b], activation[b]))
        _same_bits(tuple(v[b] for v in run[:4]) + ([v[b] for v in run[4]],), single)
    _same_bits(run, _run(case))


# ---- containers and injection
def test_device_tensor_in_device_tensor_out():
    import torch

    case = convilrma_cases.CASES[0]
    basis, activation = _factors(case)
    Xd = torch.from_numpy(np.array(_data(case))).to("cuda")
    m = _method(case)
    Yd = m(Xd, n_iter=N_ITER, basis=basis, activation=activation)
    assert isinstance(Yd, torch.Tensor) and Yd.is_cuda and Yd.dtype == torch.complex128
    run = _device_run(case)
    assert np.array_equal(Yd.cpu().numpy(), run[0])
    assert np.array_equal(np.array(m.convolutional_filter), run[1])
    assert np.array_equal(np.array(m.basis), run[2])
    Ad = m.apply(Xd)
    assert isinstance(Ad, torch.Tensor) and np.array_equal(Ad.cpu().numpy(), run[0])
    with pytest.raises(ValueError):
        _method(case)(Xd.to(torch.complex64))


def test_injected_state_continues_a_run():
    """2 + 1 iterations from the injected filter and factors against 3 in one call.  Not bitwise: the
    second call forms Y = W xb from the normalised rows, where the run in one call carries the Y it
    divided by the same psi, one rounding per entry apart -- a perturbation of the size the bars of
    the shape are made for."""
    case = convilrma_cases.CASES[1]
    X = _data(case)
    basis, activation = _factors(case)
    first = _method(case, scale_restoration=False)
    first(X, n_iter=2, basis=basis, activation=activation)
    given = [np.array(first.convolutional_filter), np.array(first.basis), np.array(first.activation)]
    kept = [v.copy() for v in given]
    second = _method(case, scale_restoration=False)
    Y = second(X, n_iter=1, convolutional_filter=given[0], basis=given[1], activation=given[2])
    assert all(np.array_equal(a, b) for a, b in zip(given, kept))  # (copied, not overwritten)
    whole = _run(case, scale_restoration=False)
    continued = (Y, np.array(second.convolutional_filter), np.array(second.basis),
                 np.array(second.activation), first.loss + second.loss[1:])
    ref = dict(zip(("output", "convolutional_filter", "basis", "activation", "loss"), whole))
    figures = _figures(continued, ref)
    print("convilrma continued run {}: ".format(case) + ", ".join(
        "{:.2e} (bar {:.1e})".format(got, bar) for got, bar in zip(figures, BARS[case])))
    for got, bar in zip(figures, BARS[case]):
        assert got <= bar
    assert all(np.array_equal(a, b) for a, b in zip(first.loss, whole[4][:3]))
    with pytest.raises(ValueError):
        _method(case)(X, n_iter=1, basis=given[1][..., :1])


def test_factors_are_drawn_from_the_generator_basis_first():
    case = convilrma_cases.CASES[0]
    m = _method(case, rng=np.random.default_rng(5), record_loss=False)
    m(_data(case), n_iter=0)
    basis, activation = convilrma_numpy.make_factors(_data(case).shape, case[6],
                                                     np.random.default_rng(5))
    assert np.array_equal(np.array(m.basis), basis)
    assert np.array_equal(np.array(m.activation), activation)


def test_apply_on_another_spectrogram():
    case = convilrma_cases.CASES[1]
    M, K, D, F, T, B, _, _ = case
    m = _method(case, record_loss=False)
    basis, activation = _factors(case)
    m(_data(case), n_iter=2, basis=basis, activation=activation)
    other = convilrma_cases.make_mixture((M, K, D, F, 61, B), seed=4)
    got = m.apply(other)
    W = np.array(m.convolutional_filter).reshape(B, F, M, (K + 1) * M)
    assert got.shape == (B, M, F, 61)
    for b in range(B):
        for f in range(F):
            xb = wpd_numpy.stack(other[b, :, f, :], K, D)
            bar = 4 * ((K + 1) * M + 2) * EPS * (np.abs(W[b, f]) @ np.abs(xb))
            assert np.all(np.abs(got[b, :, f, :] - W[b, f] @ xb) <= bar)


# ---- the failure path: an ordinary error return
def test_too_few_frames_without_loading_is_singular():
    """T = 3 < L = 6 and the last block of the stacked vector is zero in every frame: without loading
    every (bin, source) meets a pivot that is not positive."""
    from ssspy_amd.bss import ConvGaussILRMA

    M, K, D, F, T, B = SINGULAR_CASE
    X = convilrma_cases.make_mixture(SINGULAR_CASE + (2, 2))
    for callbacks, record_loss in ((None, True), (None, False), (lambda method: None, True)):
        m = ConvGaussILRMA(2, taps=K, delay=D, callbacks=callbacks, record_loss=record_loss,
                           rng=np.random.default_rng(0))
        with pytest.raises(np.linalg.LinAlgError, match=r"of 6 of 6 \(mixture, bin, source\)"):
            m(X, n_iter=3)
        assert np.all(np.isfinite(np.asarray(m.output)))
    Y = ConvGaussILRMA(2, taps=K, delay=D, diagonal_loading=1e-6,
                       rng=np.random.default_rng(0))(X, n_iter=2)
    assert np.all(np.isfinite(Y))
