"""WPE on the device against the NumPy restatement (tests/wpe_numpy.py): end to end within bars taken
from the restatement's own sensitivity (profiles/wpe_sensitivity.txt), one entry point at a time
against extended precision within bars derived from the operation counts, the routes against each
other, batches, containers, the failure paths and the composition with a separator."""

import functools

import numpy as np
import pytest

import wpe_cases
import wpe_numpy

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
N_ITER = 3

# profiles/wpe_sensitivity.txt (benchmarks/tools/wpe_sensitivity.py): 1000 x how far the restatement
# itself moves under a 1e-15 relative perturbation of the input, per shape:
# (output, prediction_filter, loss (relative))
BARS = {
    (1, 1, 1, 1, 8, 1): (2.8e-12, 8.9e-14, 1.3e-11),
    (2, 3, 1, 3, 40, 1): (6.7e-11, 3.3e-11, 7.7e-12),
    (3, 5, 3, 2, 97, 2): (2.1e-10, 1.2e-10, 7.1e-11),
    (4, 10, 3, 3, 257, 1): (3.2e-11, 2.3e-11, 4.4e-13),
    (8, 8, 2, 2, 300, 1): (1.3e-11, 9.3e-12, 4.4e-13),
    (2, 16, 3, 2, 1700, 1): (1.1e-11, 1.1e-11, 5.6e-13),
}
# the same file, row "composition": GaussILRMA(n_basis=2), 3 iterations, behind WPE(taps=3, delay=1),
# 2 iterations, on (2, 9, 64): 1000 x the movement of the separated spectrograms
COMPOSITION_CASE = (2, 3, 1, 9, 64, 1)
COMPOSITION_BAR = 9.1e-12


def _wpe(**kwargs):
    from ssspy_amd.dereverb import WPE

    return WPE(**kwargs)


@functools.lru_cache(maxsize=None)
def _mixture(case):
    X = wpe_cases.make_mixture(case)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _reference(case):
    return wpe_numpy.run(_mixture(case), case[1], case[2], n_iter=N_ITER)


@functools.lru_cache(maxsize=None)
def _device_run(case):
    m = _wpe(taps=case[1], delay=case[2])
    Y = m(_mixture(case), n_iter=N_ITER)
    return Y, np.array(m.prediction_filter), [np.array(v) for v in m.loss]


def _rel(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64) - 1).max()


# ---- parity with the restatement
@pytest.mark.parametrize("case", wpe_cases.CASES, ids=wpe_cases.case_id)
def test_parity_with_restatement(case):
    ref = _reference(case)
    Y, G, loss = _device_run(case)
    out_bar, filter_bar, loss_bar = BARS[case]
    M, K, _, F, T, B = case
    assert Y.shape == ref["output"].shape and Y.dtype == np.complex128
    assert G.shape == ((B,) if B > 1 else ()) + (F, K, M, M)
    assert len(loss) == N_ITER + 1
    figures = (np.abs(Y - ref["output"]).max(), np.abs(G - ref["prediction_filter"]).max(),
               _rel(loss, ref["loss"]))
    print("wpe parity {}: output {:.2e} (bar {:.1e}), filter {:.2e} (bar {:.1e}), loss {:.2e} "
          "(bar {:.1e})".format(case, figures[0], out_bar, figures[1], filter_bar, figures[2], loss_bar))
    assert figures[0] <= out_bar
    assert figures[1] <= filter_bar
    assert figures[2] <= loss_bar


def test_route_of_every_shape():
    """The first five shapes keep the slab in LDS, the last one re-reads it; all within 160 KiB."""
    from ssspy_amd import _lib, _ops

    for case in wpe_cases.CASES:
        M, K, _, F, T, B = case
        route, lds = _ops.wpe_route(B, M, F, T, K)
        expected = _lib.WPE_ROUTE_STREAMING if case == wpe_cases.CASES[-1] else _lib.WPE_ROUTE_RESIDENT
        assert route == expected, case
        assert 0 < lds <= 160 * 1024


# ---- one entry point at a time, against extended precision
def _extended_step(case, seed):
    """One iteration from a random filter in longdouble, per (mixture, bin), and the magnitudes the
    error bars are made of."""
    M, K, D, F, T, B = case
    L = K * M
    X = np.asarray(_mixture(case)).reshape(B, M, F, T)
    rng = np.random.default_rng(seed)
    G = 0.1 * (rng.standard_normal((B, F, L, M)) + 1j * rng.standard_normal((B, F, L, M)))
    out = {"X": X, "G": G}
    for key, shape in (("Y", (B, M, F, T)), ("dY", (B, M, F, T)), ("lambda", (B, F, T)),
                       ("dlambda", (B, F, T)), ("R", (B, F, L, L)), ("dR", (B, F, L, L)),
                       ("P", (B, F, L, M)), ("dP", (B, F, L, M))):
        out[key] = np.zeros(shape, dtype=np.clongdouble if key in "YRP" else np.longdouble)
    for b in range(B):
        for f in range(F):
            Xf = X[b, :, f, :].astype(np.clongdouble)
            Gf = G[b, f].astype(np.clongdouble)
            xs = wpe_numpy.stack_history(Xf, K, D)
            Yf = wpe_numpy.apply_filter(Xf, Gf, K, D)
            # y: a sum of L + 1 complex terms, 4 real operations each
            dy = 4 * (L + 2) * EPS * (np.abs(Xf) + np.abs(Gf).T @ np.abs(xs))
            _, st = wpe_numpy.bin_step(Xf, Gf, K, D, wpe_numpy.MAX_FLOOR, True)
            lam = st["lambda"]
            # lambda: M squares of y (2 |y| dy + dy^2 each), their sum and the division by M
            dlam = np.sum(2 * np.abs(Yf) * dy + dy ** 2, axis=0) / M + 4 * (M + 2) * EPS * lam
            # R, P: sums of T terms a conj(b) / lambda; c * T * eps * sum |terms| with c = 8 for the
            # reciprocal, the scaling and the complex product, plus what dlambda moves
            wabs = np.abs(xs) / lam
            spread = np.abs(xs) * (dlam / lam ** 2)
            out["Y"][b, :, f, :], out["dY"][b, :, f, :] = Yf, dy
            out["lambda"][b, f], out["dlambda"][b, f] = lam, dlam
            out["R"][b, f], out["P"][b, f] = st["R"], st["P"]
            out["dR"][b, f] = 8 * T * EPS * (wabs @ np.abs(xs).T) + spread @ np.abs(xs).T
            out["dP"][b, f] = 8 * T * EPS * (wabs @ np.abs(Xf).T) + spread @ np.abs(Xf).T
    return out


@pytest.mark.parametrize("case", wpe_cases.SMALL, ids=wpe_cases.case_id)
def test_step_statistics_elementwise(case):
    """lambda, R, P and the Cholesky factor of ssspy_wpe_step, every entry, from a random filter: pins
    the zero history of the first D + K - 1 frames and the tile edges."""
    from ssspy_amd import _device as dv
    from ssspy_amd import _lib, _ops

    M, K, D, F, T, B = case
    L = K * M
    ext = _extended_step(case, seed=5)
    Xd = dv.to_device(ext["X"], dtype=np.complex128)
    Gd = dv.to_device(ext["G"], dtype=np.complex128)
    info = dv.zeros((2,), dv.i32)
    _, lam, R, P, U = _ops.wpe_step(Xd, Gd, K, D, (_lib.FLOOR_MAX, 1e-10), info, want_statistics=True)
    assert info.tolist() == [0, 0]
    lam, R, P, U = (dv.to_host(t) for t in (lam, R, P, U))
    for name, got in (("lambda", lam), ("R", R), ("P", P)):
        err = np.abs(got - ext[name])
        worst = float((err / ext["d" + name]).max())
        print("wpe step {} {}: max error / bar {:.3f}".format(case, name, worst))
        assert np.all(err <= ext["d" + name]), name
    # the factor: upper triangular, real positive diagonal, and U^H U = R up to the backward error of
    # a Cholesky factorisation, |U^H U - R| <= gamma_{L+1} |U|^T |U| (Higham, th. 10.3), with 8 real
    # operations per complex multiply-add
    assert np.all(np.tril(U, -1) == 0)
    diag = np.diagonal(U, axis1=-2, axis2=-1)
    assert np.all(diag.imag == 0) and np.all(diag.real > 0)
    Ue, Re = U.astype(np.clongdouble), R.astype(np.clongdouble)
    residual = np.abs(np.conj(np.swapaxes(Ue, -1, -2)) @ Ue - Re)
    bar = 8 * (L + 1) * EPS * (np.swapaxes(np.abs(Ue), -1, -2) @ np.abs(Ue))
    print("wpe step {} factor: max residual / bar {:.3f}".format(case, float((residual / bar).max())))
    assert np.all(residual <= bar)


@pytest.mark.parametrize("case", wpe_cases.SMALL, ids=wpe_cases.case_id)
def test_apply_elementwise(case):
    from ssspy_amd import _device as dv
    from ssspy_amd import _ops

    ext = _extended_step(case, seed=6)
    Xd = dv.to_device(ext["X"], dtype=np.complex128)
    Gd = dv.to_device(ext["G"], dtype=np.complex128)
    Y = dv.to_host(_ops.wpe_apply(Xd, Gd, case[1], case[2]))
    err = np.abs(Y - ext["Y"])
    print("wpe apply {}: max error / bar {:.3f}".format(case, float((err / ext["dY"]).max())))
    assert np.all(err <= ext["dY"])
    assert np.array_equal(dv.to_host(Gd), ext["G"])  # (the filter is read, not written)


# ---- the routes agree
def _all_close(a, b, tol=1e-12):
    (Ya, Ga, la), (Yb, Gb, lb) = a, b
    assert np.abs(Ya - Yb).max() <= tol
    assert np.abs(Ga - Gb).max() <= tol
    assert _rel(la, lb) <= tol


@pytest.mark.parametrize("case", (wpe_cases.CASES[2], wpe_cases.CASES[5]), ids=wpe_cases.case_id)
def test_one_launch_against_one_launch_per_iteration(case):
    seen = []
    m = _wpe(taps=case[1], delay=case[2], callbacks=lambda method: seen.append(len(method.loss)))
    Y = m(_mixture(case), n_iter=N_ITER)
    assert seen == [1, 2, 3, 4]
    _all_close(_device_run(case), (Y, np.array(m.prediction_filter), m.loss))


@pytest.mark.parametrize("case", (wpe_cases.CASES[1], wpe_cases.CASES[3]), ids=wpe_cases.case_id)
def test_slab_in_lds_against_reread(case):
    from ssspy_amd import _routes

    with _routes.override(wpe_resident=False):
        m = _wpe(taps=case[1], delay=case[2])
        Y = m(_mixture(case), n_iter=N_ITER)
        streamed = (Y, np.array(m.prediction_filter), m.loss)
    _all_close(_device_run(case), streamed)


# ---- batches
def test_batch_equals_single_runs_and_runs_repeat():
    case = wpe_cases.CASES[2]
    X = _mixture(case)
    Y, G, loss = _device_run(case)
    for b in range(case[5]):
        m = _wpe(taps=case[1], delay=case[2])
        Yb = m(X[b], n_iter=N_ITER)
        _all_close((Y[b], G[b], [v[b] for v in loss]), (Yb, np.array(m.prediction_filter), m.loss))
    m = _wpe(taps=case[1], delay=case[2])
    Y2 = m(X, n_iter=N_ITER)
    assert np.array_equal(Y2, Y) and np.array_equal(np.array(m.prediction_filter), G)
    assert all(np.array_equal(a, b) for a, b in zip(m.loss, loss))


# ---- containers
def test_device_tensor_in_device_tensor_out():
    import torch

    case = wpe_cases.CASES[1]
    Xd = torch.from_numpy(np.array(_mixture(case))).to("cuda")
    m = _wpe(taps=case[1], delay=case[2])
    Yd = m(Xd, n_iter=N_ITER)
    assert isinstance(Yd, torch.Tensor) and Yd.is_cuda and Yd.dtype == torch.complex128
    assert tuple(Yd.shape) == _mixture(case).shape
    assert np.array_equal(Yd.cpu().numpy(), _device_run(case)[0])


def test_injected_filter_continues_a_run():
    case = wpe_cases.CASES[2]
    X = _mixture(case)
    first = _wpe(taps=case[1], delay=case[2])
    first(X, n_iter=2)
    given = np.array(first.prediction_filter)
    kept = given.copy()
    second = _wpe(taps=case[1], delay=case[2])
    Y = second(X, n_iter=1, prediction_filter=given)
    assert np.array_equal(given, kept)  # (copied, not overwritten)
    Y3, G3, loss3 = _device_run(case)
    assert np.array_equal(Y, Y3) and np.array_equal(np.array(second.prediction_filter), G3)
    assert all(np.array_equal(a, b) for a, b in zip(first.loss + second.loss[1:], loss3))
    assert np.array_equal(second.loss[0], first.loss[-1])


# ---- failure paths: ordinary error returns
def test_delay_past_the_frames_is_singular():
    X = np.array(_mixture(wpe_cases.CASES[1]))[:, :, :8]
    for delay in (8, 50):
        m = _wpe(taps=2, delay=delay)
        with pytest.raises(np.linalg.LinAlgError, match=r"3 bin"):
            m(X, n_iter=2)
        assert np.all(np.isfinite(np.asarray(m.output)))


def test_silent_channel_is_singular():
    X = np.array(_mixture(wpe_cases.CASES[1]))
    X[1] = 0
    for callbacks in (None, lambda method: None):
        with pytest.raises(np.linalg.LinAlgError):
            _wpe(taps=3, delay=1, callbacks=callbacks)(X, n_iter=2)


def test_limits_raise_as_specified():
    X = np.array(_mixture(wpe_cases.CASES[1]))
    with pytest.raises(NotImplementedError, match="taps"):
        _wpe(taps=13)(np.zeros((5, 2, 30), dtype=np.complex128))
    with pytest.raises(NotImplementedError, match="channels"):
        _wpe(taps=1)(np.zeros((9, 2, 30), dtype=np.complex128))
    with pytest.raises(ValueError):
        _wpe(delay=0)
    with pytest.raises(NotImplementedError):
        _wpe(flooring_fn=lambda x: np.maximum(x, 1e-3))
    m = _wpe(taps=3, delay=1)
    m.flooring_fn = lambda x: np.maximum(x, 1e-3)  # (set behind the constructor's back)
    with pytest.raises(NotImplementedError):
        m(X, n_iter=1)


# ---- composition with a separator
def test_wpe_in_front_of_ilrma():
    from ssspy_amd.bss.ilrma import GaussILRMA

    case = COMPOSITION_CASE
    M, K, D, F, T, _ = case
    X = _mixture(case)
    basis = np.random.default_rng(1).random((M, F, 2))
    activation = np.random.default_rng(2).random((M, 2, T))
    dereverberated = _wpe(taps=K, delay=D)(X, n_iter=2)
    ref = wpe_numpy.run(X, K, D, n_iter=2)["output"]
    Y = GaussILRMA(n_basis=2)(dereverberated, n_iter=3, basis=basis, activation=activation)
    Yr = GaussILRMA(n_basis=2)(ref, n_iter=3, basis=basis, activation=activation)
    worst = np.abs(Y - Yr).max()
    print("wpe + ilrma {}: {:.2e} (bar {:.1e})".format(case, worst, COMPOSITION_BAR))
    assert worst <= COMPOSITION_BAR
