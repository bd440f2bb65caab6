"""WPD on the device against the NumPy restatement (tests/wpd_numpy.py): end to end within bars taken
from the restatement's own sensitivity (profiles/wpd_sensitivity.txt), one iteration at a time
against extended precision within bars derived from the operation counts, taps = 0 against the MVDR
filter of the beamformers, the steering form's constraint, routes, launches, batches and repeat runs
bit for bit, containers, apply, the failure paths and the composition with a mask estimator."""

import functools

import numpy as np
import pytest

import wpd_cases
import wpd_numpy

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
N_ITER = 3

# profiles/wpd_sensitivity.txt (benchmarks/tools/wpd_sensitivity.py): 1000 x how far the restatement
# itself moves under a 1e-15 relative perturbation of the input, per shape and form:
# (output, convolutional_filter, loss (relative))
BARS = {
    (1, 1, 1, 1, 1, 8, 1): ((2.8e-12, 1.0e-12, 6.2e-12), (2.8e-12, 1.0e-12, 1.1e-11)),
    (2, 3, 1, 2, 3, 40, 1): ((6.0e-09, 3.1e-09, 1.1e-10), (2.3e-09, 9.8e-10, 4.4e-11)),
    (3, 4, 3, 3, 2, 97, 2): ((1.2e-09, 5.2e-10, 2.9e-10), (1.6e-09, 7.6e-10, 2.7e-11)),
    (4, 10, 3, 2, 3, 257, 1): ((1.5e-08, 8.6e-09, 3.0e-10), (4.3e-09, 3.1e-09, 2.8e-11)),
    (8, 7, 2, 2, 2, 300, 1): ((4.5e-09, 2.2e-09, 4.3e-10), (3.1e-09, 1.7e-09, 1.6e-10)),
    (2, 16, 3, 1, 2, 1700, 1): ((5.9e-10, 4.0e-10, 1.2e-09), (4.0e-11, 2.6e-11, 2.0e-12)),
    (4, 0, 1, 4, 3, 33, 1): ((3.8e-10, 1.4e-10, 5.5e-11), (3.6e-10, 1.4e-10, 1.8e-11)),
    (2, 1, 1, 16, 1, 20, 1): ((3.0e-11, 1.2e-11, 3.1e-12), (1.2e-09, 4.7e-10, 1.8e-11)),
}
# the same file, row "composition": WPD(taps=3, delay=1), 3 iterations, on (3, 5, 64) with two masks
# held fixed: 1000 x the movement of the output
COMPOSITION_CASE = (3, 3, 1, 2, 5, 64, 1)
COMPOSITION_BAR = 8.5e-09


def _wpd(case, **kwargs):
    from ssspy_amd.beamform import WPD

    return WPD(taps=case[1], delay=case[2], **kwargs)


@functools.lru_cache(maxsize=None)
def _data(case):
    arrays = (wpd_cases.make_mixture(case), wpd_cases.make_mask(case), wpd_cases.make_steering(case))
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _form(case, steering):
    X, mask, V = _data(case)
    return {"steering_vector": V} if steering else {"mask": mask}


@functools.lru_cache(maxsize=None)
def _reference(case, steering=False):
    return wpd_numpy.run(_data(case)[0], taps=case[1], delay=case[2], n_iter=N_ITER,
                         **_form(case, steering))


def _run(case, steering=False, X=None, form=None, n_iter=N_ITER, **kwargs):
    m = _wpd(case, **kwargs)
    Y = m(_data(case)[0] if X is None else X, n_iter=n_iter,
          **(_form(case, steering) if form is None else form))
    return Y, np.array(m.convolutional_filter), [np.array(v) for v in m.loss or ()]


@functools.lru_cache(maxsize=None)
def _device_run(case, steering=False):
    return _run(case, steering)


def _rel(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64) - 1).max()


def _same_bits(a, b):
    (Ya, Wa, la), (Yb, Wb, lb) = a, b
    assert np.array_equal(Ya, Yb)
    assert np.array_equal(Wa, Wb)
    assert len(la) == len(lb) and all(np.array_equal(x, y) for x, y in zip(la, lb))


# ---- parity with the restatement
@pytest.mark.parametrize("steering", (False, True), ids=("mask", "steering"))
@pytest.mark.parametrize("case", wpd_cases.CASES, ids=wpd_cases.case_id)
def test_parity_with_restatement(case, steering):
    ref = _reference(case, steering)
    Y, W, loss = _device_run(case, steering)
    out_bar, filter_bar, loss_bar = BARS[case][int(steering)]
    M, K, _, N, F, T, B = case
    lead = (B,) if B > 1 else ()
    assert ref["failed"] == 0
    assert Y.shape == lead + (N, F, T) and Y.dtype == np.complex128
    assert W.shape == lead + (F, N, K + 1, M)
    assert len(loss) == N_ITER + 1
    figures = (np.abs(Y - ref["output"]).max(), np.abs(W - ref["convolutional_filter"]).max(),
               _rel(loss, ref["loss"]))
    print("wpd parity {} {}: output {:.2e} (bar {:.1e}), filter {:.2e} (bar {:.1e}), loss {:.2e} "
          "(bar {:.1e})".format(case, "steering" if steering else "mask", figures[0], out_bar,
                                figures[1], filter_bar, figures[2], loss_bar))
    assert figures[0] <= out_bar
    assert figures[1] <= filter_bar
    assert figures[2] <= loss_bar


def test_signal_covariance_is_the_masked_covariance():
    from ssspy_amd.beamform import WPD, masked_covariance

    case = wpd_cases.CASES[2]
    X, mask, _ = _data(case)
    m = WPD(taps=case[1], delay=case[2])
    m(X, mask, n_iter=1)
    Phi = np.array(m.signal_covariance)
    M, _, _, N, F, _, B = case
    assert Phi.shape == (B, F, N, M, M)
    assert np.abs(Phi - masked_covariance(X, mask)).max() <= 64 * EPS * np.abs(Phi).max()
    assert np.abs(Phi - _reference(case)["signal_covariance"]).max() <= 1e-12


def test_route_of_every_shape():
    """Every shape but the one with 1700 frames keeps the slab in LDS; all within 160 KiB."""
    from ssspy_amd import _lib, _ops

    for case in wpd_cases.CASES:
        M, K, _, N, F, T, B = case
        route, lds = _ops.wpd_route(B, M, N, F, T, K)
        expected = _lib.WPD_ROUTE_STREAMING if T == 1700 else _lib.WPD_ROUTE_RESIDENT
        assert route == expected, case
        assert 0 < lds <= 160 * 1024
    with pytest.raises(ValueError):
        _ops.wpd_route(1, 8, 2, 3, 100, 8)  # (taps + 1) M = 72


# ---- one iteration, against extended precision
def _extended_step(case, seed):
    """One iteration of the mask form from a random filter in longdouble, per (mixture, bin, source),
    and the magnitudes the error bars are made of."""
    M, K, D, N, F, T, B = case
    Lb = (K + 1) * M
    X = np.asarray(_data(case)[0]).reshape(B, M, F, T)
    mask = np.asarray(_data(case)[1]).reshape(B, N, F, T)
    rng = np.random.default_rng(seed)
    W = 0.3 * (rng.standard_normal((B, F, N, Lb)) + 1j * rng.standard_normal((B, F, N, Lb)))
    out = {"X": X, "mask": mask, "W": W}
    for key, shape in (("lambda", (B, F, N, T)), ("R", (B, F, N, Lb, Lb)), ("Phi", (B, F, N, M, M))):
        out[key] = np.zeros(shape, dtype=np.longdouble if key == "lambda" else np.clongdouble)
        out["d" + key] = np.zeros(shape, dtype=np.longdouble)
    ld = np.longdouble
    for b in range(B):
        for f in range(F):
            Xf = X[b, :, f, :].astype(np.clongdouble)
            xb = wpd_numpy.stack(Xf, K, D)
            for n in range(N):
                Wf = W[b, f, n].astype(np.clongdouble)
                y = Wf @ xb
                # y: a sum of Lb complex terms, 4 real operations each
                dy = 4 * (Lb + 2) * EPS * (np.abs(Wf) @ np.abs(xb))
                lam, _ = wpd_numpy.power(y, wpd_numpy.MAX_FLOOR)
                # lambda: the square of |y| (2 |y| dy + dy^2) and its three operations
                dlam = 2 * np.abs(y) * dy + dy ** 2 + 4 * EPS * lam
                R = wpd_numpy.weighted_covariance(xb, lam, wpd_numpy.LOADING)
                # R: (1 / T) times a sum of T terms a conj(b) / lambda: c T eps sum |terms| with c = 8 for
                # the reciprocal, the scaling and the complex product, plus what dlambda moves, plus
                # the scaling by 1 / T; the loading adds its share of the errors of the diagonal and
                # the Lb additions of the trace
                wabs = np.abs(xb) / lam
                spread = np.abs(xb) * (dlam / lam ** 2)
                dR = (8 * T * EPS * (wabs @ np.abs(xb).T) + spread @ np.abs(xb).T) / T \
                    + 4 * EPS * np.abs(R)
                tr = np.trace(np.abs(R)).real
                dR = dR + np.eye(Lb) * ld(wpd_numpy.LOADING) * (
                    np.trace(dR) / Lb + (Lb + 4) * EPS * tr / Lb)
                # Phi_s: a sum of T terms m a conj(b) (c = 8 as above) over a sum of T weights
                m = mask[b, n, f].astype(ld)
                Phi = wpd_numpy.masked_covariance(Xf, m)
                a = max(m.sum(), ld(wpd_numpy.EPS))
                dPhi = 8 * T * EPS * ((np.abs(Xf) * m) @ np.abs(Xf).T) / a + (T + 4) * EPS * np.abs(Phi)
                out["lambda"][b, f, n], out["dlambda"][b, f, n] = lam, dlam
                out["R"][b, f, n], out["dR"][b, f, n] = R, dR
                out["Phi"][b, f, n], out["dPhi"][b, f, n] = Phi, dPhi
    return out


@pytest.mark.parametrize("case", wpd_cases.SMALL, ids=wpd_cases.case_id)
def test_step_statistics_elementwise(case):
    """lambda, R, Phi_s and the Cholesky factor of ssspy_wpd_step, every entry, from a random filter:
    pins the zero history of the first D + K - 1 frames and the tile edges."""
    from ssspy_amd import _device as dv
    from ssspy_amd import _lib, _ops

    M, K, D, N, F, T, B = case
    Lb = (K + 1) * M
    ext = _extended_step(case, seed=5)
    Xd = dv.to_device(ext["X"], dtype=np.complex128)
    md = dv.to_device(ext["mask"], dtype=np.float64)
    Wd = dv.to_device(ext["W"], dtype=np.complex128)
    info = dv.zeros((2,), dv.i32)
    _, lam, R, Phi, U = _ops.wpd_step(Xd, md, None, Wd, K, D, 0, wpd_numpy.LOADING,
                                      (_lib.FLOOR_MAX, 1e-6), info, want_statistics=True)
    assert info.tolist() == [0, 0]
    lam, R, Phi, U = (dv.to_host(t) for t in (lam, R, Phi, U))
    for name, got in (("lambda", lam), ("R", R), ("Phi", Phi)):
        err = np.abs(got - ext[name])
        worst = float((err / ext["d" + name]).max())
        print("wpd step {} {}: max error / bar {:.3f}".format(case, name, worst))
        assert np.all(err <= ext["d" + name]), name
    assert np.array_equal(R, np.conj(np.swapaxes(R, -1, -2)))
    assert np.array_equal(Phi, np.conj(np.swapaxes(Phi, -1, -2)))
    # the factor: upper triangular, real positive diagonal, and U^H U = R up to the backward error of
    # a Cholesky factorisation, |U^H U - R| <= gamma_{Lb+1} |U|^T |U| (Higham, th. 10.3), with 8 real
    # operations per complex multiply-add
    assert np.all(np.tril(U, -1) == 0)
    diag = np.diagonal(U, axis1=-2, axis2=-1)
    assert np.all(diag.imag == 0) and np.all(diag.real > 0)
    Ue, Re = U.astype(np.clongdouble), R.astype(np.clongdouble)
    residual = np.abs(np.conj(np.swapaxes(Ue, -1, -2)) @ Ue - Re)
    bar = 8 * (Lb + 1) * EPS * (np.swapaxes(np.abs(Ue), -1, -2) @ np.abs(Ue))
    print("wpd step {} factor: max residual / bar {:.3f}".format(case, float((residual / bar).max())))
    assert np.all(residual <= bar)


def test_taps_zero_is_the_mvdr_filter_on_phi_s_and_r():
    """taps = 0: the new filter of one iteration is ssspy_beamform_filter(Phi_s, Phi_v = R, MVDR) on
    the Phi_s and the R the iteration hands out, within the filter bar of the shape."""
    from ssspy_amd import _device as dv
    from ssspy_amd import _lib, _ops

    case = wpd_cases.CASES[6]
    M, K, D, N, F, T, B = case
    assert K == 0
    X, mask, _ = _data(case)
    Xd = dv.to_device(X[None], dtype=np.complex128)
    md = dv.to_device(mask[None], dtype=np.float64)
    rng = np.random.default_rng(8)
    W0 = 0.3 * (rng.standard_normal((B, F, N, M)) + 1j * rng.standard_normal((B, F, N, M)))
    Wd = dv.to_device(W0, dtype=np.complex128)
    info = dv.zeros((2,), dv.i32)
    _, _, R, Phi, _ = _ops.wpd_step(Xd, md, None, Wd, 0, D, 1, wpd_numpy.LOADING,
                                    (_lib.FLOOR_MAX, 1e-6), info, want_statistics=True)
    mvdr = _ops.beamform_filter(Phi, R, _lib.BEAMFORM_MVDR, 1, info=info)
    assert info.tolist() == [0, 0]
    worst = np.abs(dv.to_host(Wd) - dv.to_host(mvdr)).max()
    bar = BARS[case][0][1]
    print("wpd taps = 0 against the MVDR filter: {:.2e} (bar {:.1e})".format(worst, bar))
    assert not np.array_equal(dv.to_host(Wd), W0)
    assert worst <= bar


@pytest.mark.parametrize("case", (wpd_cases.CASES[2], wpd_cases.CASES[4]), ids=wpd_cases.case_id)
def test_steering_form_is_distortionless_on_the_device(case):
    """wb[:M]^H v = v_ref: the quotient cancels but for the roundings of the M products, their sum,
    one division and one product."""
    M = case[0]
    ref = M - 1
    V = _data(case)[2]
    _, W, _ = _run(case, steering=True, n_iter=2, reference_id=-1, record_loss=False)
    got = np.sum(W[..., 0, :] * V, axis=-1)
    scale = np.sum(np.abs(W[..., 0, :]) * np.abs(V), axis=-1)
    worst = float((np.abs(got - V[..., ref]) / (EPS * scale)).max())
    print("wpd constraint {}: {:.2f} eps (bar {} eps)".format(case, worst, 4 * (M + 4)))
    assert worst <= 4 * (M + 4)


# ---- bit for bit: routes, launches, batches, repeat runs
@pytest.mark.parametrize("steering", (False, True), ids=("mask", "steering"))
@pytest.mark.parametrize("case", (wpd_cases.CASES[2], wpd_cases.CASES[5]), ids=wpd_cases.case_id)
def test_one_launch_against_one_launch_per_iteration(case, steering):
    seen = []
    run = _run(case, steering, callbacks=lambda method: seen.append(len(method.loss)))
    assert seen == [1, 2, 3, 4]
    _same_bits(_device_run(case, steering), run)


@pytest.mark.parametrize("steering", (False, True), ids=("mask", "steering"))
@pytest.mark.parametrize("case", (wpd_cases.CASES[1], wpd_cases.CASES[3], wpd_cases.CASES[6]),
                         ids=wpd_cases.case_id)
def test_slab_in_lds_against_reread(case, steering):
    from ssspy_amd import _routes

    with _routes.override(wpd_resident=False):
        streamed = _run(case, steering)
    _same_bits(_device_run(case, steering), streamed)


def test_batch_equals_single_runs_and_runs_repeat():
    case = wpd_cases.CASES[2]
    X, mask, _ = _data(case)
    Y, W, loss = _device_run(case)
    for b in range(case[6]):
        single = _run(case, X=X[b], form={"mask": mask[b]})
        _same_bits((Y[b], W[b], [v[b] for v in loss]), single)
    _same_bits(_device_run(case), _run(case))


# ---- containers
def test_device_tensors_in_device_tensor_out():
    import torch

    case = wpd_cases.CASES[1]
    X, mask, V = _data(case)
    Xd = torch.from_numpy(np.array(X)).to("cuda")
    for steering, form in ((False, {"mask": torch.from_numpy(np.array(mask)).to("cuda")}),
                           (True, {"steering_vector": torch.from_numpy(np.array(V)).to("cuda")})):
        m = _wpd(case)
        Yd = m(Xd, n_iter=N_ITER, **form)
        assert isinstance(Yd, torch.Tensor) and Yd.is_cuda and Yd.dtype == torch.complex128
        Y, W, loss = _device_run(case, steering)
        assert tuple(Yd.shape) == Y.shape
        assert np.array_equal(Yd.cpu().numpy(), Y)
        assert np.array_equal(np.array(m.convolutional_filter), W)
    with pytest.raises(ValueError):
        _wpd(case)(Xd, torch.from_numpy(np.array(mask, dtype=np.float32)).to("cuda"))
    # any real dtype of a NumPy mask
    Y32, _, _ = _run(case, form={"mask": np.asarray(mask, dtype=np.float32)})
    Y64, _, _ = _run(case, form={"mask": np.asarray(mask, dtype=np.float32).astype(np.float64)})
    assert np.array_equal(Y32, Y64)


def test_injected_filter_continues_a_run():
    from ssspy_amd.beamform import WPD

    case = wpd_cases.CASES[2]
    X, mask, _ = _data(case)
    first = WPD(taps=case[1], delay=case[2])
    first(X, mask, n_iter=2)
    given = np.array(first.convolutional_filter)
    kept = given.copy()
    second = WPD(taps=case[1], delay=case[2])
    Y = second(X, mask, n_iter=1, convolutional_filter=given)
    assert np.array_equal(given, kept)  # (copied, not overwritten)
    Y3, W3, loss3 = _device_run(case)
    assert np.array_equal(Y, Y3) and np.array_equal(np.array(second.convolutional_filter), W3)
    assert all(np.array_equal(a, b) for a, b in zip(first.loss + second.loss[1:], loss3))
    assert np.array_equal(second.loss[0], first.loss[-1])


def test_apply_on_another_spectrogram():
    from ssspy_amd.beamform import WPD

    case = wpd_cases.CASES[2]
    M, K, D, N, F, T, B = case
    X, mask, _ = _data(case)
    m = WPD(taps=K, delay=D, record_loss=False)
    Y = m(X, mask, n_iter=2)
    assert np.array_equal(m.apply(X), Y)
    other = wpd_cases.make_mixture((M, K, D, N, F, 61, B), seed=4)
    got = m.apply(other)
    W = np.array(m.convolutional_filter).reshape(B, F, N, (K + 1) * M)
    assert got.shape == (B, N, F, 61)
    for b in range(B):
        for f in range(F):
            xb = wpd_numpy.stack(other[b, :, f, :], K, D)
            want = W[b, f] @ xb
            bar = 4 * ((K + 1) * M + 2) * EPS * (np.abs(W[b, f]) @ np.abs(xb))
            assert np.all(np.abs(got[b, :, f, :] - want) <= bar)
    with pytest.raises(ValueError):
        m.apply(other[:, :2])


# ---- failure paths: ordinary error returns
def test_too_few_frames_without_loading_is_singular():
    """T = 3 < Lb = 8 and the last block of the stacked vector is zero in every frame: without
    loading every (bin, source) meets a pivot that is not positive."""
    case = wpd_cases.CASES[1]
    X, mask, _ = _data(case)
    X, mask = np.array(X[:, :, :3]), np.array(mask[:, :, :3])
    for callbacks, record_loss in ((None, True), (None, False), (lambda method: None, True),
                                   (lambda method: None, False)):
        m = _wpd(case, diagonal_loading=0.0, callbacks=callbacks, record_loss=record_loss)
        # (a triple counts once, however many launches the call makes)
        with pytest.raises(np.linalg.LinAlgError, match=r"of 6 \(mixture, bin, source\)"):
            m(X, mask, n_iter=3)
        out = np.asarray(m.output)
        assert np.all(np.isfinite(out))
        assert np.array_equal(out, np.broadcast_to(X[0], out.shape))  # (the start filter e_ref)
    Y = _wpd(case)(X, mask, n_iter=2)  # (with the default loading the same call goes through)
    assert np.all(np.isfinite(Y))


def test_loss_record_after_a_failed_pivot_holds_the_kept_state():
    """ssspy_wpd_steps on the singular input above: every (bin, source) fails in iteration 0, keeps
    the start filter, and the loss term of that state fills entries 1 .. n_steps of the record, as the
    restatement adds the kept filter's loss to every later entry."""
    from ssspy_amd import _device as dv
    from ssspy_amd import _lib, _ops

    case = wpd_cases.CASES[1]
    M, K, D, N, F, _, _ = case
    X, mask, _ = _data(case)
    X, mask = np.array(X[:, :, :3]), np.array(mask[:, :, :3])
    Xd = dv.to_device(X[None], dtype=np.complex128)
    md = dv.to_device(mask[None], dtype=np.float64)
    W = np.zeros((1, F, N, (K + 1) * M), dtype=np.complex128)
    W[..., 0] = 1
    Wd = dv.to_device(W, dtype=np.complex128)
    info = dv.zeros((2,), dv.i32)
    n_steps = 3
    slots = dv.zeros((F * N, n_steps + 1), dv.f64)
    _ops.wpd_steps(Xd, md, None, Wd, K, D, 0, 0.0, (_lib.FLOOR_MAX, 1e-6), n_steps, info,
                   loss_data=slots, slot_stride=n_steps + 1)
    assert info.tolist() == [F * N, 0]
    assert np.array_equal(dv.to_host(Wd), W)
    got = dv.to_host(slots)
    assert np.all(np.isfinite(got)) and np.all(got != 0)
    assert all(np.array_equal(got[:, s], got[:, 0]) for s in range(1, n_steps + 1))
    ref = wpd_numpy.run(X, mask, K, D, n_iter=n_steps, loading=0.0)
    assert ref["failed"] == F * N
    # (a few roundings per frame term; a logarithm near zero is off by eps absolutely, not relatively)
    bar = 256 * EPS * (np.abs(got).sum(axis=0) + F * N)
    assert np.all(np.abs(got.sum(axis=0) - np.asarray(ref["loss"])) <= bar)


def test_all_zero_mask_gives_zeros_without_an_error():
    case = wpd_cases.CASES[1]
    X, mask, _ = _data(case)
    mask = np.array(mask)
    mask[1] = 0
    m = _wpd(case)
    Y = m(X, mask, n_iter=2)
    assert np.all(Y[1] == 0) and np.all(np.array(m.convolutional_filter)[:, 1] == 0)
    assert np.any(Y[0] != 0) and np.all(np.isfinite(m.loss))
    ref = wpd_numpy.run(X, mask, case[1], case[2], n_iter=2)
    assert np.abs(Y - ref["output"]).max() <= BARS[case][0][0]


# ---- composition with a mask estimator
def test_cacgmm_in_front_of_wpd():
    from ssspy_amd.bss.cacgmm import CACGMM

    case = COMPOSITION_CASE
    M, K, D, N, F, T, _ = case
    X = wpd_cases.make_mixture(case)
    cacgmm = CACGMM(n_sources=N, rng=np.random.default_rng(0))
    cacgmm(X, n_iter=5)
    posterior = np.array(cacgmm.posterior)
    assert posterior.shape == (N, F, T)
    Y = _wpd(case)(X, posterior, n_iter=N_ITER)
    ref = wpd_numpy.run(X, posterior, K, D, n_iter=N_ITER)
    worst = np.abs(Y - ref["output"]).max()
    print("cacgmm + wpd {}: {:.2e} (bar {:.1e})".format(case, worst, COMPOSITION_BAR))
    assert worst <= COMPOSITION_BAR
