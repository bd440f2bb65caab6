"""Gradient / natural-gradient IVA on the device against the golden vectors of the reference and the
NumPy restatement (tests/grad_iva_numpy.py).

Bars: 1e-8 relative Frobenius on filters and outputs, rtol 1e-9 on loss lists,
1e-10 on the single operator and on batch = single.  The parity runs take 10 iterations (6 above 8
sources): the reference and a restatement through W U W^H differ by 3e-13 there, by 1e-10 after 20
and by 4e-8 after 50 (plain-gradient Gauss IVA amplifies rounding: W^-H, and 1 / alpha has no floor).
"""

import functools

import numpy as np
import pytest

import grad_iva_cases as tg
import grad_iva_numpy as gn
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL, LOSS_RTOL, OP_TOL, BATCH_TOL = 1e-8, 1e-9, 1e-10, 1e-10
NAMED = ["GradLaplaceIVA", "GradGaussIVA", "NaturalGradLaplaceIVA", "NaturalGradGaussIVA"]


def _iva():
    from ssspy_amd.bss import iva

    return iva


def _flooring():
    from ssspy_amd.special import flooring

    return flooring


def _mixture(seed, N, F, T):
    from ssspy_amd.utils.dataset import nmf_mixture

    return nmf_mixture(seed, N, F, T)


@pytest.mark.parametrize("name", tg.CASES)
def test_separators_replay_golden(name):
    g = load_golden(name)
    snap = tg.Snapshots()
    m = getattr(_iva(), str(g["meta_cls"]))(callbacks=snap, **tg.golden_kwargs(g, _flooring()))
    init = tg.golden_init(g)
    Y = m(g["X"], n_iter=int(g["meta_n_iter"]), **init)
    for key in g:
        if key.startswith("it"):
            print(name, key, rel_err(snap.store[key], g[key]))
    print(name, "final", rel_err(np.asarray(m.demix_filter), g["final_demix_filter"]),
          rel_err(Y, g["final_output"]), np.max(np.abs(np.array(m.loss) / g["loss"] - 1)))
    tg.check_against_golden(g, m, Y, snap, TOL, LOSS_RTOL)
    if init:
        assert np.array_equal(init["demix_filter"], g["demix_filter0"])


SHAPES = [(2, 1025, 37), (4, 1, 50), (5, 33, 45), (8, 17, 70), (9, 5, 100), (16, 3, 150)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n{}_f{}_t{}".format(*s))
@pytest.mark.parametrize("holonomic", [True, False], ids=["hol", "nonhol"])
@pytest.mark.parametrize("cls", NAMED)
def test_named_classes_match_restatement(cls, holonomic, shape):
    N, F, T = shape
    n_iter = 10 if N <= 8 else 6
    X = _mixture(500 + N, N, F, T)
    ref = gn.CLASSES[cls](is_holonomic=holonomic)
    Yr = ref(X, n_iter=n_iter)
    m = getattr(_iva(), cls)(is_holonomic=holonomic)
    Y = m(X, n_iter=n_iter)
    print(cls, holonomic, shape, rel_err(m.demix_filter, ref.demix_filter), rel_err(Y, Yr),
          np.max(np.abs(np.array(m.loss) / np.array(ref.loss) - 1)))
    assert rel_err(m.demix_filter, ref.demix_filter) < TOL
    assert rel_err(Y, Yr) < TOL
    np.testing.assert_allclose(m.loss, ref.loss, rtol=LOSS_RTOL)
    if "Gauss" in cls:
        assert rel_err(m.variance, ref.variance) < TOL


@pytest.mark.parametrize("holonomic", [True, False], ids=["hol", "nonhol"])
@pytest.mark.parametrize("cls", NAMED)
def test_batch_of_three_equals_single_runs_and_restatement(cls, holonomic):
    N, F, T = 3, 20, 37
    X = np.stack([_mixture(520 + b, N, F, T) for b in range(3)])
    m = getattr(_iva(), cls)(is_holonomic=holonomic)
    Y = m(X, n_iter=10)
    assert Y.shape == X.shape and np.array(m.loss).shape == (11, 3)
    for b in range(3):
        s = getattr(_iva(), cls)(is_holonomic=holonomic)
        Ys = s(X[b], n_iter=10)
        assert rel_err(Y[b], Ys) < BATCH_TOL
        assert rel_err(m.demix_filter[b], s.demix_filter) < BATCH_TOL
        np.testing.assert_allclose(np.array(m.loss)[:, b], s.loss, rtol=BATCH_TOL)
        ref = gn.CLASSES[cls](is_holonomic=holonomic)
        assert rel_err(Y[b], ref(X[b], n_iter=10)) < TOL
        np.testing.assert_allclose(np.array(m.loss)[:, b], ref.loss, rtol=LOSS_RTOL)


@pytest.mark.parametrize("cls", NAMED)
def test_two_runs_are_bit_identical(cls):
    X = np.stack([_mixture(530 + b, 4, 65, 50) for b in range(2)])
    runs = []
    for _ in range(2):
        m = getattr(_iva(), cls)()
        Y = m(X, n_iter=10)
        runs.append((Y, np.array(m.demix_filter), np.array(m.loss)))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("cls", NAMED)
def test_update_once_by_hand_equals_call(cls):
    X = _mixture(540, 3, 33, 45)
    a = getattr(_iva(), cls)(scale_restoration=False)
    Ya = a(X, n_iter=5)
    b = getattr(_iva(), cls)(scale_restoration=False, record_loss=False)
    b(X, n_iter=0)
    for _ in range(5):
        b.update_once()
    assert rel_err(b.demix_filter, a.demix_filter) < BATCH_TOL
    assert rel_err(b.output, Ya) < BATCH_TOL  # (formed lazily from the filters)
    assert abs(b.compute_loss() / a.loss[-1] - 1) < LOSS_RTOL


@pytest.mark.parametrize("cls", NAMED)
def test_record_loss_with_and_without_callback(cls):
    X = _mixture(550, 4, 33, 45)
    seen = []
    a = getattr(_iva(), cls)(callbacks=lambda method: seen.append(len(method.loss)))
    Ya = a(X, n_iter=10)
    b = getattr(_iva(), cls)()
    Yb = b(X, n_iter=10)
    c = getattr(_iva(), cls)(record_loss=False)
    Yc = c(X, n_iter=10)
    assert seen == list(range(1, 12)) and len(b.loss) == 11 and c.loss is None
    np.testing.assert_allclose(b.loss, a.loss, rtol=LOSS_RTOL)
    assert rel_err(Yb, Ya) < BATCH_TOL and rel_err(Yc, Ya) < BATCH_TOL
    d = getattr(_iva(), cls)()
    d(X, n_iter=10, initial_call=False)
    np.testing.assert_allclose(d.loss, a.loss[1:], rtol=LOSS_RTOL)


@pytest.mark.parametrize("cls", ["GradLaplaceIVA", "NaturalGradLaplaceIVA"])
def test_host_evaluated_floor_equals_kernel_floor(cls):
    X = _mixture(560, 3, 20, 45)
    eps = float(np.median(np.linalg.norm(X, axis=1)))  # (acts on about half of the frames)

    def disguised(x):
        return np.maximum(x, eps)

    a = getattr(_iva(), cls)(flooring_fn=functools.partial(_flooring().max_flooring, eps=eps))
    b = getattr(_iva(), cls)(flooring_fn=disguised)
    Ya, Yb = a(X, n_iter=10), b(X, n_iter=10)
    assert rel_err(Yb, Ya) < BATCH_TOL
    np.testing.assert_allclose(b.loss, a.loss, rtol=LOSS_RTOL)
    ref = gn.CLASSES[cls](flooring_fn=disguised)
    assert rel_err(Yb, ref(X, n_iter=10)) < TOL


@pytest.mark.parametrize("holonomic", [True, False])
@pytest.mark.parametrize("natural", [True, False])
def test_generic_classes_with_closures_equal_named(natural, holonomic):
    iva = _iva()
    X = _mixture(570, 3, 20, 45)
    named = (iva.NaturalGradLaplaceIVA if natural else iva.GradLaplaceIVA)(is_holonomic=holonomic)
    generic = (iva.NaturalGradIVA if natural else iva.GradIVA)(
        contrast_fn=tg.generic_contrast_fn, score_fn=tg.generic_score_fn, is_holonomic=holonomic)
    Yn, Yg = named(X, n_iter=10), generic(X, n_iter=10)
    assert rel_err(Yg, Yn) < TOL
    assert rel_err(generic.demix_filter, named.demix_filter) < TOL
    np.testing.assert_allclose(generic.loss, named.loss, rtol=LOSS_RTOL)


def test_constructor_contract():
    iva = _iva()
    with pytest.raises(ValueError, match="Specify contrast function."):
        iva.GradIVA(score_fn=tg.generic_score_fn)
    with pytest.raises(ValueError, match="Specify score function."):
        iva.NaturalGradIVA(contrast_fn=tg.generic_contrast_fn)
    m = iva.NaturalGradLaplaceIVA()
    assert m.step_size == 0.1 and m.is_holonomic is True
    assert repr(m) == ("GradIVA(step_size=0.1, is_holonomic=True, scale_restoration=True, "
                       "record_loss=True, reference_id=0)")
    assert iva.GradLaplaceIVA(flooring_fn=None).flooring_fn(3.0) == 3.0
    # the defaults of the reference's code (ssspy/bss/iva.py:333, :747, :919): False on the base class,
    # True on GradIVA / NaturalGradIVA (whose docstrings say False)
    closures = dict(contrast_fn=tg.generic_contrast_fn, score_fn=tg.generic_score_fn)
    assert iva.GradIVABase(**closures).is_holonomic is False
    assert iva.GradIVA(**closures).is_holonomic is True
    assert iva.NaturalGradIVA(**closures).is_holonomic is True
    for cls in NAMED:
        assert getattr(iva, cls)().is_holonomic is True


def test_borrowed_closures_take_the_compatibility_path():
    """Closures taken from a named instance read THAT instance's floor / variance: on another
    separator they are user closures (the tag alone must not put them on the device path)."""
    iva = _iva()
    X = _mixture(575, 3, 12, 40)
    eps = float(np.median(np.linalg.norm(X, axis=1)))
    donor = iva.NaturalGradLaplaceIVA(flooring_fn=functools.partial(_flooring().max_flooring, eps=eps))
    borrowed = iva.NaturalGradIVA(contrast_fn=donor.contrast_fn, score_fn=donor.score_fn)
    Yd, Yb = donor(X, n_iter=5), borrowed(X, n_iter=5)
    assert borrowed._score is None and donor._score is not None
    assert rel_err(Yb, Yd) < TOL  # (the donor's floor, not the borrower's default one)


@pytest.mark.parametrize("cls", ["GradGaussIVA", "NaturalGradGaussIVA"])
def test_overridden_source_model_is_called(cls):
    """A subclass's ``update_source_model`` runs before every step, as in the reference, and the
    step takes the variance it leaves."""
    X = _mixture(576, 3, 12, 40)

    class Device(getattr(_iva(), cls)):
        calls = 0

        def update_source_model(self):
            type(self).calls += 1
            super().update_source_model()
            self.variance = 2.0 * np.asarray(self.variance)

    class Restated(gn.CLASSES[cls]):
        def update_source_model(self):
            super().update_source_model()
            self.variance = 2.0 * self.variance

    m, ref = Device(), Restated()
    Y, Yr = m(X, n_iter=5), ref(X, n_iter=5)
    assert Device.calls == 5
    assert rel_err(Y, Yr) < TOL and rel_err(m.variance, ref.variance) < TOL
    np.testing.assert_allclose(m.loss, ref.loss, rtol=LOSS_RTOL)


@pytest.mark.parametrize("restoration,reference_id", [(False, 0), (True, 0), ("projection_back", 2),
                                                      ("minimal_distortion_principle", 1)])
def test_scale_restorations(restoration, reference_id):
    X = _mixture(580, 3, 20, 45)
    kwargs = dict(scale_restoration=restoration, reference_id=reference_id)
    ref = gn.NaturalGradGaussIVA(**kwargs)
    Yr = ref(X, n_iter=10)
    m = _iva().NaturalGradGaussIVA(**kwargs)
    Y = m(X, n_iter=10)
    assert rel_err(Y, Yr) < TOL and rel_err(m.demix_filter, ref.demix_filter) < TOL
    assert rel_err(m.output, Yr) < TOL


def test_singular_injected_filter_raises_linalg_error():
    X = _mixture(590, 3, 8, 40)
    W = np.tile(np.eye(3, dtype=np.complex128), (8, 1, 1))
    W[5, 2] = W[5, 1]  # two equal rows in one bin: an exact zero pivot
    with pytest.raises(np.linalg.LinAlgError):
        _iva().GradLaplaceIVA(record_loss=False)(X, n_iter=2, demix_filter=W)


def test_seventeen_sources_are_refused():
    X = np.random.default_rng(0).standard_normal((17, 2, 40)) + 0j
    with pytest.raises(NotImplementedError, match="16"):
        _iva().NaturalGradLaplaceIVA()(X, n_iter=1)


@pytest.mark.parametrize("N", list(range(2, 17)))
def test_step_operator_against_numpy(N):
    import torch

    from ssspy_amd import _device as dv
    from ssspy_amd import _ops

    B, F, eta = 2, 70, 0.1
    rng = np.random.default_rng(600 + N)

    def crandn(*shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)

    W = np.eye(N) + 0.3 * crandn(B, F, N, N)
    A = crandn(B, F, N, N, 2 * N)
    U = A @ A.conj().swapaxes(-1, -2) / (2 * N)  # Hermitian PSD like weighted covariances
    WH = W.conj().swapaxes(-1, -2)
    P = np.stack([(W @ U[:, :, n] @ WH)[:, :, n, :] for n in range(N)], axis=2)
    eye = np.eye(N)
    slots = _ops.iva_grad_step_logdet_slots(B, F, N)
    for natural in (True, False):
        for holonomic in (True, False):
            D = P - eye if holonomic else (1 - eye) * P
            want = W - eta * (D @ W if natural else D @ np.linalg.inv(W).conj().swapaxes(-1, -2))
            for stats in (U, P):
                Wd = dv.to_device(W, dtype=np.complex128)
                info = dv.zeros((2,), dv.i32)
                shares = dv.zeros((slots, 3 * B), dv.f64, Wd.device)
                _ops.iva_grad_step(Wd, dv.to_device(stats, dtype=np.complex128), natural, holonomic,
                                   eta, info, logdet=shares.reshape(-1)[B:], logdet_stride=3 * B)
                torch.cuda.synchronize()
                assert rel_err(dv.to_host(Wd), want) < OP_TOL, (natural, holonomic, stats.ndim)
                got = dv.to_host(shares)
                assert not got[:, :B].any() and not got[:, 2 * B:].any()  # (only its own entries)
                np.testing.assert_allclose(got[:, B:2 * B].sum(axis=0),
                                           np.linalg.slogdet(W)[1].sum(axis=1), rtol=OP_TOL)
                assert info.tolist() == [0, 0]


def test_score_weight_operator_against_numpy():
    from ssspy_amd import _device as dv
    from ssspy_amd import _lib, _ops

    rng = np.random.default_rng(620)
    r2 = rng.random((2, 3, 37)) * 4
    r2d = dv.to_device(r2, dtype=np.float64)
    for kind, eps, fn in ((_lib.FLOOR_MAX, 1.0, lambda r: np.maximum(r, 1.0)),
                          (_lib.FLOOR_ADD, 0.5, lambda r: r + 0.5), (_lib.FLOOR_NONE, 0.0, lambda r: r)):
        w = _ops.iva_score_weight(r2d, 9, _lib.CONTRAST_LAPLACE, (kind, eps))
        np.testing.assert_allclose(dv.to_host(w), 1 / fn(np.sqrt(r2)), rtol=1e-14)
    var = dv.zeros((2, 3, 37), dv.f64, r2d.device)
    w = _ops.iva_score_weight(r2d, 9, _lib.CONTRAST_GAUSS, (_lib.FLOOR_MAX, 1.0), variance=var)
    np.testing.assert_allclose(dv.to_host(var), r2 / 9, rtol=1e-15)
    np.testing.assert_allclose(dv.to_host(w), 9 / r2, rtol=1e-14)
    given = rng.random((2, 3, 37)) + 0.5
    var = dv.to_device(given, dtype=np.float64)
    w = _ops.iva_score_weight(r2d, 9, _lib.CONTRAST_GAUSS_FIXED, (_lib.FLOOR_NONE, 0.0), variance=var)
    assert np.array_equal(dv.to_host(var), given)
    np.testing.assert_allclose(dv.to_host(w), 1 / given, rtol=1e-14)


def test_bench_shape_loss_falls_over_100_iterations():
    """One mixture of the benchmark shape (4 sources, 1025 bins, 512 frames), 100 iterations of
    NaturalGradLaplaceIVA at the default step: the loss list is finite and ends below where it
    starts (the reference's holonomic runs fall monotonically; no parity is asserted here)."""
    X = _mixture(1000, 4, 1025, 512)
    m = _iva().NaturalGradLaplaceIVA()
    m(X, n_iter=100)
    loss = np.array(m.loss)
    print("loss", loss[0], loss[1], loss[-1])
    assert loss.shape == (101,) and np.isfinite(loss).all()
    assert loss[-1] < loss[0]
