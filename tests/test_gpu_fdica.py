"""FDICA on the device against the golden vectors of the reference and the NumPy restatement
(tests/fdica_numpy.py), on every route: the bin-resident kernel with the slab in LDS, the same kernel
streaming the slab, and the per-iteration operators.

Bars: 1e-8 relative Frobenius on filters and outputs, rtol 1e-9 on loss lists,
1e-10 on single operators, on batch = single and on route = route.  The parity runs take 10
iterations (5 for IP2): per-bin Laplace IP overfits short bins and 1 / |y| amplifies rounding, the
reference itself moves by 1e-7 after 30 iterations of IP1 under a 1e-15 perturbation of its input.
"""

import functools

import numpy as np
import pytest

import fdica_cases as tc
import fdica_numpy as fn
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL, LOSS_RTOL, OP_TOL, BATCH_TOL = 1e-8, 1e-9, 1e-10, 1e-10
# (class, constructor arguments, iterations)
FORMS = [
    ("GradLaplaceFDICA", dict(is_holonomic=True), 10),
    ("GradLaplaceFDICA", dict(is_holonomic=False), 10),
    ("NaturalGradLaplaceFDICA", dict(is_holonomic=True), 10),
    ("NaturalGradLaplaceFDICA", dict(is_holonomic=False), 10),
    ("AuxLaplaceFDICA", dict(spatial_algorithm="IP1"), 10),
    ("AuxLaplaceFDICA", dict(spatial_algorithm="IP2"), 5),
]
FORM_IDS = ["grad_hol", "grad_nonhol", "natgrad_hol", "natgrad_nonhol", "ip1", "ip2"]
KERNEL_FORMS, KERNEL_IDS = FORMS[:5], FORM_IDS[:5]


def _fdica():
    from ssspy_amd.bss import fdica

    return fdica


def _flooring():
    from ssspy_amd.special import flooring

    return flooring


def _mixture(seed, N, F, T):
    from ssspy_amd.utils.dataset import nmf_mixture

    return nmf_mixture(seed, N, F, T)


def _algorithm(cls, kwargs):
    from ssspy_amd import _lib

    if cls.startswith("Aux"):
        return _lib.FDICA_AUX_IP2 if kwargs.get("spatial_algorithm") == "IP2" else _lib.FDICA_AUX_IP1
    return _lib.FDICA_NATURAL_GRAD if cls.startswith("Natural") else _lib.FDICA_GRAD


# 1
@pytest.mark.parametrize("name", tc.CASES)
def test_separators_replay_golden(name):
    g = load_golden(name)
    snap = tc.Snapshots()
    m = getattr(_fdica(), str(g["meta_cls"]))(callbacks=snap, **tc.golden_kwargs(g, _flooring()))
    init = tc.golden_init(g)
    Y = m(g["X"], n_iter=int(g["meta_n_iter"]), **init)
    for key in g:
        if key.startswith("it"):
            print(name, key, rel_err(snap.store[key], g[key]))
    print(name, "final", rel_err(np.asarray(m.demix_filter), g["final_demix_filter"]),
          rel_err(Y, g["final_output"]), np.max(np.abs(np.array(m.loss) / g["loss"] - 1)))
    tc.check_against_golden(g, m, Y, snap, TOL, LOSS_RTOL)
    if init:
        assert np.array_equal(init["demix_filter"], g["demix_filter0"])


@pytest.mark.parametrize("name", tc.CASES)
def test_golden_without_callbacks(name):
    """The same fixtures with nothing looking in between: one launch where the route allows."""
    g = load_golden(name)
    m = getattr(_fdica(), str(g["meta_cls"]))(**tc.golden_kwargs(g, _flooring()))
    Y = m(g["X"], n_iter=int(g["meta_n_iter"]), **tc.golden_init(g))
    print(name, rel_err(np.asarray(m.demix_filter), g["final_demix_filter"]),
          rel_err(Y, g["final_output"]), np.max(np.abs(np.array(m.loss) / g["loss"] - 1)))
    np.testing.assert_allclose(np.array(m.loss), g["loss"], rtol=LOSS_RTOL)
    assert rel_err(np.asarray(m.demix_filter), g["final_demix_filter"]) < TOL
    assert rel_err(Y, g["final_output"]) < TOL


# 2
SHAPES = [(2, 1025, 37), (4, 1, 50), (5, 33, 45), (8, 17, 70), (3, 5, 257), (9, 5, 100),
          (16, 3, 150)]


# The seeds are chosen on the restatement alone, by the fixture generator's criterion: run against
# itself on an input perturbed by 1e-15 relative (three trials, every form) it stays within 1e-10 in
# filters and output, 100x under the bar.  Short bins make some draws ill-conditioned: at seed
# 700 + N the restatement of IP2 moves by 1.8e-8 at (2, 1025, 37), at 1700 + N by 1.3e-7 at
# (5, 33, 45) and IP1 by 2.4e-9 at (16, 3, 150); at the seeds below the worst figure is 8.0e-11.
PARITY_SEEDS = {(2, 1025, 37): 1702, (4, 1, 50): 1704, (5, 33, 45): 2705, (8, 17, 70): 1708,
                (3, 5, 257): 1703, (9, 5, 100): 1709, (16, 3, 150): 2716}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n{}_f{}_t{}".format(*s))
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_named_classes_match_restatement(form, shape):
    cls, kwargs, n_iter = form
    N, F, T = shape
    # (the solver walks every permutation of the sources: N! of them)
    kwargs = dict(kwargs, permutation_alignment=N <= 8)
    X = _mixture(PARITY_SEEDS[shape], N, F, T)
    ref = fn.CLASSES[cls](**kwargs)
    Yr = ref(X, n_iter=n_iter)
    m = getattr(_fdica(), cls)(**kwargs)
    Y = m(X, n_iter=n_iter)
    print(cls, kwargs, shape, rel_err(m.demix_filter, ref.demix_filter), rel_err(Y, Yr),
          np.max(np.abs(np.array(m.loss) / np.array(ref.loss) - 1)))
    assert rel_err(m.demix_filter, ref.demix_filter) < TOL
    assert rel_err(Y, Yr) < TOL
    np.testing.assert_allclose(m.loss, ref.loss, rtol=LOSS_RTOL)


# 3
ROUTE_SHAPES = [((4, 9, 70), "FDICA_ROUTE_RESIDENT"), ((2, 3, 2100), "FDICA_ROUTE_STREAMING"),
                ((3, 5, 1025), "FDICA_ROUTE_STREAMING"), ((4, 3, 768), "FDICA_ROUTE_RESIDENT"),
                ((4, 3, 769), "FDICA_ROUTE_STREAMING"), ((8, 3, 70), "FDICA_ROUTE_COMPOSED")]


@pytest.mark.parametrize("shape,route", ROUTE_SHAPES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("form", KERNEL_FORMS, ids=KERNEL_IDS)
def test_routes_agree(form, shape, route):
    from ssspy_amd import _lib, _ops, _routes

    cls, kwargs, n_iter = form
    N, F, T = shape
    assert _ops.fdica_route(1, N, F, T, _algorithm(cls, kwargs)) == getattr(_lib, route)
    X = _mixture(720 + N, N, F, T)
    kwargs = dict(kwargs, permutation_alignment=False, scale_restoration=False)
    a = getattr(_fdica(), cls)(**kwargs)
    assert a(X, n_iter=0) is not None and a._kernel_route() == getattr(_lib, route)
    Ya = a(X, n_iter=n_iter)
    with _routes.override(fdica_kernel=False):
        b = getattr(_fdica(), cls)(**kwargs)
        b(X, n_iter=0)
        assert b._kernel_route() == _lib.FDICA_ROUTE_COMPOSED
        Yb = b(X, n_iter=n_iter)
    print(cls, kwargs, shape, rel_err(a.demix_filter, b.demix_filter),
          np.max(np.abs(np.array(a.loss) / np.array(b.loss) - 1)))
    assert rel_err(a.demix_filter, b.demix_filter) < BATCH_TOL
    assert rel_err(Ya, Yb) < BATCH_TOL
    np.testing.assert_allclose(a.loss, b.loss, rtol=BATCH_TOL)


def test_route_function():
    from ssspy_amd import _lib, _ops

    for alg in (_lib.FDICA_GRAD, _lib.FDICA_NATURAL_GRAD, _lib.FDICA_AUX_IP1):
        assert _ops.fdica_route(1, 4, 1025, 512, alg) == _lib.FDICA_ROUTE_RESIDENT
        assert _ops.fdica_route(128, 4, 1025, 768, alg) == _lib.FDICA_ROUTE_RESIDENT
        assert _ops.fdica_route(1, 4, 1025, 769, alg) == _lib.FDICA_ROUTE_STREAMING
        assert _ops.fdica_route(1, 2, 3, 1536, alg) == _lib.FDICA_ROUTE_RESIDENT
        assert _ops.fdica_route(1, 2, 3, 1537, alg) == _lib.FDICA_ROUTE_STREAMING
        assert _ops.fdica_route(1, 5, 33, 45, alg) == _lib.FDICA_ROUTE_COMPOSED
        assert _ops.fdica_route(1, 8, 2049, 1024, alg) == _lib.FDICA_ROUTE_COMPOSED
        assert _ops.fdica_route(1, 9, 5, 100, alg) == _lib.FDICA_ROUTE_COMPOSED
        assert _ops.fdica_route(1, 1, 5, 100, alg) == _lib.FDICA_ROUTE_COMPOSED
    assert _ops.fdica_route(1, 4, 9, 70, _lib.FDICA_AUX_IP2) == _lib.FDICA_ROUTE_COMPOSED
    with pytest.raises(ValueError):
        _ops.fdica_route(1, 4, 0, 70, _lib.FDICA_GRAD)


def _run_steps(X, W, alg, holonomic, n_steps, floor, record=True):
    """(W', loss (n_steps + 1, B, F), logdet likewise, guard bands, info) of one launch."""
    import torch

    from ssspy_amd import _device as dv
    from ssspy_amd import _ops

    B, N, F, T = X.shape
    S = (n_steps + 1) * B
    Xd, Wd = dv.to_device(X, dtype=np.complex128), dv.to_device(W, dtype=np.complex128)
    info = dv.zeros((2,), dv.i32)
    bufs = [dv.zeros((F, 3 * S), dv.f64, Xd.device) for _ in range(2)]
    if record:
        _ops.fdica_steps(Xd, Wd, alg, holonomic, 0.1, floor, n_steps, info,
                         bufs[0].reshape(-1)[S:], bufs[1].reshape(-1)[S:], 3 * S)
    else:
        _ops.fdica_steps(Xd, Wd, alg, holonomic, 0.1, floor, n_steps, info)
    torch.cuda.synchronize()
    got = [dv.to_host(b) for b in bufs]
    guards = [g[:, :S] for g in got] + [g[:, 2 * S:] for g in got]
    terms = [g[:, S:2 * S].reshape(F, n_steps + 1, B).transpose(1, 2, 0) for g in got]
    return dv.to_host(Wd), terms[0], terms[1], guards, info.tolist()


# 4
@pytest.mark.parametrize("shape", [(4, 9, 70), (2, 3, 2100), (7, 5, 45)],
                         ids=lambda s: "n{}_f{}_t{}".format(*s))
@pytest.mark.parametrize("form", KERNEL_FORMS, ids=KERNEL_IDS)
def test_ten_steps_in_one_launch_equal_ten_launches_bitwise(form, shape):
    from ssspy_amd import _lib

    cls, kwargs, _ = form
    N, F, T = shape
    alg, hol = _algorithm(cls, kwargs), kwargs.get("is_holonomic", False)
    X = np.stack([_mixture(730 + b, N, F, T) for b in range(2)])
    W0 = np.tile(np.eye(N, dtype=np.complex128), (2, F, 1, 1))
    floor = (_lib.FLOOR_MAX, 1e-10)
    W10, loss10, logdet10, _, info = _run_steps(X, W0, alg, hol, 10, floor)
    assert info == [0, 0]
    W = W0
    for s in range(10):
        W, loss1, logdet1, _, info = _run_steps(X, W, alg, hol, 1, floor)
        assert np.array_equal(loss1[0], loss10[s]) and np.array_equal(logdet1[0], logdet10[s])
    assert np.array_equal(loss1[1], loss10[10]) and np.array_equal(logdet1[1], logdet10[10])
    assert np.array_equal(W, W10)
    # and the loss arrays do not change the filters
    Wn, _, _, _, _ = _run_steps(X, W0, alg, hol, 10, floor, record=False)
    assert np.array_equal(Wn, W10)


# 5
# (T = 700 is slab resident up to 4 sources; 1600 / 1100 / 800 frames are the re-reading form there)
STEP_SHAPES = [(N, T) for N in range(2, 9) for T in (37, 700)] + [(2, 1600), (3, 1100), (4, 800)]


@pytest.mark.parametrize("N,T", STEP_SHAPES, ids=["{}-t{}".format(*s) for s in STEP_SHAPES])
def test_steps_operator_against_numpy(N, T):
    from ssspy_amd import _lib

    B, F = 2, 5
    rng = np.random.default_rng(740 + N)

    def crandn(*shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)

    X = crandn(B, N, F, T)
    W = np.eye(N) + 0.3 * crandn(B, F, N, N)
    for cls, kwargs, _ in KERNEL_FORMS:
        alg, hol = _algorithm(cls, kwargs), kwargs.get("is_holonomic", False)
        got, loss, logdet, guards, info = _run_steps(X, W, alg, hol, 1, (_lib.FLOOR_MAX, 1e-10))
        assert info == [0, 0]
        assert not any(g.any() for g in guards)  # (only its own entries)
        for b in range(B):
            ref = fn.CLASSES[cls](**kwargs)
            ref.input = X[b]
            ref._reset(demix_filter=W[b])
            states = [ref.demix_filter]
            ref.update_once()
            states.append(ref.demix_filter)
            assert rel_err(got[b], states[1]) < OP_TOL, (cls, kwargs, b)
            for s, Ws in enumerate(states):
                Y = np.matmul(Ws, X[b].transpose(1, 0, 2))  # (F, N, T)
                np.testing.assert_allclose(loss[s, b], np.sum(np.mean(2 * np.abs(Y), axis=2), axis=1),
                                           rtol=OP_TOL)
                np.testing.assert_allclose(logdet[s, b], np.linalg.slogdet(Ws)[1], rtol=OP_TOL,
                                           atol=1e-12)


# 6
def test_weight_operator_against_numpy():
    from ssspy_amd import _device as dv
    from ssspy_amd import _lib, _ops

    rng = np.random.default_rng(750)
    B, S, F, T = 2, 3, 5, 300
    Y = rng.standard_normal((B, S, F, T)) + 1j * rng.standard_normal((B, S, F, T))
    Yd = dv.to_device(Y, dtype=np.complex128)
    a = np.abs(Y)
    for kind, eps, floor in ((_lib.FLOOR_MAX, 1.0, lambda r: np.maximum(r, 1.0)),
                             (_lib.FLOOR_ADD, 0.5, lambda r: r + 0.5),
                             (_lib.FLOOR_NONE, 0.0, lambda r: r)):
        w = _ops.fdica_weight(Yd, False, (kind, eps))
        np.testing.assert_allclose(dv.to_host(w), 1 / floor(a), rtol=1e-14)
        slots = dv.zeros((F, 3 * B), dv.f64, Yd.device)
        w = _ops.fdica_weight(Yd, True, (kind, eps), contrast=slots.reshape(-1)[B:],
                              contrast_stride=3 * B)
        np.testing.assert_allclose(dv.to_host(w), 2 / floor(2 * a), rtol=1e-14)
        got = dv.to_host(slots)
        assert not got[:, :B].any() and not got[:, 2 * B:].any()
        np.testing.assert_allclose(got[:, B:2 * B].T, np.sum(np.mean(2 * a, axis=3), axis=1),
                                   rtol=1e-13)


# 7
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_batch_of_three_equals_single_runs_and_restatement(form):
    cls, kwargs, n_iter = form
    N, F, T = 3, 20, 61
    X = np.stack([_mixture(760 + b, N, F, T) for b in range(3)])
    m = getattr(_fdica(), cls)(**kwargs)
    Y = m(X, n_iter=n_iter)
    assert Y.shape == X.shape and np.array(m.loss).shape == (n_iter + 1, 3)
    for b in range(3):
        s = getattr(_fdica(), cls)(**kwargs)
        Ys = s(X[b], n_iter=n_iter)
        assert rel_err(Y[b], Ys) < BATCH_TOL
        assert rel_err(m.demix_filter[b], s.demix_filter) < BATCH_TOL
        np.testing.assert_allclose(np.array(m.loss)[:, b], s.loss, rtol=BATCH_TOL)
        ref = fn.CLASSES[cls](**kwargs)
        assert rel_err(Y[b], ref(X[b], n_iter=n_iter)) < TOL
        np.testing.assert_allclose(np.array(m.loss)[:, b], ref.loss, rtol=LOSS_RTOL)


# 8
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_two_runs_are_bit_identical(form):
    cls, kwargs, n_iter = form
    X = np.stack([_mixture(770 + b, 4, 65, 50) for b in range(2)])
    runs = []
    for _ in range(2):
        m = getattr(_fdica(), cls)(**kwargs)
        Y = m(X, n_iter=n_iter)
        runs.append((Y, np.array(m.demix_filter), np.array(m.loss)))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# 9
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_update_once_by_hand_equals_call(form):
    cls, kwargs, _ = form
    kwargs = dict(kwargs, scale_restoration=False, permutation_alignment=False)
    X = _mixture(780, 3, 33, 45)
    a = getattr(_fdica(), cls)(**kwargs)
    Ya = a(X, n_iter=5)
    b = getattr(_fdica(), cls)(record_loss=False, **kwargs)
    b(X, n_iter=0)
    for _ in range(5):
        b.update_once()
    assert rel_err(b.demix_filter, a.demix_filter) < BATCH_TOL
    assert rel_err(b.output, Ya) < BATCH_TOL  # (formed lazily from the filters)
    assert abs(b.compute_loss() / a.loss[-1] - 1) < LOSS_RTOL


# 10
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_record_loss_with_and_without_callback(form):
    cls, kwargs, n_iter = form
    X = _mixture(790, 4, 33, 45)
    seen = []
    a = getattr(_fdica(), cls)(callbacks=lambda method: seen.append(len(method.loss)), **kwargs)
    Ya = a(X, n_iter=n_iter)
    b = getattr(_fdica(), cls)(**kwargs)
    Yb = b(X, n_iter=n_iter)
    c = getattr(_fdica(), cls)(record_loss=False, **kwargs)
    Yc = c(X, n_iter=n_iter)
    assert seen == list(range(1, n_iter + 2)) and len(b.loss) == n_iter + 1 and c.loss is None
    np.testing.assert_allclose(b.loss, a.loss, rtol=LOSS_RTOL)
    assert rel_err(Yb, Ya) < BATCH_TOL and rel_err(Yc, Ya) < BATCH_TOL
    d = getattr(_fdica(), cls)(**kwargs)
    d(X, n_iter=n_iter, initial_call=False)
    np.testing.assert_allclose(d.loss, a.loss[1:], rtol=LOSS_RTOL)


# 11
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_host_evaluated_floor_equals_kernel_floor(form):
    cls, kwargs, n_iter = form
    X = _mixture(800, 3, 20, 45)
    eps = float(np.median(np.abs(X)))  # (acts on about half of the entries)

    def disguised(x):
        return np.maximum(x, eps)

    a = getattr(_fdica(), cls)(flooring_fn=functools.partial(_flooring().max_flooring, eps=eps),
                               **kwargs)
    b = getattr(_fdica(), cls)(flooring_fn=disguised, **kwargs)
    Ya, Yb = a(X, n_iter=n_iter), b(X, n_iter=n_iter)
    assert rel_err(Yb, Ya) < BATCH_TOL
    np.testing.assert_allclose(b.loss, a.loss, rtol=LOSS_RTOL)
    ref = fn.CLASSES[cls](flooring_fn=disguised, **kwargs)
    assert rel_err(Yb, ref(X, n_iter=n_iter)) < TOL


# 12
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_generic_classes_with_closures_equal_named(form):
    cls, kwargs, n_iter = form
    fdica = _fdica()
    X = _mixture(810, 3, 20, 45)
    named = getattr(fdica, cls)(**kwargs)
    if cls.startswith("Aux"):
        generic = fdica.AuxFDICA(contrast_fn=tc.generic_contrast_fn,
                                 d_contrast_fn=tc.generic_d_contrast_fn, **kwargs)
    else:
        generic = getattr(fdica, cls.replace("Laplace", ""))(
            contrast_fn=tc.generic_contrast_fn, score_fn=tc.generic_score_fn, **kwargs)
    Yn, Yg = named(X, n_iter=n_iter), generic(X, n_iter=n_iter)
    assert generic._model is None and named._model is not None
    assert rel_err(Yg, Yn) < TOL
    assert rel_err(generic.demix_filter, named.demix_filter) < TOL
    np.testing.assert_allclose(generic.loss, named.loss, rtol=LOSS_RTOL)


def test_borrowed_closures_take_the_compatibility_path():
    """Closures taken from a named instance read THAT instance's floor: on another separator they
    are user closures (the tag alone must not put them on the device path)."""
    from ssspy_amd import _lib

    fdica = _fdica()
    X = _mixture(815, 3, 12, 40)
    eps = float(np.median(np.abs(X)))
    # (no alignment: its floor is the separator's own ``flooring_fn``, which differs between the two)
    donor = fdica.NaturalGradLaplaceFDICA(
        flooring_fn=functools.partial(_flooring().max_flooring, eps=eps),
        permutation_alignment=False)
    borrowed = fdica.NaturalGradFDICA(contrast_fn=donor.contrast_fn, score_fn=donor.score_fn,
                                      permutation_alignment=False)
    Yd, Yb = donor(X, n_iter=5), borrowed(X, n_iter=5)
    assert borrowed._model is None and donor._model is not None
    assert borrowed._kernel_route() == _lib.FDICA_ROUTE_COMPOSED
    assert rel_err(Yb, Yd) < TOL  # (the donor's floor, not the borrower's default one)


# 13
@pytest.mark.parametrize("form", [FORMS[2], FORMS[4]], ids=["natgrad", "ip1"])
def test_permutation_alignment_of_shuffled_bins(form):
    cls, kwargs, n_iter = form
    N, F, T = 3, 24, 120
    X = _mixture(820, N, F, T)
    rng = np.random.default_rng(821)
    W0 = np.tile(np.eye(N, dtype=np.complex128), (F, 1, 1))
    for i in range(F):  # the rows of the initial filters shuffled per bin: so are the estimates
        W0[i] = W0[i][rng.permutation(N)]
    out = {}
    for align in (True, False):
        ref = fn.CLASSES[cls](permutation_alignment=align, **kwargs)
        Yr = ref(X, n_iter=n_iter, demix_filter=W0)
        m = getattr(_fdica(), cls)(permutation_alignment=align, **kwargs)
        Y = m(X, n_iter=n_iter, demix_filter=W0)
        assert rel_err(Y, Yr) < TOL and rel_err(m.demix_filter, ref.demix_filter) < TOL
        out[align] = Y
    assert rel_err(out[True], out[False]) > 0.1  # (the alignment moved rows)
    m = getattr(_fdica(), cls)(permutation_alignment=False, scale_restoration=False, **kwargs)
    m(X, n_iter=n_iter, demix_filter=W0)
    m.solve_permutation_by_correlation(flooring_fn=None)
    ref = fn.CLASSES[cls](permutation_alignment=True, scale_restoration=False, flooring_fn=None,
                          **kwargs)
    ref.flooring_fn = functools.partial(fn.max_flooring, eps=1e-10)  # (the iterations' floor)
    ref.input = X.copy()
    ref._reset(demix_filter=W0)
    for _ in range(n_iter):
        ref.update_once()
    ref.flooring_fn = fn.identity
    ref.solve_permutation()
    assert rel_err(m.demix_filter, ref.demix_filter) < TOL and rel_err(m.output, ref.output) < TOL
    with pytest.raises(NotImplementedError):
        bad = getattr(_fdica(), cls)(permutation_alignment="posterior_score", **kwargs)
        bad(X, n_iter=1)


# 14
@pytest.mark.parametrize("restoration,reference_id", [(False, 0), (True, 0), ("projection_back", 2),
                                                      ("minimal_distortion_principle", 1)])
def test_scale_restorations(restoration, reference_id):
    X = _mixture(830, 3, 20, 45)
    kwargs = dict(scale_restoration=restoration, reference_id=reference_id)
    ref = fn.AuxLaplaceFDICA(**kwargs)
    Yr = ref(X, n_iter=10)
    m = _fdica().AuxLaplaceFDICA(**kwargs)
    Y = m(X, n_iter=10)
    assert rel_err(Y, Yr) < TOL and rel_err(m.demix_filter, ref.demix_filter) < TOL
    assert rel_err(m.output, Yr) < TOL


# 15
def test_singular_injected_filter_raises_linalg_error():
    X = _mixture(840, 3, 8, 40)
    W = np.tile(np.eye(3, dtype=np.complex128), (8, 1, 1))
    W[5, 2] = W[5, 1]  # two equal rows in one bin: an exact zero pivot
    with pytest.raises(np.linalg.LinAlgError):
        _fdica().GradLaplaceFDICA(record_loss=False)(X, n_iter=2, demix_filter=W)


# 16
def test_seventeen_sources_are_refused():
    X = np.random.default_rng(0).standard_normal((17, 2, 40)) + 0j
    with pytest.raises(NotImplementedError, match="16"):
        _fdica().AuxLaplaceFDICA(permutation_alignment=False)(X, n_iter=1)


# 17
def test_constructor_contract():
    fdica = _fdica()
    closures = dict(contrast_fn=tc.generic_contrast_fn, score_fn=tc.generic_score_fn)
    with pytest.raises(ValueError, match="Specify contrast function."):
        fdica.GradFDICA(score_fn=tc.generic_score_fn)
    with pytest.raises(ValueError, match="Specify score function."):
        fdica.NaturalGradFDICA(contrast_fn=tc.generic_contrast_fn)
    with pytest.raises(ValueError, match="Specify contrast function."):
        fdica.AuxFDICA(d_contrast_fn=tc.generic_d_contrast_fn)
    with pytest.raises(ValueError, match="reference_id"):
        fdica.AuxLaplaceFDICA(reference_id=None)
    for cls in ("GradFDICA", "NaturalGradFDICA"):
        assert getattr(fdica, cls)(**closures).is_holonomic is False
    for cls in ("GradLaplaceFDICA", "NaturalGradLaplaceFDICA"):
        m = getattr(fdica, cls)()
        assert m.is_holonomic is False and m.step_size == 0.1
        assert repr(m) == (cls + "(step_size=0.1, is_holonomic=False, permutation_alignment=True, "
                           "scale_restoration=True, record_loss=True, reference_id=0)")
    assert repr(fdica.GradFDICABase(**closures)) == (
        "GradFDICA(step_size=0.1, permutation_alignment=True, scale_restoration=True, "
        "record_loss=True, reference_id=0)")
    assert repr(fdica.NaturalGradFDICA(scale_restoration=False, **closures)) == (
        "NaturalGradFDICA(step_size=0.1, is_holonomic=False, permutation_alignment=True, "
        "scale_restoration=False, record_loss=True)")
    m = fdica.AuxLaplaceFDICA()
    assert m.spatial_algorithm == "IP" and not hasattr(m, "pair_selector")
    assert repr(m) == ("AuxLaplaceFDICA(spatial_algorithm=IP, permutation_alignment=True, "
                       "scale_restoration=True, record_loss=True, reference_id=0)")
    assert repr(fdica.AuxFDICA(spatial_algorithm="IP2", contrast_fn=tc.generic_contrast_fn,
                               d_contrast_fn=tc.generic_d_contrast_fn)) == (
        "AuxFDICA(spatial_algorithm=IP2, permutation_alignment=True, scale_restoration=True, "
        "record_loss=True, reference_id=0)")
    assert repr(fdica.FDICABase(contrast_fn=tc.generic_contrast_fn)) == (
        "FDICA(, permutation_alignment=True, scale_restoration=True, record_loss=True, "
        "reference_id=0)")
    assert fdica.AuxLaplaceFDICA(spatial_algorithm="IP2").pair_selector is not None
    assert fdica.GradLaplaceFDICA(flooring_fn=None).flooring_fn(3.0) == 3.0
    with pytest.raises(AssertionError):
        fdica.AuxLaplaceFDICA(spatial_algorithm="ISS")


# 18
def test_bench_shape_loss_falls_over_100_iterations():
    """One mixture of the benchmark shape (4 sources, 1025 bins, 512 frames), 100 iterations: the
    loss of AuxLaplaceFDICA is finite and non-increasing up to 1e-9 of its first value (every run of
    the reference was monotone for IP1), NaturalGradLaplaceFDICA ends below where it starts.  No
    parity is asserted here."""
    X = _mixture(1000, 4, 1025, 512)
    m = _fdica().AuxLaplaceFDICA()
    m(X, n_iter=100)
    loss = np.array(m.loss)
    print("aux loss", loss[0], loss[1], loss[-1], np.max(np.diff(loss)))
    assert loss.shape == (101,) and np.isfinite(loss).all()
    assert np.all(np.diff(loss) <= 1e-9 * abs(loss[0]))
    m = _fdica().NaturalGradLaplaceFDICA()
    m(X, n_iter=100)
    loss = np.array(m.loss)
    print("natural gradient loss", loss[0], loss[1], loss[-1])
    assert loss.shape == (101,) and np.isfinite(loss).all() and loss[-1] < loss[0]
