"""MaskingADMMHVA on the device: the cepstral pass on ADMM's operand element by element against an
extended evaluation (tests/hva_numpy.py in longdouble), the masked auxiliary step against NumPy, the
class against the golden vectors of the reference, and the equalities between the ways to run the
same thing.

Bars (those of tests/test_gpu_hva.py): 1e-8 relative Frobenius on filters, states and outputs, 1e-10
on single operators and on every equality; the cepstral pass has the absolute bar per column of
``test_gpu_hva.cepstrum_bar`` with the forming error of Z restated at ``admm_cepstrum_bar``.
"""

import functools

import numpy as np
import pytest

import admmbss_cases as ac
import admmhva_cases as hc
import hva_cases
import hva_numpy as hn
from conftest import load_golden, rel_err
from test_gpu_hva import FLOORS, OP_TOL, TOL, cepstrum_bar

pytestmark = pytest.mark.gpu

_ids = dict(ids=lambda s: "b{}_n{}_f{}_t{}".format(*s))


def _hva():
    from ssspy_amd.bss import hva

    return hva


def _fl():
    from ssspy_amd.special import flooring

    return flooring


def _dev(a, dtype=np.complex128):
    from ssspy_amd import _device as dv

    return dv.to_device(np.ascontiguousarray(a), dtype=dtype)


def _host(t):
    from ssspy_amd import _device as dv

    return dv.to_host(t)


def _crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _z_of(X, W, aux2, dual2, relax, dtype=np.clongdouble):
    """Z = relax W x + (1 - relax) aux2 + dual2 in ``dtype``; aux2 is not read at relax 1."""
    Z = np.einsum("bfnm,bmft->bnft", W.astype(dtype), X.astype(dtype))
    if relax != 1:
        Z = dtype(relax) * Z + dtype(1 - relax) * aux2.astype(dtype)
    return Z + dual2.astype(dtype)


# ------------------------------------------------------------------ the cepstral pass
# the shapes of the issue: F = 2 and 3 (transforms of length 2 and 4), T = 1 and T below a tile, T one
# over a multiple of the tile (257, 129), 16 sources, both routes (F = 2, 3, 5, 33, 9) and the direct
# sum only (F = 12), two mixtures
CEPSTRUM_SHAPES = [(2, 2, 2, 50), (1, 3, 3, 7), (1, 3, 5, 1), (2, 4, 33, 257), (1, 16, 9, 40),
                   (1, 5, 12, 129)]
MASK_ITERS = (0, 2)


@functools.lru_cache(maxsize=None)
def _cepstrum_inputs(shape, relax):
    """X, W, aux2, dual2 (one penalty) with exact zeros in Z, as ``test_gpu_hva._cepstrum_inputs``
    places them: every bin of frame 0 of source 0 of mixture 0 (a whole column) and bin 1 of one
    frame of source 1 (one entry), by zero rows of W and zero entries of both states."""
    B, N, F, T = shape
    rng = np.random.default_rng(sum(shape) + 1)
    X = _crandn(rng, B, N, F, T)
    W = _crandn(rng, B, F, N, N) / np.sqrt(N)
    aux2, dual2 = _crandn(rng, B, 1, N, F, T), _crandn(rng, B, 1, N, F, T)
    t1 = min(3, T - 1)
    W[0, :, 0, :] = 0
    W[0, 1, 1, :] = 0
    for state in (aux2, dual2):
        state[0, 0, 0, :, 0] = 0
        state[0, 0, 1, 1, t1] = 0
    Z = _z_of(X, W, aux2[:, 0], dual2[:, 0], relax)
    size = relax * np.einsum("bfnm,bmft->bnft", np.abs(W), np.abs(X)) + np.abs(dual2[:, 0])
    if relax != 1:
        size = size + abs(1 - relax) * np.abs(aux2[:, 0])
    assert np.count_nonzero(Z == 0) == F + 1
    return X, W, aux2, dual2, Z, size


def admm_cepstrum_bar(Z, size, flooring_fn, mask_iter):
    """``cepstrum_bar`` of tests/test_gpu_hva.py for Z = relax W x + (1 - relax) aux2 + dual2.

    There the kernel forms an entry of Z with N complex fused multiply-adds and one addition, and its
    modulus is off by at most (4 N + 8) u s with s = sum_m |W2||x| + |dual|.  Here, with
    s = relax sum_m |W||x| + |1 - relax||aux2| + |dual2| (``size``), the N fused multiply-adds and the
    last addition are the same (the error of W x is scaled by relax, as its share of s is), and
    between them stand, per real component, two more products and one more addition:
    relax (W x) at u relax |W x|, (1 - relax) aux2 at 2 u |1 - relax||aux2| (the product, and the
    difference 1 - relax itself) and their sum at u of it, 4 u s at most per component and
    sqrt(2) 4 u s < 6 u s on the modulus.  So the modulus is off by at most (4 N + 14) u s; everything
    after it is ``cepstrum_bar`` unchanged, which takes s and multiplies it by (4 N + 8)."""
    N = Z.shape[1]
    return cepstrum_bar(Z, size * ((4 * N + 14) / (4 * N + 8)), flooring_fn, mask_iter)


@pytest.mark.parametrize("relax", [1.0, 1.25])
@pytest.mark.parametrize("floor", list(FLOORS))
@pytest.mark.parametrize("shape", CEPSTRUM_SHAPES, **_ids)
def test_cepstral_pass_on_the_admm_operand(shape, floor, relax):
    from ssspy_amd import _lib, _ops

    B, N, F, T = shape
    X, W, aux2, dual2, Z, size = _cepstrum_inputs(shape, relax)
    kind, eps, flooring_fn = FLOORS[floor]
    power_of_two = (F - 1) & (F - 2) == 0
    routes = [_lib.HVA_ROUTE_AUTO, _lib.HVA_ROUTE_DIRECT] if power_of_two else [_lib.HVA_ROUTE_AUTO]
    given_aux2 = aux2 if relax != 1 else np.full_like(aux2, np.nan)  # (not read at relaxation 1)
    dX, dW, da, dd = _dev(X), _dev(W), _dev(given_aux2), _dev(dual2)
    table = _ops.hva_cos_table(F, dX.device)
    for mask_iter in MASK_ITERS:
        ref, bar, bad = admm_cepstrum_bar(Z, size, flooring_fn, mask_iter)
        assert bad.any() == (floor == "none") and not bad.all()
        assert float(np.max(bar)) < 1e-5  # (the bar itself stays far under the size of varrho)
        got = []
        for route in routes:
            out = _host(_ops.hva_admm_cepstrum(dX, dW, da, dd, 0, table, (kind, eps), mask_iter,
                                               relax, route=route))
            assert out.shape == shape and out.dtype == np.float64
            nan = np.isnan(out)
            assert np.array_equal(nan, np.broadcast_to(bad, shape))  # log 0 as in NumPy, no more
            err = np.where(nan, 0, np.abs(out - ref.astype(np.float64)))
            worst = float(np.max(err / bar))
            print("admm cepstrum", shape, floor, relax, mask_iter, route,
                  "max err {:.2e} err/bar {:.3f}".format(float(np.max(err)), worst))
            assert worst < 1
            got.append(np.where(nan, 0, out))
        if len(got) == 2:  # the two routes agree within the same bar
            assert float(np.max(np.abs(got[0] - got[1]) / bar)) < 1
    assert np.array_equal(_host(dd), dual2)  # the pass leaves the states alone
    assert np.array_equal(_host(da), given_aux2, equal_nan=True)


def test_cepstral_pass_refusals():
    from ssspy_amd import _lib, _ops

    X, W, aux2, dual2, _, _ = _cepstrum_inputs((1, 5, 12, 129), 1.25)
    dX, dW, da, dd = _dev(X), _dev(W), _dev(aux2), _dev(dual2)
    table = _ops.hva_cos_table(12, dX.device)
    out = _ops.hva_admm_cepstrum(dX, dW, da, dd, 0, table, (0, 0.0), 1, 1.25)
    with pytest.raises(NotImplementedError):  # no FFT of length 22
        _ops.hva_admm_cepstrum(dX, dW, da, dd, 0, table, (0, 0.0), 1, 1.25, route=_lib.HVA_ROUTE_FFT)
    with pytest.raises(ValueError):
        _ops.hva_admm_cepstrum(dX, dW, da, da, 0, table, (0, 0.0), 1, 1.25)
    with pytest.raises(ValueError, match="stride"):
        _lib.check(_lib.load().ssspy_hva_admm_cepstrum(
            _ops.ptr(dX), _ops.ptr(dW), _ops.ptr(da), _ops.ptr(dd), 5 * 12 * 129 - 1, _ops.ptr(table),
            _ops.ptr(out), 1, 5, 12, 129, 1.25, 0, 0.0, 1, _lib.HVA_ROUTE_AUTO, _ops._st()), "stride")
    big = np.zeros((1, 1, 17, 2, 4), dtype=complex)
    with pytest.raises(NotImplementedError, match="1..16 sources"):
        _ops.hva_admm_cepstrum(_dev(big[:, 0]), _dev(np.zeros((1, 2, 17, 17), dtype=complex)),
                               _dev(big), _dev(big), 0, _ops.hva_cos_table(2, dX.device), (0, 0.0),
                               1, 1.0)


# ------------------------------------------------------------------ the masked auxiliary step
AUX_SHAPES = [(2, 3, 5, 70), (1, 2, 3, 300), (1, 9, 4, 40), (1, 16, 2, 7)]


@pytest.mark.parametrize("relax", [1.0, 1.25])
@pytest.mark.parametrize("shape", AUX_SHAPES, **_ids)
def test_masked_aux_step(shape, relax):
    """Against NumPy, on penalty 1 of two (a batch stride of 2 N F T; the other slice is untouched).
    One (source, frame) column of varrho is NaN: the sum over sources makes the mask of every source
    of that frame NaN in NumPy, and exactly those entries of both outputs are NaN here.  With
    relaxation 1 auxiliary2 is not read: it holds NaN."""
    from ssspy_amd import _ops

    B, N, F, T = shape
    Q, q, gamma = 2, 1, 0.4
    rng = np.random.default_rng(70 + N)
    X, W = _crandn(rng, B, N, F, T), _crandn(rng, B, F, N, N) / np.sqrt(N)
    aux2, dual2 = _crandn(rng, B, Q, N, F, T), _crandn(rng, B, Q, N, F, T)
    varrho = 3 * rng.standard_normal((B, N, F, T))
    varrho[0, 0, :, 2] = np.nan
    Z = _z_of(X, W, aux2[:, q], dual2[:, q], relax, dtype=np.complex128)
    with np.errstate(invalid="ignore"):
        mask = hn.mask_of(varrho, gamma)
        stable = hn.stable_mask_of(varrho, gamma)
    column = np.zeros(shape, dtype=bool)
    column[0, :, :, 2] = True
    assert np.array_equal(np.isnan(mask), column) and np.array_equal(np.isnan(stable), column)
    assert rel_err(stable[~column], mask[~column]) < 1e-13
    if relax == 1:
        aux2[:, q] = np.nan
    da, dd = _dev(aux2), _dev(dual2)
    _ops.hva_aux_step(_dev(X), _dev(W), da, dd, q, _dev(varrho, dtype=np.float64), gamma, relax)
    got_a, got_d = _host(da), _host(dd)
    assert np.array_equal(got_a[:, 0], aux2[:, 0]) and np.array_equal(got_d[:, 0], dual2[:, 0])
    for got in (got_a[:, q], got_d[:, q]):
        assert np.array_equal(np.isnan(got.real), column) and np.array_equal(np.isnan(got.imag), column)
    want_a = mask * Z
    errs = (rel_err(got_a[:, q][~column], want_a[~column]),
            rel_err(got_d[:, q][~column], (Z - want_a)[~column]))
    print("hva_aux_step", shape, relax, errs)
    assert max(errs) < OP_TOL


def test_masked_aux_step_refusals():
    from ssspy_amd import _lib, _ops

    B, N, F, T = 1, 3, 4, 9
    rng = np.random.default_rng(5)
    dX, dW = _dev(_crandn(rng, B, N, F, T)), _dev(_crandn(rng, B, F, N, N))
    da, dd = _dev(_crandn(rng, B, 1, N, F, T)), _dev(_crandn(rng, B, 1, N, F, T))
    dv = _dev(rng.standard_normal((B, N, F, T)), dtype=np.float64)
    with pytest.raises(ValueError):  # auxiliary2 and dual2 in the same memory
        _ops.hva_aux_step(dX, dW, da, da, 0, dv, 0.5, 1.0)
    with pytest.raises(ValueError, match="stride"):
        _lib.check(_lib.load().ssspy_hva_aux_step(
            _ops.ptr(dX), _ops.ptr(dW), _ops.ptr(da), _ops.ptr(dd), N * F * T - 1, _ops.ptr(dv), 0.5,
            1.0, B, N, F, T, _ops._st()), "stride")
    big = _dev(np.zeros((1, 1, 17, 2, 4), dtype=complex))
    with pytest.raises(NotImplementedError, match="1..16 sources"):
        _ops.hva_aux_step(_dev(np.zeros((1, 17, 2, 4), dtype=complex)),
                          _dev(np.zeros((1, 2, 17, 17), dtype=complex)), big,
                          _dev(np.zeros((1, 1, 17, 2, 4), dtype=complex)), 0,
                          _dev(np.zeros((1, 17, 2, 4)), dtype=np.float64), 0.5, 1.0)


# ------------------------------------------------------------------ the class
def _construct(spec, **extra):
    return hc.construct(_hva(), _fl(), spec, **extra)


def _states(m):
    return [np.array(getattr(m, k)) for k in ("demix_filter",) + ac.ADMM_STATES]


def _errs(m, other, Y, Yo):
    return [rel_err(a, b) for a, b in zip(_states(m), _states(other))] + [rel_err(Y, Yo)]


@pytest.mark.parametrize("name", hc.CASES)
def test_class_replays_golden(name):
    g = load_golden(name)
    spec = hc.golden_spec(g)
    snap, seen = ac.Snapshots("MaskingADMMBSS"), []
    shapes = [("output", g["X"].shape), ("demix_filter", g["final_demix_filter"].shape),
              ("auxiliary1", g["final_demix_filter"].shape), ("dual1", g["final_demix_filter"].shape),
              ("auxiliary2", g["X"].shape), ("dual2", g["X"].shape)]

    def look(method):  # callbacks see NumPy arrays of the right shapes
        seen.append(all(isinstance(getattr(method, k), np.ndarray) and getattr(method, k).shape == v
                        for k, v in shapes))

    m = _construct(spec, callbacks=[snap, look])
    assert (m.device_floor() is None) == (spec["flooring"] == "lambda")
    init = ac.golden_init(g)
    Y = m(g["X"], n_iter=spec["n_iter"], **init)
    ac.check_against_golden(g, m, Y, snap, TOL, None, show=name)
    assert len(seen) == spec["n_iter"] + 1 and all(seen)
    assert m.attenuation == (spec["attenuation"] or 1 / spec["N"])
    for key, value in init.items():
        assert np.array_equal(value, g[key + "0"])


@pytest.mark.parametrize("floor", ["max", "add"])
def test_first_iteration_from_the_zero_state(floor):
    """W = 0, so Z = 0 exactly; with a floor the mask is the finite constant N ** -attenuation and
    auxiliary2 = dual2 = 0."""
    spec = dict(hc.DEFAULTS, N=3, F=9, T=40, flooring=floor, rho=0.5, scale_restoration=False)
    m = _construct(spec)
    assert m.device_floor() is not None
    m(ac.mixture(1, 3, 9, 40), n_iter=1)
    assert not np.any(m.demix_filter)
    assert np.array_equal(m.auxiliary1, np.broadcast_to(np.sqrt(1 / 0.5) * np.eye(3), (9, 3, 3)))
    assert m.auxiliary2.shape == (3, 9, 40) == m.dual2.shape
    assert not np.any(m.auxiliary2) and not np.any(m.dual2)
    assert m.attenuation == 1 / 3


def _batch_input(spec, B):
    return np.stack([ac.mixture(spec["seed"] + 20 * b, spec["N"], spec["F"], spec["T"])
                     for b in range(B)])


@pytest.mark.parametrize("floor", ["max", "add", "none"])
def test_device_route_equals_compatibility_route(floor):
    """The same flooring behind a lambda is not recognised: the inherited update_once with the host
    mask_fn.  Without a floor the states are injected (Z = 0 has no mask there)."""
    spec = dict(hc.DEFAULTS, N=3, F=17, T=50, seed=3, flooring=floor, relaxation=1.25)
    X = _batch_input(spec, 2)
    init = {}
    if floor == "none":
        parts = [hc.injected(dict(spec, inject=True, seed=3 + 20 * b)) for b in range(2)]
        init = {k: np.stack([p[k] for p in parts]) for k in parts[0]}
    named = hva_cases.flooring_of(floor, _fl()) or _fl().identity
    m = _construct(spec)
    host = _hva().MaskingADMMHVA(**dict(hc.build_kwargs(spec, _fl()), flooring_fn=lambda x: named(x)))
    assert m.device_floor() is not None and host.device_floor() is None
    Y, Yh = m(X, n_iter=10, **init), host(X, n_iter=10, **init)
    errs = _errs(m, host, Y, Yh)
    print(floor, errs)
    assert np.isfinite(Y).all() and max(errs) < TOL


def test_both_transform_routes_in_the_class():
    from ssspy_amd import _lib

    spec = dict(hc.DEFAULTS, N=2, F=9, T=40, seed=3)
    X = ac.mixture(3, 2, 9, 40)
    m, direct = _construct(spec), _construct(spec)
    direct._transform_route = _lib.HVA_ROUTE_DIRECT
    assert m.transform_route(9) == _lib.HVA_ROUTE_FFT
    assert direct.transform_route(9) == _lib.HVA_ROUTE_DIRECT
    assert m.transform_route(12) == _lib.HVA_ROUTE_DIRECT
    Y, Yd = m(X, n_iter=10), direct(X, n_iter=10)
    assert max(_errs(m, direct, Y, Yd)) < OP_TOL


def test_batch_of_three_equals_the_single_calls():
    spec = dict(hc.DEFAULTS, N=3, F=9, T=40, seed=4, mask_iter=2, relaxation=1.25)
    X = _batch_input(spec, 3)
    m = _construct(spec)
    Y = m(X, n_iter=10)
    assert m.dual2.shape == (3, 3, 9, 40) and m.demix_filter.shape == (3, 9, 3, 3)
    for b in range(3):
        single = _construct(spec)
        Ys = single(X[b], n_iter=10)
        assert single.auxiliary2.shape == (3, 9, 40)
        errs = [rel_err(a[b], s) for a, s in zip(_states(m), _states(single))] + [rel_err(Y[b], Ys)]
        assert max(errs) < OP_TOL


def test_update_once_by_hand_equals_call():
    spec = dict(hc.DEFAULTS, N=3, F=9, T=40, seed=5, scale_restoration=False)
    X = ac.mixture(5, 3, 9, 40)
    m = _construct(spec)
    Y = m(X, n_iter=10)
    hand = _construct(spec)
    hand(X, n_iter=0)
    for _ in range(10):
        hand.update_once()
    for a, b in zip(_states(hand), _states(m)):
        assert np.array_equal(a, b)
    assert rel_err(hand.separate(X, hand.demix_filter), Y) < OP_TOL


@pytest.mark.parametrize("shape", [(2, 17, 50), (5, 12, 40)], ids=["n2_fft", "n5_direct"])
def test_two_runs_are_bit_identical(shape):
    N, F, T = shape
    spec = dict(hc.DEFAULTS, N=N, F=F, T=T, seed=3, relaxation=1.25)
    X = ac.mixture(3, N, F, T)
    runs = []
    for _ in range(2):
        m = _construct(spec)
        runs.append([m(X, n_iter=10)] + _states(m))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_class_refusals():
    with pytest.raises(NotImplementedError, match="up to 16 sources"):
        _hva().MaskingADMMHVA()(ac.mixture(1, 17, 2, 40), n_iter=1)
    for floor in ("max", "lambda"):  # a single bin, on either route
        m = _hva().MaskingADMMHVA(flooring_fn=hva_cases.flooring_of(floor, _fl()))
        with pytest.raises(ValueError, match="Invalid number of FFT data points"):
            m(ac.mixture(1, 2, 1, 40), n_iter=1)
