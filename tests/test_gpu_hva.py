"""MaskingPDSHVA / HVA on the device: the cepstral pass element by element against an extended
evaluation of its formulas (tests/hva_numpy.py in longdouble), the masked dual step against NumPy,
the classes against the golden vectors of the reference and against the NumPy restatement, and the
equalities between the ways to run the same thing.

Bars: 1e-8 relative Frobenius on filters, dual variables and outputs, 1e-10 on
single operators and on every equality; the cepstral pass has its own absolute bar per column, derived
at ``cepstrum_bar``.
"""

import functools

import numpy as np
import pytest

import hva_cases as hc
import hva_numpy as hn
import pdsbss_cases as pc
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL, OP_TOL = 1e-8, 1e-10
U = 2.0 ** -53


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


# ------------------------------------------------------------------ the cepstral pass
# F = 2 and 3 (transforms of length 2 and 4: no interior term, one); T = 1 and T below a tile; T one
# over a multiple of the tile (257, 129) and several tiles; 16 sources; F = 2^k + 1 with both routes
# (2, 3, 5, 33, 9, 129) and F = 12, 100 with the direct sum only; two mixtures
CEPSTRUM_SHAPES = [(2, 2, 2, 50), (1, 3, 3, 7), (1, 3, 5, 1), (2, 4, 33, 257), (1, 5, 12, 129),
                   (1, 16, 9, 40), (1, 2, 129, 70), (1, 2, 100, 70)]
FLOORS = {"none": (0, 0.0, None), "max": (1, 1e-10, functools.partial(hn.max_flooring, eps=1e-10)),
          "add": (2, 1e-6, functools.partial(hn.add_flooring, eps=1e-6))}


@functools.lru_cache(maxsize=None)
def _cepstrum_inputs(shape):
    """X, W2, dual (one penalty) with exact zeros in Z: every bin of frame 0 of source 0 of mixture 0
    (a whole column) and bin 1 of one frame of source 1 (one entry of a column), by zero rows of W2
    and zero entries of the dual variable."""
    B, N, F, T = shape
    rng = np.random.default_rng(sum(shape))
    X = _crandn(rng, B, N, F, T)
    W2 = _crandn(rng, B, F, N, N) / np.sqrt(N)
    dual = _crandn(rng, B, 1, N, F, T)
    W2[0, :, 0, :] = 0
    dual[0, 0, 0, :, 0] = 0
    W2[0, 1, 1, :] = 0
    dual[0, 0, 1, 1, min(3, T - 1)] = 0
    ld = np.clongdouble
    Z = dual[:, 0].astype(ld) + np.einsum("bfnm,bmft->bnft", W2.astype(ld), X.astype(ld))
    size = np.einsum("bfnm,bmft->bnft", np.abs(W2), np.abs(X)) + np.abs(dual[:, 0])
    assert np.count_nonzero(Z == 0) == F + 1
    return X, W2, dual, Z, size


def cepstrum_bar(Z, size, flooring_fn, mask_iter):
    """(reference varrho in longdouble, absolute bar per column (B, N, 1, T), bad columns).

    With u = 2^-53, n = 2 (F - 1), everything measured on the extended evaluation:

    * the kernel forms an entry of Z with N complex fused multiply-adds and one addition: its
      modulus is off by at most (4 N + 8) u s, s = sum_m |W2||x| + |dual| (``size``), so zeta = log a
      by e0 = (4 N + 8) u s / a + 2 u |zeta| + 2 u (hypot and log at an ulp each); e0 is taken as the
      maximum over the bins of the column.
    * the mean over F bins: e0 + F u max|zeta|; rho: e_rho = 2 e0 + (F + 1) u max|zeta|.
    * nu = D(rho) / n: the weights of D add up to n, so the input error passes as e_rho, and a sum
      of F terms with a table at an ulp adds (F + 6) u R, R = max|rho|.  (The FFT route sums fewer
      terms per output, but rounds relative to the larger of the two frames it transforms together:
      R, P and the maxima of zeta and varrho are therefore taken over the whole tensor.)
    * h(nu) = sigma(nu) nu: sigma' is at most A = (pi / 2)^mask_iter and |nu| at most R, so
      |h'| <= H = (1 + A) max(1, R); the product pi sigma and the cosines add 8 u max(1, R) before h'.
      e_p = H (e_rho + (F + 6) u R + 8 u max(1, R)).
    * varrho = D(sigma nu) + mean: n e_p + (F + 6) u n P with P = max|sigma nu|, the error of the
      mean and 4 u max|varrho| for the last addition.

    A column that holds log 0 (no floor) is NaN throughout in NumPy, and must be here."""
    B, N, F, T = Z.shape
    n = 2 * (F - 1)
    ref, rho, product = hn.cepstrum_chain(Z, flooring_fn, mask_iter, dtype=np.longdouble)
    bad = ~np.isfinite(ref).all(axis=2, keepdims=True)
    a = np.abs(Z) if flooring_fn is None else flooring_fn(np.abs(Z))
    good = np.broadcast_to(~bad, Z.shape)
    a, zeta = np.where(good, a, 1), np.where(good, np.log(np.where(good, a, 1)), 0)
    e0 = np.max((4 * N + 8) * U * np.where(good, size, 0) / a + 2 * U * np.abs(zeta) + 2 * U,
                axis=2, keepdims=True).astype(np.float64)
    zm, R = float(np.max(np.abs(zeta))), float(np.max(np.abs(rho[good])))
    P, vm = float(np.max(np.abs(product[good]))), float(np.max(np.abs(ref[good])))
    e_mean = e0 + F * U * zm
    e_rho = 2 * e0 + (F + 1) * U * zm
    H = (1 + (np.pi / 2) ** mask_iter) * max(1.0, R)
    e_p = H * (e_rho + (F + 6) * U * R + 8 * U * max(1.0, R))
    bar = n * e_p + (F + 6) * U * n * P + e_mean + 4 * U * vm
    return ref, bar, bad


def _check_cepstral_pass(shape, floor, mask_iters):
    from ssspy_amd import _lib, _ops

    B, N, F, T = shape
    X, W2, dual, Z, size = _cepstrum_inputs(shape)
    kind, eps, flooring_fn = FLOORS[floor]
    power_of_two = (F - 1) & (F - 2) == 0
    auto = _ops.hva_route(F)
    assert auto == (_lib.HVA_ROUTE_FFT if power_of_two else _lib.HVA_ROUTE_DIRECT)
    assert _ops.hva_route(F, _lib.HVA_ROUTE_DIRECT) == _lib.HVA_ROUTE_DIRECT
    if not power_of_two:
        with pytest.raises(ValueError):
            _ops.hva_route(F, _lib.HVA_ROUTE_FFT)
    routes = [_lib.HVA_ROUTE_AUTO, _lib.HVA_ROUTE_DIRECT] if power_of_two else [_lib.HVA_ROUTE_AUTO]
    dX, dW2, dd = _dev(X), _dev(W2), _dev(dual)
    table = _ops.hva_cos_table(F, dX.device)
    for mask_iter in mask_iters:
        ref, bar, bad = cepstrum_bar(Z, size, flooring_fn, mask_iter)
        assert bad.any() == (floor == "none") and not bad.all()
        assert float(np.max(bar)) < 1e-5  # (the bar itself stays far under the size of varrho)
        got = []
        for route in routes:
            out = _host(_ops.hva_cepstrum(dX, dW2, dd, 0, table, (kind, eps), mask_iter, route=route))
            assert out.shape == shape and out.dtype == np.float64
            nan = np.isnan(out)
            assert np.array_equal(nan, np.broadcast_to(bad, shape))  # log 0 as in NumPy, no more
            err = np.where(nan, 0, np.abs(out - ref.astype(np.float64)))
            worst = float(np.max(err / bar))
            print("cepstrum", shape, floor, mask_iter, route, "max err {:.2e} err/bar {:.3f}".format(
                float(np.max(err)), worst))
            assert worst < 1
            got.append(np.where(nan, 0, out))
        if len(got) == 2:  # the two routes agree within the same bar
            assert float(np.max(np.abs(got[0] - got[1]) / bar)) < 1
    assert np.array_equal(_host(dd), dual)  # the pass leaves the dual variable alone


@pytest.mark.parametrize("floor", list(FLOORS))
@pytest.mark.parametrize("shape", CEPSTRUM_SHAPES, ids=lambda s: "b{}_n{}_f{}_t{}".format(*s))
def test_cepstral_pass_elementwise(shape, floor):
    _check_cepstral_pass(shape, floor, (0, 1, 3))


@pytest.mark.parametrize("floor", ["none", "max"])
def test_cepstral_pass_at_an_stft_size(floor):
    """F = 1025: the slab cap, not the frame count, sets the tile (8 frames on the FFT route, 4 on the
    direct sum), 9 frames make a second, short tile."""
    _check_cepstral_pass((1, 2, 1025, 9), floor, (1,))


def test_cosine_table():
    from ssspy_amd import _ops

    for F in (2, 3, 6, 12, 33, 100, 1025):
        table = _host(_ops.hva_cos_table(F, _dev(np.zeros(1)).device))
        j = np.arange(2 * (F - 1), dtype=np.longdouble)
        want = np.cos(4 * np.arctan(np.longdouble(1)) * j / (F - 1)).astype(np.float64)
        assert np.max(np.abs(table - want)) <= 2 * U  # an ulp of a number below one
        assert table[0] == 1 and table[F - 1] == -1
        if F % 2:
            assert table[(F - 1) // 2] == 0 and table[3 * (F - 1) // 2] == 0


def test_cepstral_pass_refusals():
    from ssspy_amd import _lib, _ops

    with pytest.raises(ValueError):
        _ops.hva_route(1)
    with pytest.raises(ValueError):
        _ops.hva_route(8193)
    assert _ops.hva_route(4097) == _lib.HVA_ROUTE_FFT and _ops.hva_route(1025) == _lib.HVA_ROUTE_FFT
    assert _ops.hva_route(2049) == _lib.HVA_ROUTE_FFT and _ops.hva_route(8192) == _lib.HVA_ROUTE_DIRECT
    X, W2, dual, _, _ = _cepstrum_inputs((1, 5, 12, 129))
    dX, dW2, dd = _dev(X), _dev(W2), _dev(dual)
    table = _ops.hva_cos_table(12, dX.device)
    with pytest.raises(NotImplementedError):
        _ops.hva_cepstrum(dX, dW2, dd, 0, table, (0, 0.0), 1, route=_lib.HVA_ROUTE_FFT)


# ------------------------------------------------------------------ the masked dual step
@pytest.mark.parametrize("relax", [1.0, 1.25])
@pytest.mark.parametrize("shape", [(2, 3, 5, 70), (1, 2, 3, 300), (1, 9, 4, 40), (1, 16, 2, 7)],
                         ids=lambda s: "b{}_n{}_f{}_t{}".format(*s))
def test_masked_dual_step(shape, relax):
    """Against the reference's expression; in one column the spread of varrho is 800, where exp(2
    varrho) overflows and the reference's expression is inf / inf: finite here, and equal to the
    expression with the maximum subtracted."""
    from ssspy_amd import _ops

    B, N, F, T = shape
    rng = np.random.default_rng(60 + N)
    X, W2 = _crandn(rng, B, N, F, T), _crandn(rng, B, F, N, N) / np.sqrt(N)
    dual = _crandn(rng, B, 1, N, F, T)
    varrho = 3 * rng.standard_normal((B, N, F, T))
    varrho[0, 0, 1, 2], varrho[0, 1, 1, 2] = 400.0, -400.0
    gamma = 0.4
    Z = dual[:, 0] + np.einsum("bfnm,bmft->bnft", W2, X)
    with np.errstate(over="ignore", invalid="ignore"):
        plain = hn.mask_of(varrho, gamma)
    stable = hn.stable_mask_of(varrho, gamma)
    overflowed = ~np.isfinite(plain)
    assert overflowed[0, :, 1, 2].any() and overflowed.sum() <= N and np.isfinite(stable).all()
    assert rel_err(stable[~overflowed], plain[~overflowed]) < 1e-13
    dd = _dev(dual)
    _ops.hva_dual_step(_dev(X), _dev(W2), dd, 0, _dev(varrho, dtype=np.float64), gamma, relax)
    got = _host(dd)[:, 0]
    assert np.isfinite(got).all()
    for mask, keep in ((plain, ~overflowed), (stable, np.ones_like(overflowed))):
        want = relax * (Z - mask * Z) + (1 - relax) * dual[:, 0]
        assert rel_err(got[keep], want[keep]) < OP_TOL
    # the column that overflows, on its own (it would vanish in the norm of the whole)
    want = relax * (Z - stable * Z) + (1 - relax) * dual[:, 0]
    assert rel_err(got[0, :, 1, 2], want[0, :, 1, 2]) < OP_TOL


# ------------------------------------------------------------------ the classes
def _construct(spec, **extra):
    return hc.construct(_hva(), _fl(), spec, **extra)


@pytest.mark.parametrize("name", hc.CASES)
def test_separators_replay_golden(name):
    g = load_golden(name)
    spec = hc.golden_spec(g)
    snap, seen = pc.Snapshots(), []

    def look(method):  # callbacks see NumPy arrays of the right shapes
        seen.append(all(isinstance(getattr(method, k), np.ndarray) and getattr(method, k).shape == v
                        for k, v in (("output", g["X"].shape), ("dual", g["X"].shape),
                                     ("demix_filter", g["final_demix_filter"].shape))))

    m = _construct(spec, callbacks=[snap, look])
    assert (m.device_floor() is None) == (spec["flooring"] == "lambda")
    init = pc.golden_init(g)
    Y = m(g["X"], n_iter=spec["n_iter"], **init)
    pc.check_against_golden(g, m, Y, snap, TOL, None, show=name)
    assert len(seen) == spec["n_iter"] + 1 and all(seen)
    assert m.attenuation == (spec["attenuation"] or 1 / spec["N"])
    if init:
        assert np.array_equal(init["demix_filter"], g["demix_filter0"])
        assert np.array_equal(init["dual"], g["dual0"])


# Shapes no fixture has.  The seeds are chosen on the restatement alone, by the fixture generator's
# criterion: run against itself on an input perturbed by 1e-15 relative (three trials) it stays
# within 1e-10 in filters, dual variable and output (the figure it moves by is beside each case).
PARITY = {
    "n2_long_fft": dict(N=2, F=17, T=300, seed=1, relaxation=1.25),            # 2.8e-15
    "n5_direct": dict(N=5, F=10, T=70, seed=2, mask_iter=2, attenuation=0.3),  # 3.9e-15
    "n16_add": dict(N=16, F=5, T=130, seed=3, flooring="add", cls="HVA"),      # 5.5e-15
    "n3_f2_none": dict(N=3, F=2, T=33, seed=4, flooring="none", mask_iter=0,   # 1.3e-14
                       scale_restoration="projection_back"),
}


def _parity_input(spec):
    X = pc.laplace_mixture(spec["seed"], spec["N"], spec["F"], spec["T"])
    return hc.construct(hn.CLASSES, hn, spec).normalize_by_spectral_norm(X)


@pytest.mark.parametrize("name", list(PARITY))
def test_classes_match_restatement(name):
    spec = dict(hc.DEFAULTS, **PARITY[name])
    X = _parity_input(spec)
    ref = hc.construct(hn.CLASSES, hn, spec)
    Yr = ref(X, n_iter=spec["n_iter"])
    m = _construct(spec)
    Y = m(X, n_iter=spec["n_iter"])
    errs = (rel_err(m.demix_filter, ref.demix_filter), rel_err(m.dual, ref.dual), rel_err(Y, Yr))
    print(name, errs)
    assert max(errs) < TOL
    assert repr(m) == repr(ref)


def test_batch_of_three_equals_the_single_calls():
    spec = dict(hc.DEFAULTS, N=3, F=9, T=70, mask_iter=2, relaxation=1.25)
    X = np.stack([_parity_input(dict(spec, seed=5 + 20 * b)) for b in range(3)])
    m = _construct(spec)
    Y = m(X, n_iter=10)
    assert m.dual.shape == (3, 3, 9, 70) and m.demix_filter.shape == (3, 9, 3, 3)
    for b in range(3):
        single = _construct(spec)
        Ys = single(X[b], n_iter=10)
        assert single.dual.shape == (3, 9, 70)
        assert max(rel_err(m.demix_filter[b], single.demix_filter), rel_err(m.dual[b], single.dual),
                   rel_err(Y[b], Ys)) < OP_TOL


@pytest.mark.parametrize("floor", ["max", "add", "none"])
def test_device_route_equals_compatibility_route(floor):
    """The same flooring behind a lambda is not recognised: the inherited update_once with the host
    mask_fn, Z to the host and the mask back up."""
    spec = dict(hc.DEFAULTS, N=4, F=9, T=70, seed=2, flooring=floor, relaxation=1.25)
    X = np.stack([_parity_input(dict(spec, seed=2 + 20 * b)) for b in range(2)])
    named = hc.flooring_of(floor, _fl()) or _fl().identity
    m = _construct(spec)
    host = _hva().MaskingPDSHVA(**dict(hc.build_kwargs(spec, _fl()), flooring_fn=lambda x: named(x)))
    assert m.device_floor() is not None and host.device_floor() is None
    Y, Yh = m(X, n_iter=10), host(X, n_iter=10)
    errs = (rel_err(m.demix_filter, host.demix_filter), rel_err(m.dual, host.dual), rel_err(Y, Yh))
    print(floor, errs)
    assert max(errs) < TOL


def test_both_transform_routes_in_the_class():
    from ssspy_amd import _lib

    spec = dict(hc.DEFAULTS, N=3, F=17, T=70, seed=2)
    X = _parity_input(spec)
    m, direct = _construct(spec), _construct(spec)
    direct._transform_route = _lib.HVA_ROUTE_DIRECT
    assert m.transform_route(17) == _lib.HVA_ROUTE_FFT
    assert direct.transform_route(17) == _lib.HVA_ROUTE_DIRECT
    assert m.transform_route(12) == _lib.HVA_ROUTE_DIRECT
    Y, Yd = m(X, n_iter=10), direct(X, n_iter=10)
    assert max(rel_err(m.demix_filter, direct.demix_filter), rel_err(m.dual, direct.dual),
               rel_err(Y, Yd)) < OP_TOL


def test_update_once_by_hand_equals_call():
    spec = dict(hc.DEFAULTS, N=3, F=9, T=70, seed=2, scale_restoration=False)
    X = _parity_input(spec)
    m = _construct(spec)
    Y = m(X, n_iter=10)
    hand = _construct(spec)
    hand(X, n_iter=0)
    for _ in range(10):
        hand.update_once()
    assert np.array_equal(np.asarray(hand.demix_filter), np.asarray(m.demix_filter))
    assert np.array_equal(np.asarray(hand.dual), np.asarray(m.dual))
    assert rel_err(hand.separate(X, hand.demix_filter), Y) < OP_TOL


@pytest.mark.parametrize("name", ["n2_long_fft", "n5_direct"])
def test_two_runs_are_bit_identical(name):
    spec = dict(hc.DEFAULTS, **PARITY[name])
    X = _parity_input(spec)
    runs = []
    for _ in range(2):
        m = _construct(spec)
        Y = m(X, n_iter=10)
        runs.append((Y, np.array(m.demix_filter), np.array(m.dual)))
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_refusals():
    with pytest.raises(NotImplementedError, match="up to 16 sources"):
        _hva().MaskingPDSHVA()(pc.laplace_mixture(1, 17, 2, 40), n_iter=1)
    for floor in ("max", "lambda"):  # a single bin, on either route
        m = _hva().HVA(flooring_fn=hc.flooring_of(floor, _fl()))
        with pytest.raises(ValueError, match="Invalid number of FFT data points"):
            m(pc.laplace_mixture(1, 2, 1, 40), n_iter=1)
