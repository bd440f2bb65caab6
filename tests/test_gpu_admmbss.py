"""ADMMBSS / MaskingADMMBSS / ADMMIVA / PDSIVA on the device: every entry point of csrc/admmbss.hip on
its own against NumPy in extended precision (np.clongdouble; tests/prox_reference.py for the
proximal operator of -log|det|), the classes against the golden vectors of the reference, and the
equalities between the ways to run the same thing.

Bars (those of tests/test_gpu_pdsbss.py): 1e-8 relative Frobenius on filters, states and outputs,
rtol 1e-9 on the finite loss entries (non-finite ones by position and sign), 1e-10 on single
operators and on every equality.
"""

import warnings

import numpy as np
import pytest

import admmbss_cases as ac
import admmbss_numpy as an
import pdsbss_cases as pc
import prox_reference as pr
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL, LOSS_RTOL, OP_TOL = 1e-8, 1e-9, 1e-10
EXT = np.clongdouble


def _admm():
    from ssspy_amd.bss import admmbss

    return admmbss


def _ns():
    """A namespace with every class under test."""
    from ssspy_amd.bss import admmbss, iva

    return {"ADMMBSS": admmbss.ADMMBSS, "MaskingADMMBSS": admmbss.MaskingADMMBSS,
            "ADMMIVA": iva.ADMMIVA, "PDSIVA": iva.PDSIVA}


def _prox():
    from ssspy_amd.linalg import prox

    return prox


def _dev(a, dtype=np.complex128):
    from ssspy_amd import _device as dv

    return dv.to_device(np.ascontiguousarray(a), dtype=dtype)


def _host(t):
    from ssspy_amd import _device as dv

    return dv.to_host(t)


def _crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ------------------------------------------------------------------ the zero-matrix convention
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 8, 9, 16])
def test_neg_logdet_of_the_zero_matrix_is_a_scaled_identity(N):
    """What the filter step relies on in the first iteration from the zero state: for an argument that
    is exactly zero the existing routine returns sqrt(step_size) I, the value the reference gets from
    LAPACK (U = V = I)."""
    zero = np.zeros((3, N, N), dtype=complex)
    for step in (0.25, 1.0, 2.0, 1e3):
        got = _prox().neg_logdet(zero, step_size=step)
        assert rel_err(got, np.sqrt(step) * np.broadcast_to(np.eye(N), zero.shape)) < 1e-15
        assert not np.any(got[:, ~np.eye(N, dtype=bool)])


# ------------------------------------------------------------------ the passes
# N = 2 .. 16 over both forms of every kernel (the size at compile time up to 8, at run time above; G
# = 2, 4, 8, 16); F = 3 and 33: a partial wave of bins in the lane-per-bin kernels, and two bins per
# chunk with a short last chunk in the norm pass over bins; T = 1, 63 and 257: the frame tail and more
# than one walk of a workgroup's 256 threads; B = 1 and 3.
PASS_SHAPES = [(3, 2, 3, 1), (1, 2, 33, 257), (3, 3, 33, 63), (1, 4, 33, 257), (3, 5, 3, 257),
               (1, 8, 3, 63), (3, 9, 33, 1), (1, 9, 3, 63), (1, 16, 3, 257), (3, 16, 3, 63)]
_ids = dict(ids=lambda s: "b{}_n{}_f{}_t{}".format(*s))


def _gram(X, Q):
    """Q conj(X) X^T + I per bin in extended precision, (B, F, N, N)."""
    Xe = X.astype(EXT)
    return Q * np.einsum("bmft,bkft->bfmk", Xe.conj(), Xe) + np.eye(X.shape[1], dtype=EXT)


@pytest.mark.parametrize("shape", PASS_SHAPES, **_ids)
def test_gram_inverse_pass(shape):
    """The residual A Ainv - I with A in extended precision; kappa(A) is printed (below 1e3 here)."""
    from ssspy_amd import _ops

    B, N, F, T = shape
    rng = np.random.default_rng(100 + N)
    X = 0.3 * _crandn(rng, B, N, F, T)
    for Q in (1, 3):
        got = _host(_ops.admmbss_gram_inverse(_dev(X), Q))
        A = _gram(X, Q)
        res = np.einsum("bfmk,bfkn->bfmn", A, got.astype(EXT)) - np.eye(N)
        err = float(np.max(np.sqrt(np.sum(np.abs(res) ** 2, axis=(-2, -1)))))
        kappa = float(np.max(np.linalg.cond(A.astype(np.complex128))))
        print("gram_inverse", shape, Q, err, kappa)
        assert kappa < 1e3 and err < OP_TOL
        assert rel_err(got, np.conj(np.swapaxes(got, -1, -2))) < 1e-15  # Hermitian


@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("shape", PASS_SHAPES, **_ids)
def test_contraction_pass(shape, Q):
    from ssspy_amd import _ops

    B, N, F, T = shape
    rng = np.random.default_rng(11)
    X, aux2, dual2 = _crandn(rng, B, N, F, T), _crandn(rng, B, Q, N, F, T), _crandn(rng, B, Q, N, F, T)
    got = _host(_ops.admmbss_contract(_dev(aux2), _dev(dual2), _dev(X)))
    diff = (aux2.astype(EXT) - dual2.astype(EXT)).sum(axis=1)
    want = np.einsum("bnft,bmft->bfnm", diff, X.astype(EXT).conj()).astype(np.complex128)
    err = max(rel_err(g, w) for g, w in zip(got.reshape(B * F, N, N), want.reshape(B * F, N, N)))
    print("contract", shape, Q, err)
    assert err < OP_TOL


@pytest.mark.parametrize("relax", [1.0, 1.5])
@pytest.mark.parametrize("N", [2, 3, 4, 5, 8, 9, 16])
def test_filter_step_pass(N, relax):
    """Per bin against the extended reference (99 bins up to 5 sources: a second workgroup and a
    partial wave; 33 above, where the reference takes a second per size); bins 0 and 20 have an
    all-zero right-hand side and dual1, so their argument is exactly zero: W = 0 and auxiliary1 =
    sqrt(1 / rho) I there."""
    from ssspy_amd import _ops

    rng = np.random.default_rng(20 + N)
    B, F, rho = (3 if N <= 5 else 1), 33, 0.5
    X = 0.3 * _crandn(rng, B, N, F, 40)
    Ainv = np.linalg.inv(_gram(X, 1).astype(np.complex128))
    aux1 = np.eye(N) + 0.3 * _crandn(rng, B, F, N, N)
    dual1, R = 0.2 * _crandn(rng, B, F, N, N), 0.5 * _crandn(rng, B, F, N, N)
    for t in (aux1, dual1, R):
        t.reshape(B * F, N, N)[[0, 20]] = 0
    dW, da, dd = _dev(np.full_like(R, np.nan)), _dev(aux1), _dev(dual1)
    _ops.admmbss_filter_step(_dev(Ainv), _dev(R), dW, da, dd, rho, relax)
    W = np.einsum("bfmk,bfkn->bfmn", Ainv.astype(EXT), aux1.astype(EXT) - dual1 + R)
    U = relax * W + (1 - relax) * aux1
    V = pr.neg_logdet(U + dual1, 1 / rho)
    Y = dual1 + U - V

    def per_bin(got, want):
        got, want = got.reshape(B * F, -1), want.astype(np.complex128).reshape(B * F, -1)
        denom = np.linalg.norm(want, axis=1)
        return np.max(np.linalg.norm(got - want, axis=1) / np.where(denom > 0, denom, 1.0))

    errs = (per_bin(_host(dW), W), per_bin(_host(da), V), per_bin(_host(dd), Y))
    print("filter_step", N, relax, errs)
    assert max(errs) < OP_TOL
    for k in (0, 20):
        assert not np.any(_host(dW).reshape(B * F, N, N)[k])
        assert rel_err(_host(da).reshape(B * F, N, N)[k], np.sqrt(1 / rho) * np.eye(N)) < 1e-15


KINDS = ["l1", "l21_sources", "l21_bins", "l21_frames"]
AXES = {"l1": None, "l21_sources": 0, "l21_bins": 1, "l21_frames": 2}


def _aux_inputs(shape, Q, q, seed=31):
    """X, W, auxiliary2, dual2 with an exactly zero group of Z under every axis in mixture 0: frame 0,
    bin 0 and source 0."""
    B, N, F, T = shape
    rng = np.random.default_rng(seed)
    X, W = _crandn(rng, B, N, F, T), _crandn(rng, B, F, N, N) / np.sqrt(N)
    aux2, dual2 = _crandn(rng, B, Q, N, F, T), _crandn(rng, B, Q, N, F, T)
    X[0, :, :, 0] = 0
    X[0, :, 0, :] = 0
    W[0, :, 0, :] = 0
    for S in (aux2, dual2):
        S[0, q, :, :, 0] = 0
        S[0, q, :, 0, :] = 0
        S[0, q, 0] = 0
    return X, W, aux2, dual2


def _z_ext(X, W, aux2_q, dual2_q, relax):
    """Z in extended precision; with relaxation 1 auxiliary2 takes no part."""
    Y = np.einsum("bfnm,bmft->bnft", W.astype(EXT), X.astype(EXT))
    if relax == 1:
        return Y + dual2_q
    return relax * Y + (1 - relax) * aux2_q.astype(EXT) + dual2_q


def _prox_ext(Z, kind, step):
    norm = np.abs(Z) if AXES[kind] is None else \
        np.sqrt(np.sum(np.abs(Z) ** 2, axis=AXES[kind] + 1, keepdims=True))
    norm = np.where(norm < step, step, norm)
    return np.maximum(1 - step / norm, 0) * Z


@pytest.mark.parametrize("relax", [1.0, 1.5])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", PASS_SHAPES, **_ids)
def test_aux_step_pass(shape, kind, relax):
    """The step sits inside the range of the norms (both sides of it occur) and one whole group of Z
    is exactly zero: 0 there, not NaN.  With relaxation 1 auxiliary2 is not read: it holds NaN."""
    from ssspy_amd import _lib, _ops

    B, N, F, T = shape
    Q, q = 2, 1
    X, W, aux2, dual2 = _aux_inputs(shape, Q, q)
    Z = _z_ext(X, W, aux2[:, q], dual2[:, q], relax)
    norms = np.abs(Z) if AXES[kind] is None else np.sqrt(np.sum(np.abs(Z) ** 2, axis=AXES[kind] + 1))
    step = float(np.median(norms[norms > 0]))
    assert np.any(norms < step) and np.any(norms == 0)
    assert np.any(norms > step) or norms[norms > 0].size == 1
    V = _prox_ext(Z, kind, step)
    if relax == 1:
        aux2[:, q] = np.nan
    dX, dW, da, dd = _dev(X), _dev(W), _dev(aux2), _dev(dual2)
    r2 = None
    if kind == "l21_bins":
        r2 = _ops.admmbss_bin_norms(dX, dW, da, dd, q, relax)
        assert rel_err(_host(r2), np.sum(np.abs(Z) ** 2, axis=2).astype(np.float64)) < OP_TOL
    assert rel_err(_host(_ops.admmbss_form_z(dX, dW, da, dd, q, relax)),
                   Z.astype(np.complex128)) < OP_TOL
    _ops.admmbss_aux_step(dX, dW, da, dd, q, getattr(_lib, "PROX_" + kind.upper()), step, relax,
                          r2=r2)
    got_a, got_d = _host(da), _host(dd)
    assert np.isfinite(got_a[:, q]).all() and np.isfinite(got_d).all()
    # the other penalty's slices are untouched
    assert np.array_equal(got_a[:, 0], aux2[:, 0]) and np.array_equal(got_d[:, 0], dual2[:, 0])
    errs = (rel_err(got_a[:, q], V.astype(np.complex128)),
            rel_err(got_d[:, q], (Z - V).astype(np.complex128)))
    print("aux_step", shape, kind, relax, errs)
    assert max(errs) < OP_TOL


@pytest.mark.parametrize("relax", [1.0, 1.5])
def test_mask_and_given_passes(relax):
    from ssspy_amd import _lib, _ops

    shape = (3, 3, 5, 70)
    X, W, aux2, dual2 = _aux_inputs(shape, 1, 0, seed=41)
    rng = np.random.default_rng(42)
    Z = _z_ext(X, W, aux2[:, 0], dual2[:, 0], relax).astype(np.complex128)
    mask, V = rng.random(shape), _crandn(rng, *shape)
    for kind, given, want in ((_lib.PROX_MASK, mask, mask * Z), (_lib.PROX_GIVEN, V, V)):
        da, dd = _dev(aux2), _dev(dual2)
        _ops.admmbss_aux_step(_dev(X), _dev(W), da, dd, 0, kind, 1.0, relax, given=_dev(given))
        assert rel_err(_host(da)[:, 0], want) < OP_TOL
        assert rel_err(_host(dd)[:, 0], Z - want) < OP_TOL


@pytest.mark.parametrize("shape", [(2, 3, 5, 70), (1, 16, 2, 7), (1, 2, 1, 257)], **_ids)
def test_z_at_relaxation_one_is_the_pds_z(shape):
    """The Z formers of the two families are kept in step by hand: at relaxation 1 the ADMM Z and its
    norms over bins are those of PDSBSS bit for bit, and auxiliary2 (NaN here) is not read."""
    from ssspy_amd import _ops

    B, N, F, T = shape
    rng = np.random.default_rng(53)
    dX, dW = _dev(_crandn(rng, B, N, F, T)), _dev(_crandn(rng, B, F, N, N) / np.sqrt(N))
    dd = _dev(_crandn(rng, B, 1, N, F, T))
    da = _dev(np.full((B, 1, N, F, T), np.nan + 1j * np.nan))
    Z = _host(_ops.pdsbss_form_z(dX, dW, dd, 0))
    assert np.isfinite(Z).all()
    assert np.array_equal(_host(_ops.admmbss_form_z(dX, dW, da, dd, 0, 1.0)), Z)
    assert np.array_equal(_host(_ops.admmbss_bin_norms(dX, dW, da, dd, 0, 1.0)),
                          _host(_ops.pdsbss_bin_norms(dX, dW, dd, 0)))


# ------------------------------------------------------------------ the classes
def _construct(ns, prox_ns, spec, **extra):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return ns[spec["cls"]](**ac.build_kwargs(spec, prox_ns), **extra)


@pytest.mark.parametrize("name", ac.CASES)
def test_separators_replay_golden(name):
    """Every fixture through the public classes (the batched one as one (B, N, F, T) call)."""
    g = load_golden(name)
    spec = ac.golden_spec(g)
    snap, seen = ac.Snapshots(spec["cls"]), []

    def look(method):  # callbacks see NumPy arrays of the reference's shapes
        seen.append(all(isinstance(getattr(method, k), np.ndarray)
                        and getattr(method, k).shape == g["it1_" + k].shape for k in snap.names))

    m = _construct(_ns(), _prox(), spec, callbacks=[snap, look])
    init = ac.golden_init(g)
    Y = m(g["X"], n_iter=spec["n_iter"], **init)
    ac.check_against_golden(g, m, Y, snap, TOL, LOSS_RTOL, show=name)
    assert len(seen) == spec["n_iter"] + 1 and all(seen)
    for key, value in init.items():  # injected arrays are copied, never mutated
        assert np.array_equal(value, g[key + "0"])
    if spec["cls"] != "PDSIVA" and not init:
        # the first iteration from the zero state: W = 0 exactly, and +inf in the loss list there
        assert not np.any(snap.store["it1_demix_filter"])
        if m.loss is not None:
            assert np.all(np.asarray(m.loss[1]) == np.inf)


# Shapes no fixture has, against the restatement.  The seeds are chosen on the restatement alone, by
# the fixture generator's criterion (1e-10 under a 1e-15 perturbation, three trials).
PARITY = {
    "n16": dict(N=16, F=5, T=64, penalties=["l21_bins"]),
    # (seed 7: the restatement moves by 3.0e-12; at seeds 1, 2 and 3 by 3.5e-10, 4.9e-9 and 1.2e-7)
    "q3": dict(N=3, F=9, T=70, seed=7, penalties=["l21_bins", "l1", "l21_sources"], rho=2.0,
               relaxation=1.25, record_loss=True, scale_restoration="projection_back"),
    # (two sources and more than 128 frames: both waves of a row of the contraction hold data; seed
    # 6: the restatement moves by 6.7e-14, at seeds 1 and 3 by 2.4e-10 and 2.7e-8)
    "n2_long": dict(N=2, F=5, T=300, seed=6, penalties=["l21_frames"], relaxation=1.25),
    "masking": dict(N=4, F=9, T=70, seed=2, cls="MaskingADMMBSS", penalties=["mask"],
                    record_loss=True, relaxation=1.25),
}


def _stable(spec, X):
    """The generator's gate on the restatement: how far it moves under 1e-15 relative."""
    def run(Xin):
        m = _construct(an.CLASSES, an, spec)
        Y = m(Xin, n_iter=spec["n_iter"])
        return [Y, m.demix_filter] + [getattr(m, k) for k in ac.ADMM_STATES]

    base, rng, worst = run(X), np.random.default_rng(spec["seed"] + 11), 0.0
    for _ in range(3):
        moved = run(X * (1 + 1e-15 * rng.standard_normal(X.shape)))
        worst = max([worst] + [rel_err(a, b) for a, b in zip(moved, base)])
    return worst


@pytest.mark.parametrize("name", list(PARITY))
def test_classes_match_restatement(name):
    spec = dict(ac.DEFAULTS, **PARITY[name])
    X = ac.mixtures(spec)
    moved = _stable(spec, X)
    print(name, "restatement moves by", moved)
    assert moved < 1e-10
    ref = _construct(an.CLASSES, an, spec)
    Yr = ref(X, n_iter=spec["n_iter"])
    m = _construct(_ns(), _prox(), spec)
    Y = m(X, n_iter=spec["n_iter"])
    errs = [rel_err(Y, Yr), rel_err(m.demix_filter, ref.demix_filter)] + \
        [rel_err(getattr(m, k), getattr(ref, k)) for k in ac.ADMM_STATES]
    print(name, errs)
    assert max(errs) < TOL
    if ref.loss is not None:
        ac.check_loss(m.loss, ref.loss, LOSS_RTOL)


@pytest.mark.parametrize("kind", KINDS)
def test_device_route_equals_compatibility_route(kind):
    """The same operator behind a lambda is not recognised and takes the compatibility path."""
    from ssspy_amd.bss.proxbss import device_prox

    spec = dict(ac.DEFAULTS, N=4, F=9, T=70, B=2, seed=2, penalties=[kind])
    X = ac.mixtures(spec)
    named = pc.prox_of(kind, _prox())
    kw = dict(relaxation=1.25, record_loss=False)
    m = _admm().ADMMBSS(prox_penalty=named, **kw)
    closure = _admm().ADMMBSS(prox_penalty=lambda z, step_size=1: named(z, step_size=step_size), **kw)
    assert device_prox(m.prox_penalty[0]) is not None
    assert device_prox(closure.prox_penalty[0]) is None
    Y, Yc = m(X, n_iter=10), closure(X, n_iter=10)
    errs = [rel_err(Y, Yc), rel_err(m.demix_filter, closure.demix_filter)] + \
        [rel_err(getattr(m, k), getattr(closure, k)) for k in ac.ADMM_STATES]
    print(kind, errs)
    assert max(errs) < OP_TOL


def test_batch_equals_single_runs():
    """B = 3 with a user closure among the penalties: every mixture against its own single run
    (1e-10); the callable sees one (n_sources, n_bins, n_frames) mixture at a time."""
    spec = dict(ac.DEFAULTS, N=3, F=9, T=70, B=3, penalties=["l21_bins", "elastic"],
                record_loss=True, relaxation=1.25)
    X = ac.mixtures(spec)
    seen = []

    def watched(z, step_size=1):
        seen.append(z.shape)
        return pc.prox_elastic(z, step_size=step_size)

    m = _construct(_ns(), _prox(), spec)
    m.prox_penalty[1] = watched
    Y = m(X, n_iter=10)
    assert set(seen) == {(3, 9, 70)} and len(seen) == 30
    assert m.auxiliary2.shape == m.dual2.shape == (3, 2, 3, 9, 70)
    assert m.auxiliary1.shape == m.dual1.shape == m.demix_filter.shape == (3, 9, 3, 3)
    loss = np.array(m.loss)
    assert loss.shape == (11, 3)
    for b in range(3):
        single = _construct(_ns(), _prox(), spec)
        Ys = single(X[b], n_iter=10)
        errs = [rel_err(Y[b], Ys), rel_err(m.demix_filter[b], single.demix_filter)] + \
            [rel_err(getattr(m, k)[b], getattr(single, k)) for k in ac.ADMM_STATES]
        assert max(errs) < OP_TOL
        ac.check_loss(loss[:, b], single.loss, OP_TOL)


@pytest.mark.parametrize("name", ["q3", "masking"])
def test_two_runs_are_bit_identical(name):
    spec = dict(ac.DEFAULTS, **PARITY[name])
    X = ac.mixtures(spec)
    runs = []
    for _ in range(2):
        m = _construct(_ns(), _prox(), spec)
        Y = m(X, n_iter=10)
        runs.append([Y, np.array(m.demix_filter), np.array(m.loss)] +
                    [np.array(getattr(m, k)) for k in ac.ADMM_STATES])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_default_state_equals_injected_zero_state():
    """Also through the deprecated ``aux1`` / ``aux2`` keywords, which warn."""
    spec = dict(ac.DEFAULTS, N=3, F=9, T=40, penalties=["l21_bins", "l1"])
    X = ac.mixtures(spec)
    m = _construct(_ns(), _prox(), spec)
    Y = m(X, n_iter=5)
    zero1, zero2 = np.zeros((9, 3, 3), dtype=complex), np.zeros((2, 3, 9, 40), dtype=complex)
    injected = _construct(_ns(), _prox(), spec)
    Yi = injected(X, n_iter=5, auxiliary1=zero1, dual1=zero1, auxiliary2=zero2, dual2=zero2)
    old = _construct(_ns(), _prox(), spec)
    with pytest.warns(DeprecationWarning, match="aux[12] is deprecated"):
        Yo = old(X, n_iter=5, aux1=zero1, aux2=zero2)
    for other, Yother in ((injected, Yi), (old, Yo)):
        assert np.array_equal(Y, Yother)
        for k in ("demix_filter",) + ac.ADMM_STATES:
            assert np.array_equal(np.asarray(getattr(m, k)), np.asarray(getattr(other, k)))
    assert not np.any(zero1) and not np.any(zero2)
    with pytest.raises(ValueError, match="auxiliary2 must have shape"):
        _construct(_ns(), _prox(), spec)(X, n_iter=1, auxiliary2=zero2[:1])


def test_more_than_16_sources_is_refused():
    X = ac.mixture(1, 17, 2, 40)
    with pytest.raises(NotImplementedError, match="up to 16 sources"):
        _admm().ADMMBSS(prox_penalty=_prox().l1, record_loss=False)(X, n_iter=1)
    with pytest.raises(NotImplementedError, match="up to 16 sources"):
        _admm().MaskingADMMBSS(mask_fn=ac.smooth_mask)(X, n_iter=1)
