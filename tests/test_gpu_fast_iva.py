"""FastIVA / FasterIVA, whiten / pca and their kernels on the device.

Whole runs replay every reference fixture through the public classes (outputs and W P at 1e-8
relative Frobenius, losses at rtol 1e-9) in the phase gauge of tests/fast_iva_cases.py; each kernel
is checked on its own against ``numpy.longdouble``; the contracts of the sibling classes hold.

Gauge handling of the two things the reference ties to LAPACK's eigenvector phases: an injected
``demix_filter`` acts on the whitened mixture, so it is handed over as W0 D^H with D the unit
factors between the device's whitened mixture and the fixture's; and the minimal distortion
principle refits the filters on the unwhitened input but applies them to the whitened one, so its
result depends on D -- there the expectation is the restatement run in the device's gauge (the
restatement in the fixture's gauge equals the fixture at 1e-11, tests/test_golden_fast_iva.py).
"""

import inspect
import re

import numpy as np
import pytest

import fast_iva_cases as fc
import fast_iva_numpy as fn
from conftest import load_golden

pytestmark = pytest.mark.gpu

OUT_TOL, LOSS_RTOL, OP_TOL, BATCH_TOL = 1e-8, 1e-9, 1e-10, 1e-10
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def amd():
    import ssspy_amd.bss.iva as iva
    import ssspy_amd.transform as transform
    from ssspy_amd import _device as dv, _lib, _ops
    from ssspy_amd.special import flooring
    return dict(iva=iva, transform=transform, dv=dv, lib=_lib, ops=_ops, flooring=flooring)


def build(amd, cfg, **over):
    kw = dict(flooring_fn=fc.flooring_for(cfg["flooring"], amd["flooring"]),
              scale_restoration=cfg["scale_restoration"], reference_id=cfg["reference_id"],
              **fc.closures_for(cfg["cls"], cfg["contrast"]))
    kw.update(over)
    return getattr(amd["iva"], cfg["cls"])(**kw)


# ------------------------------------------------------------------------------ whole runs
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_fixture_through_public_class(amd, name):
    g, cfg = load_golden(name), fc.settings(name)
    X, n_iter = g["X"], int(g["meta_n_iter"])
    D = fn.gauge_between(g["whitened_input"], amd["transform"].whiten(X))  # D Z_ref = Z_device
    snap = fc.ActionSnapshots()
    m = build(amd, cfg, callbacks=snap)
    init = {"demix_filter": fc.regauge_filter(g["demix_filter0"], D)} if cfg["init_filter"] else {}
    Y = m(X, n_iter=n_iter, **init)
    assert len(m.loss) == n_iter + 1
    np.testing.assert_allclose(m.loss, g["loss"], rtol=LOSS_RTOL)
    for key in ("it1_action", "it2_action"):
        assert fc.err_up_to_row_phase(snap.store[key], g[key]) <= OUT_TOL, key
    want_Y, want_A = g["final_output"], g["final_action"]
    if cfg["scale_restoration"] == "minimal_distortion_principle":
        from test_golden_fast_iva import replay
        r, _, want_Y, _ = replay(name, gauge_like=np.asarray(m.whitened_input), regauge=D)
        want_A = fc.filter_action(r)
    if cfg["scale_restoration"]:
        errs = fc.err(Y, want_Y), fc.err(fc.filter_action(m, X), want_A)
    else:
        errs = fc.err_up_to_row_phase(Y, want_Y), fc.err_up_to_row_phase(fc.filter_action(m, X), want_A)
    assert max(errs) <= OUT_TOL


@pytest.mark.parametrize("cls", ["FastIVA", "FasterIVA"])
@pytest.mark.parametrize("shape", [(2, 5, 17), (3, 7, 33), (4, 17, 70)])
def test_fresh_input_against_restatement(amd, cls, shape):
    cfg = dict(fc.DEFAULTS, cls=cls, contrast="smooth", scale_restoration="projection_back")
    X = fc.gen_mixture(900 + shape[0], *shape)
    m = build(amd, cfg)
    Y = m(X, n_iter=5)
    r = fn.CLASSES[cls](scale_restoration="projection_back", **fc.closures_for(cls, "smooth"))
    Yr = r(X, n_iter=5)
    np.testing.assert_allclose(m.loss, r.loss, rtol=LOSS_RTOL)
    assert fc.err(Y, Yr) <= OUT_TOL
    assert fc.err(fc.filter_action(m, X), fc.filter_action(r)) <= OUT_TOL


# --------------------------------------------------------------------- kernels on their own
def _ld(x):
    return np.asarray(x, dtype=np.clongdouble if np.iscomplexobj(x) else np.longdouble)


@pytest.mark.parametrize("N", [2, 3, 5, 8, 9, 16])
@pytest.mark.parametrize("B, F, T", [(1, 1, 1), (1, 16, 63), (3, 17, 64), (1, 17, 65), (3, 16, 130)])
def test_statistics_pass_elementwise(amd, N, B, F, T):
    """c, b, a against longdouble sums.  Error of a length-T sum of products formed from an N-term
    dot product: (T + 2 N + 4) eps times the sum of the moduli of its terms."""
    dv, ops = amd["dv"], amd["ops"]
    rng = np.random.default_rng(N * 1000 + F * 10 + T)
    Z = rng.standard_normal((B, N, F, T)) + 1j * rng.standard_normal((B, N, F, T))
    W = rng.standard_normal((B, F, N, N)) + 1j * rng.standard_normal((B, F, N, N))
    phi, psi = rng.random((B, N, T)), rng.standard_normal((B, N, T))
    phi[rng.random(phi.shape) < 0.2] = 0.0  # (some weights exactly zero)
    c, b, a = (dv.to_host(t) for t in ops.fast_iva_stats(
        dv.to_device(Z), dv.to_device(W), dv.to_device(phi), dv.to_device(psi)))
    Zl, Wl, pl, sl = _ld(Z), _ld(W), _ld(phi), _ld(psi)
    Y = np.einsum("bfnm,bmft->bnft", Wl, Zl)
    absY = np.einsum("bfnm,bmft->bnft", np.abs(Wl), np.abs(Zl))
    bound = (T + 2 * N + 4) * EPS
    c_ref = np.einsum("bnt,bnft,bmft->bfnm", pl, Y.conj(), Zl)
    c_mag = np.einsum("bnt,bnft,bmft->bfnm", pl, absY, np.abs(Zl))
    b_ref = np.einsum("bnt,bnft->bfn", sl, np.abs(Y) ** 2)
    b_mag = np.einsum("bnt,bnft->bfn", np.abs(sl), absY ** 2)
    a_ref = np.broadcast_to(pl.sum(-1)[:, None, :], (B, F, N))
    assert np.all(np.abs(c - c_ref) <= 2 * bound * c_mag + 1e-300)
    assert np.all(np.abs(b - b_ref) <= 2 * bound * b_mag + 1e-300)
    assert np.all(np.abs(a - a_ref) <= bound * a_ref + 1e-300)


def _conditioned_filters(rng, F, N, cond):
    """(1, F, N, N) with cond(W W^H) spread up to ``cond``."""
    A = rng.standard_normal((F, N, N)) + 1j * rng.standard_normal((F, N, N))
    u, _, vh = np.linalg.svd(A)
    s = np.sqrt(np.logspace(0, np.log10(cond), N))[np.newaxis, :] * np.ones((F, 1))
    s[0] = 1.0  # (one bin already unitary)
    return ((u * s[:, np.newaxis, :]) @ vh)[np.newaxis]


@pytest.mark.parametrize("N", [2, 3, 4, 5, 8, 9, 16])
def test_orthonormalize_rows(amd, N):
    dv, ops = amd["dv"], amd["ops"]
    rng = np.random.default_rng(40 + N)
    W = _conditioned_filters(rng, 17, N, 1e6)
    info = dv.zeros((1,), dv.i32)
    got = dv.to_host(ops.orthonormalize_rows(dv.to_device(W), info))
    assert int(info.item()) == 0
    _polar_checks(got, W, N)


def _polar_checks(got, M, N):
    """``got`` against the polar factor of M (formed in longdouble): unitary to 1e-12, and within the
    operator bar of numpy's SVD form u v^H, whose own error is of order eps cond(M) = 2e-13 at
    cond(M M^H) = 1e6."""
    Q = _ld(got)
    assert np.max(np.abs(Q @ Q.conj().swapaxes(-1, -2) - np.eye(N))) <= 1e-12
    assert fc.err(got, fn.polar_unitary(np.asarray(M, dtype=np.complex128))) <= OP_TOL


@pytest.mark.parametrize("N", [2, 3, 4, 5, 8, 9, 16])
def test_fast_step_against_longdouble_update(amd, N):
    """The moments are chosen so that the updated filter, before its rows are orthonormalised, is a
    matrix M with cond(M M^H) spread up to 1e6."""
    dv, ops = amd["dv"], amd["ops"]
    rng = np.random.default_rng(60 + N)
    F, T = 17, 40
    W = _conditioned_filters(rng, F, N, 10.0)
    M = _conditioned_filters(rng, F, N, 1e6)
    b, a = rng.standard_normal((1, F, N)), np.broadcast_to(rng.random((1, 1, N)) * T, (1, F, N)).copy()
    c = ((a - b)[..., None] * W - T * M).conj()
    info = dv.zeros((1,), dv.i32)
    got = dv.to_host(ops.fast_iva_step(dv.to_device(W), dv.to_device(c), dv.to_device(b),
                                       dv.to_device(a), T, info))
    new = ((_ld(a) - _ld(b))[..., None] * _ld(W) - _ld(c).conj()) / T
    assert int(info.item()) == 0
    _polar_checks(got, new, N)


@pytest.mark.parametrize("N", [2, 3, 4, 5, 8, 9, 16])
def test_faster_step_rows_are_principal_eigenvectors(amd, N):
    """Before the orthonormalisation row n is the conjugate principal eigenvector of U_n: checked
    through the step on U_n that share one orthonormal eigenbasis (then W^H holds the principal
    vectors themselves and the orthonormalisation changes nothing), up to a phase per row; the
    error of an eigenvector is of order eps / gap."""
    dv, ops = amd["dv"], amd["ops"]
    rng = np.random.default_rng(80 + N)
    F, gap = 17, 0.05
    Q = np.linalg.qr(rng.standard_normal((F, N, N)) + 1j * rng.standard_normal((F, N, N)))[0]
    U = np.empty((1, F, N, N, N), dtype=np.complex128)
    for n in range(N):
        lam = rng.random((F, N)) * (1 - gap)
        lam[:, n] = 1.0  # source n's largest eigenvalue belongs to column n of Q
        U[0, :, n] = (Q * lam[:, np.newaxis, :]) @ Q.conj().transpose(0, 2, 1)
    info = dv.zeros((1,), dv.i32)
    W = dv.to_device(np.tile(np.eye(N, dtype=np.complex128), (1, F, 1, 1)))
    got = dv.to_host(ops.faster_iva_step(W, dv.to_device(U), info))[0]
    assert int(info.item()) == 0
    want = Q.conj().transpose(0, 2, 1)  # row n = conj of column n
    assert fc.err_up_to_row_phase(got, want) <= 64 * N * EPS / gap


@pytest.mark.parametrize("N", [2, 3, 4, 5, 8, 9, 16])
def test_faster_step_with_nearly_parallel_eigenvectors(amd, N):
    """U_n = v_n v_n^H + 0.1 I with unit v_n that are the rows of a matrix whose Gram matrix is
    conditioned up to 1e6: the matrix of conjugate principal eigenvectors the step orthonormalises is
    conj(V) up to a phase per row, and the row phases commute with the polar factor."""
    dv, ops = amd["dv"], amd["ops"]
    rng = np.random.default_rng(90 + N)
    F = 17
    V = _conditioned_filters(rng, F, N, 1e6)[0]
    V = V / np.linalg.norm(V, axis=-1, keepdims=True)
    assert np.max(np.linalg.cond(V @ V.conj().transpose(0, 2, 1))) <= 1e7
    U = (V[..., :, np.newaxis] * V.conj()[..., np.newaxis, :] + 0.1 * np.eye(N))[np.newaxis]
    info = dv.zeros((1,), dv.i32)
    W = dv.to_device(np.tile(np.eye(N, dtype=np.complex128), (1, F, 1, 1)))
    got = dv.to_host(ops.faster_iva_step(W, dv.to_device(U), info))[0]
    assert int(info.item()) == 0
    assert np.max(np.abs(got @ got.conj().transpose(0, 2, 1) - np.eye(N))) <= 1e-12
    # eigenvector error eps / gap (gap 1 / 1.1) seen through the polar factor of a matrix with
    # cond(M) <= 3.2e3: within the operator bar
    assert fc.err_up_to_row_phase(got, fn.polar_unitary(V.conj())) <= OP_TOL


@pytest.mark.parametrize("N", [2, 3, 4, 5, 8, 9, 16])
def test_whiten_and_pca_outputs(amd, N):
    tr = amd["transform"]
    X = np.stack([fc.gen_mixture(700 + N + b, N, 17, 6 * N + 5) for b in range(2)])
    T = X.shape[-1]
    Z = tr.whiten(X)
    C = np.einsum("bmft,bnft->bfmn", Z, Z.conj()) / T
    assert np.max(np.abs(C - np.eye(N))) <= 1e-12
    assert fc.err(tr.whiten(X[0]), Z[0]) == 0.0
    for ascend in (True, False):
        Y = tr.pca(X, ascend=ascend)
        C = np.einsum("bmft,bnft->bfmn", Y, Y.conj()) / T
        d = np.real(np.diagonal(C, axis1=-2, axis2=-1))
        off = C - d[..., np.newaxis] * np.eye(N)
        assert np.max(np.abs(off)) <= 1e-12 * np.max(d)
        assert np.all(np.diff(d, axis=-1) <= 0 if ascend else np.diff(d, axis=-1) >= 0)
        lam = np.linalg.eigvalsh(np.einsum("bmft,bnft->bfmn", X, X.conj()) / T)
        np.testing.assert_allclose(np.sort(d, axis=-1), lam, rtol=1e-10)


def test_transform_fixture_and_errors(amd):
    tr, g = amd["transform"], load_golden(fc.TRANSFORM_FIXTURE)
    for key in ("c3", "c4", "r2", "r3"):
        x = g["x_" + key]
        for name, got in (("whiten_", tr.whiten(x)), ("pca_ascend_", tr.pca(x, ascend=True)),
                          ("pca_descend_", tr.pca(x, ascend=False))):
            assert got.shape == x.shape and np.iscomplexobj(got) == np.iscomplexobj(x)
            assert fc.err_up_to_row_phase(got, g[name + key]) <= OP_TOL, (name, key)
    rng = np.random.default_rng(0)
    for fnc in (tr.whiten, tr.pca):
        with pytest.raises(ValueError, match="Real tensor is expected"):
            fnc(rng.standard_normal((2, 9)) + 0j)
        with pytest.raises(ValueError, match="Complex tensor is expected"):
            fnc(rng.standard_normal((2, 2, 3, 9)))
        with pytest.raises(ValueError, match="The dimension of input is expected"):
            fnc(rng.standard_normal((9,)))


# ----------------------------------------------------------------------------------- contracts
@pytest.mark.parametrize("cls", ["FastIVA", "FasterIVA"])
def test_batch_equals_single_runs_and_runs_are_bit_identical(amd, cls):
    cfg = dict(fc.DEFAULTS, cls=cls, contrast="smooth")
    X = np.stack([fc.gen_mixture(930 + b, 3, 17, 40) for b in range(3)])
    m = build(amd, cfg)
    Y = m(X, n_iter=4)
    Y2 = build(amd, cfg)(X, n_iter=4)
    assert np.array_equal(Y, Y2)
    for b in range(3):
        s = build(amd, cfg)
        assert fc.err(s(X[b], n_iter=4), Y[b]) <= BATCH_TOL
        np.testing.assert_allclose(s.loss, [v[b] for v in m.loss], rtol=BATCH_TOL)


@pytest.mark.parametrize("cls", ["FastIVA", "FasterIVA"])
def test_update_once_by_hand_and_record_loss(amd, cls):
    cfg = dict(fc.DEFAULTS, cls=cls)
    X = fc.gen_mixture(940, 3, 7, 33)
    m = build(amd, cfg, scale_restoration=False)
    Y = m(X, n_iter=3)
    calls = []
    h = build(amd, cfg, scale_restoration=False, callbacks=lambda s: calls.append(len(s.loss)))
    h._bind_input(X)
    h._reset()
    for _ in range(3):
        h.update_once()
    assert np.array_equal(h.separate(np.asarray(h.whitened_input), h.demix_filter,
                                     use_whitening=False), Y)
    c = build(amd, cfg, scale_restoration=False, callbacks=lambda s: calls.append(len(s.loss)))
    c(X, n_iter=3)
    assert c.loss == m.loss and calls == [1, 2, 3, 4]
    q = build(amd, cfg, scale_restoration=False, record_loss=False)
    assert np.array_equal(q(X, n_iter=3), Y) and q.loss is None
    # initial_call=False: no entry for the initial state
    n = build(amd, cfg, scale_restoration=False)
    n(X, n_iter=3, initial_call=False)
    assert n.loss == m.loss[1:]


def test_host_floor_equals_kernel_floor(amd):
    X = fc.gen_mixture(950, 3, 7, 33)
    for cls in ("FastIVA", "FasterIVA"):
        cfg = dict(fc.DEFAULTS, cls=cls, contrast="smooth", flooring=("max", 5.0))
        dev = build(amd, cfg)(X, n_iter=4)
        host = build(amd, cfg, flooring_fn=lambda x: np.maximum(x, 5.0))(X, n_iter=4)
        assert fc.err(host, dev) <= OP_TOL


def test_separate_with_and_without_whitening(amd):
    X = fc.gen_mixture(960, 3, 7, 33)
    m = build(amd, dict(fc.DEFAULTS, cls="FastIVA"))
    W = fc.initial_filter(1, 3, 7)
    Z = amd["transform"].whiten(X)
    assert fc.err(m.separate(X, W), np.einsum("fnm,mft->nft", W, Z)) <= OP_TOL
    assert fc.err(m.separate(X, W, use_whitening=False), np.einsum("fnm,mft->nft", W, X)) <= OP_TOL


def test_signatures_reprs_and_errors(amd):
    iva = amd["iva"]
    with pytest.raises(ValueError, match="Specify contrast function."):
        iva.FastIVA()
    lap = fc.laplace_closures()
    with pytest.raises(ValueError, match="Specify derivative of contrast function."):
        iva.FasterIVA(contrast_fn=lap["contrast_fn"])
    with pytest.raises(ValueError, match="Specify second order derivative of contrast function."):
        iva.FastIVA(contrast_fn=lap["contrast_fn"], d_contrast_fn=lap["d_contrast_fn"])
    assert repr(iva.FastIVA(**lap)) == "FastIVA(scale_restoration=True, record_loss=True, reference_id=0)"
    assert repr(iva.FasterIVA(**fc.closures_for("FasterIVA", "laplace"), scale_restoration=False,
                              record_loss=False)) == \
        "FasterIVA(scale_restoration=False, record_loss=False)"
    def sig(obj):
        return re.sub(r" at 0x[0-9a-f]+", "", str(inspect.signature(obj)))

    nd = "numpy.ndarray"
    fl = ("flooring_fn: Optional[Callable[[{0}], {0}]] = functools.partial(<function max_flooring>, "
          "eps=1e-10), ").format(nd)
    tail = ("callbacks: Union[Callable[[ForwardRef('{1}')], NoneType], "
            "List[Callable[[ForwardRef('{1}')], NoneType]], NoneType] = None, "
            "scale_restoration: Union[bool, str] = True, record_loss: bool = True, "
            "reference_id: int = 0) -> None")
    cf = "{2}_fn: Callable[[{0}], {0}] = None, "
    assert sig(amd["transform"].whiten) == "(input: {0}) -> {0}".format(nd)
    assert sig(amd["transform"].pca) == "(input: {0}, ascend: bool = True) -> {0}".format(nd)
    assert sig(iva.FastIVABase.__init__) == ("(self, " + fl + tail).format(nd, "IVABase")
    assert sig(iva.FastIVA.__init__) == (
        "(self, " + cf.format(nd, 0, "contrast") + cf.format(nd, 0, "d_contrast")
        + cf.format(nd, 0, "dd_contrast") + fl + tail).format(nd, "FastIVA")
    assert sig(iva.FasterIVA.__init__) == (
        "(self, " + cf.format(nd, 0, "contrast") + cf.format(nd, 0, "d_contrast")
        + fl + tail).format(nd, "FasterIVA")
    for cls in (iva.FastIVABase, iva.FastIVA, iva.FasterIVA):
        assert sig(cls.separate) == ("(self, input: {0}, demix_filter: {0}, "
                                     "use_whitening: bool = True) -> {0}").format(nd)
        assert sig(cls.__call__) == ("(self, input: {0}, n_iter: int = 100, "
                                     "initial_call: bool = True, **kwargs) -> {0}").format(nd)
    for cls in (iva.FastIVA, iva.FasterIVA):
        assert sig(cls.update_once) == ("(self, flooring_fn: Union[str, Callable[[{0}], {0}], "
                                        "NoneType] = 'self') -> None").format(nd)
    rng = np.random.default_rng(1)
    for N in (1, 17):
        X = rng.standard_normal((N, 3, 40)) + 1j * rng.standard_normal((N, 3, 40))
        with pytest.raises(NotImplementedError, match="FastIVA takes 2 to 16 sources"):
            iva.FastIVA(**lap)(X, n_iter=1)
        with pytest.raises(NotImplementedError, match="FasterIVA takes 2 to 16 sources"):
            iva.FasterIVA(**fc.closures_for("FasterIVA", "laplace"))(X, n_iter=1)
        for fnc in (amd["transform"].whiten, amd["transform"].pca):
            with pytest.raises(NotImplementedError, match="2 to 16 channels"):
                fnc(X)


@pytest.mark.parametrize("cls", ["FastIVA", "FasterIVA"])
def test_singular_injected_filter_raises(amd, cls):
    X = fc.gen_mixture(970, 3, 7, 33)
    # two sources with the same filter in every bin: the same norms, weights and statistics, so the
    # rows stay equal through both updates (equal rows in ONE bin do not: the weights differ)
    W0 = np.tile(np.eye(3, dtype=np.complex128), (7, 1, 1))
    W0[:, 1] = W0[:, 0]
    with pytest.raises(np.linalg.LinAlgError):
        build(amd, dict(fc.DEFAULTS, cls=cls))(X, n_iter=2, demix_filter=W0)


def test_loss_falls_over_100_iterations(amd):
    """A smoke test, not a parity test: one mixture of the size of configs[1] (N=4, F=1025, T=512)."""
    X = fc.gen_mixture(980, 4, 1025, 512)
    m = build(amd, dict(fc.DEFAULTS, cls="FastIVA"))
    m(X, n_iter=100)
    assert len(m.loss) == 101 and m.loss[-1] < m.loss[0] and np.all(np.isfinite(m.loss))
