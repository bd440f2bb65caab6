"""GPU tests of the time-domain ICA classes (ssspy_amd/bss/ica.py, csrc/ica.hip).

Bars: 1e-8 relative Frobenius on filters, snapshots and outputs, rtol 1e-9 on loss
lists, against the golden vectors of the reference and against the NumPy restatement
(tests/ica_numpy.py, itself pinned to the goldens to 1e-10).  The statistics pass is compared entry
by entry with np.longdouble sums under the derived bound of DESIGN.md ("ICA": (T + 2 N + c) eps
sum |terms|, c = 32).  Every case prints what it measured.
"""

import numpy as np
import pytest
import torch

import ica_numpy as inp
from conftest import load_golden, rel_err
from ica_cases import (CASES, Snapshots, check_against_golden, gen_sources, golden_init,
                       golden_kwargs)
from ssspy_amd import _device as dv
from ssspy_amd import _lib, _ops, _routes
from ssspy_amd.bss import ica

pytestmark = pytest.mark.gpu

TOL, LOSS_RTOL = 1e-8, 1e-9
EPS = np.finfo(np.float64).eps
C_BOUND = 32
TILE = 256  # samples one workgroup takes per round
CHUNK = 2048  # == _ops.ica_chunk_samples(N, T), asserted below
T_EDGES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 57]
KINDS = {"laplace": _lib.ICA_LAPLACE, "logistic": _lib.ICA_LOGISTIC, "logcosh": _lib.ICA_LOGCOSH}


def test_chunk_is_a_constant_of_the_shape():
    for N, T in ((2, 1), (16, 10 ** 6), (4, 160000)):
        assert _ops.ica_chunk_samples(N, T) == CHUNK


# ---- golden replay --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_golden_replay(name):
    g = load_golden(name)
    n_iter = int(g["meta_n_iter"])
    snap = Snapshots(n_iter)
    cls = getattr(ica, str(g["meta_cls"]))
    m = cls(callbacks=snap, **golden_kwargs(g, named=ica))
    want = ica.COMPATIBILITY if str(g["meta_nonlinearity"]) == "closure" else ica.DEVICE
    assert ica.route(m)[0] == want
    init = golden_init(g)
    Y = m(g["X"], n_iter=n_iter, **init)
    check_against_golden(g, m, Y, snap, TOL, LOSS_RTOL, report=name)
    N, T = g["X"].shape
    assert (m.n_sources, m.n_channels, m.n_samples) == (N, N, T)
    assert np.array_equal(m.input, g["X"]) and m.output.shape == (N, T)
    if "whitened_input" in g:
        err = rel_err(m.whitened_input, g["whitened_input"])
        print("{}: whitened_input {:.1e}".format(name, err))
        assert err < 1e-10
    if init:  # copied, not aliased
        assert np.array_equal(init["demix_filter"], g["demix_filter0"])
        assert m.demix_filter is not init["demix_filter"]

    # without callbacks the iterations are enqueued in one go: the same numbers
    m2 = cls(**golden_kwargs(g, named=ica))
    Y2 = m2(g["X"], n_iter=n_iter, **golden_init(g))
    assert rel_err(Y2, g["final_output"]) < TOL
    np.testing.assert_allclose(m2.loss, g["loss"], rtol=LOSS_RTOL)


# ---- the named classes and triples against the restatement ------------------------------------------
def _methods(mod, named):
    g1, s1, d1 = named["logistic"]
    g2, s2, d2 = named["logcosh"]
    return {
        "GradLaplaceICA": lambda: mod.GradLaplaceICA(step_size=0.05),
        "NaturalGradLaplaceICA": lambda: mod.NaturalGradLaplaceICA(is_holonomic=True),
        "GradICA-logcosh": lambda: mod.GradICA(contrast_fn=g2, score_fn=s2, is_holonomic=True),
        "NaturalGradICA-logistic": lambda: mod.NaturalGradICA(contrast_fn=g1, score_fn=s1),
        "FastICA-logistic": lambda: mod.FastICA(contrast_fn=g1, score_fn=s1, d_score_fn=d1),
        "FastICA-logcosh": lambda: mod.FastICA(contrast_fn=g2, score_fn=s2, d_score_fn=d2),
    }


# every T with two N; N covers 2, 3, 4, 5, 8, 9, 16
SHAPES = [(1, 2), (1, 9), (63, 3), (63, 16), (64, 4), (64, 8), (65, 5), (65, 9),
          (TILE - 1, 2), (TILE - 1, 8), (TILE, 3), (TILE, 16), (TILE + 1, 4), (TILE + 1, 9),
          (CHUNK - 1, 5), (CHUNK - 1, 16), (CHUNK, 2), (CHUNK, 9), (CHUNK + 1, 8), (CHUNK + 1, 3),
          (3 * CHUNK + 57, 4), (3 * CHUNK + 57, 16)]


def conditioned_sources(seed, N, T, limit=1e4):
    """gen_sources with the first seed (seed, seed + 7919, ...) whose covariance has a condition
    number below ``limit``.  A random mixing matrix is now and then close to singular (1.1e7 at
    N = 16 for one of the seeds below), and FastICA on such an input does not hold still: the
    restatement itself moves by 1e-8 in three iterations when the input is perturbed by 1e-15,
    where the generator of the golden vectors demands 1e-10.  Below 1e4 it moves by 4e-10 at most."""
    while T >= 4 * N:
        X = gen_sources(seed, N, T)
        if np.linalg.cond(X @ X.T) < limit:
            return X
        seed += 7919
    return gen_sources(seed, N, T)


@pytest.mark.parametrize("T,N", SHAPES)
def test_named_classes_match_restatement(T, N):
    X = conditioned_sources(1000 + 17 * N + T, N, T)
    dev, ref = _methods(ica, ica.NAMED), _methods(inp, ica.NAMED)
    for name in dev:
        if name.startswith("FastICA") and T < 4 * N:
            continue  # (whitening needs a covariance of full rank, well away from singular)
        md, mr = dev[name](), ref[name]()
        assert ica.route(md)[0] == ica.DEVICE
        Yd, Yr = md(X, n_iter=3), mr(X, n_iter=3)
        errs = (rel_err(md.demix_filter, mr.demix_filter), rel_err(Yd, Yr),
                float(np.max(np.abs(np.array(md.loss) / np.array(mr.loss) - 1))))
        print("T={} N={} {}: filter {:.1e} output {:.1e} loss {:.1e}".format(T, N, name, *errs))
        assert errs[0] < TOL and errs[1] < TOL
        np.testing.assert_allclose(md.loss, mr.loss, rtol=LOSS_RTOL)


# ---- the statistics pass, entry by entry ----------------------------------------------------------------
def _terms_longdouble(kind, y):
    one = np.longdouble(1)
    if kind == "laplace":
        return np.abs(y), np.sign(y), np.zeros_like(y)
    if kind == "logistic":
        e = np.exp(-np.abs(y))
        s = np.where(y >= 0, one / (one + e), e / (one + e))
        return np.maximum(y, 0) + np.log1p(e), s, s * (one - s)
    th = np.tanh(y)
    return np.abs(y) + np.log1p(np.exp(-2 * np.abs(y))) - np.log(np.longdouble(2)), th, one - th * th


def _contrast_scale(kind, y, G):
    """sum |terms| of one contrast value: log-cosh is the sum |y| + log1p(.) - log 2 of terms up to
    log 2 each, whatever the size of the result."""
    return np.abs(y) + 2 * np.log(2.0) if kind == "logcosh" else np.abs(G)


@pytest.mark.parametrize("N", [2, 4, 8, 9, 16])
def test_stats_pass_elementwise(N):
    worst = 0.0
    for T in T_EDGES:
        rng = np.random.default_rng(40 * N + T)
        X = gen_sources(2000 + N + T, N, T)
        if T > 40:
            X[:, 20:31] = 0.0  # exact zeros: sign(0) = 0
        W = np.eye(N) + 0.3 * rng.standard_normal((N, N))
        Xl, Wl = X.astype(np.longdouble), W.astype(np.longdouble)
        Yl = Wl @ Xl
        A = np.abs(Wl) @ np.abs(Xl)  # |y| <= a, and the rounding of y is N eps a
        nonzero = np.abs(Yl)[A > 0]
        assert nonzero.size == 0 or np.min(nonzero / A[A > 0]) > 1e-9  # no sign can flip
        Xd, Wd = dv.to_device(X[None]), dv.to_device(W[None])
        ws = _ops.ica_workspace(1, N, T, Xd.device)
        means = dv.empty((1, N * N + 2 * N), dv.f64, Xd.device)
        for kind in KINDS:
            G, Phi, dPhi = _terms_longdouble(kind, Yl)
            for right, R, Ra in ((_lib.ICA_RIGHT_Y, Yl, A), (_lib.ICA_RIGHT_X, Xl, np.abs(Xl))):
                _ops.ica_stats(Xd, Wd, ws, KINDS[kind], right)
                _ops.ica_step(ws, Wd, T, _lib.ICA_FOLD_ONLY, means=means)
                got = dv.to_host(means)[0].astype(np.longdouble) * T
                factor = (T + 2 * N + C_BOUND) * EPS
                exact = np.concatenate([(Phi @ R.T).ravel(), G.sum(axis=1), dPhi.sum(axis=1)])
                scale = np.concatenate([((np.abs(Phi) + A) @ Ra.T).ravel(),
                                        (_contrast_scale(kind, Yl, G) + A).sum(axis=1),
                                        (np.abs(dPhi) + A).sum(axis=1)])
                ratio = np.abs(got - exact) / (factor * scale)
                worst = max(worst, float(ratio.max()))
                assert (ratio <= 1).all(), (T, kind, right, float(ratio.max()))
        _ops.check_workspace_canaries()
    print("N={}: worst error / bound {:.2e}".format(N, worst))


def test_stats_pass_given_phi_and_batch_records():
    """The closures' form (phi and phi' read from memory) and one record per (mixture, chunk)."""
    B, N, T = 3, 5, 2 * CHUNK + 9
    rng = np.random.default_rng(5)
    X, W = rng.standard_normal((B, N, T)), rng.standard_normal((B, N, N))
    Phi, dPhi = rng.standard_normal((B, N, T)), rng.standard_normal((B, N, T))
    Xd, Wd = dv.to_device(X), dv.to_device(W)
    ws = _ops.ica_workspace(B, N, T, Xd.device)
    assert ws[1] == B * 3 * (N * N + 2 * N) * 8
    means = dv.empty((B, N * N + 2 * N), dv.f64, Xd.device)
    _ops.ica_stats(Xd, Wd, ws, _lib.ICA_GIVEN, _lib.ICA_RIGHT_Y, phi=dv.to_device(Phi),
                   dphi=dv.to_device(dPhi))
    _ops.ica_step(ws, Wd, T, _lib.ICA_FOLD_ONLY, means=means)
    got = dv.to_host(means)
    Y = W @ X
    for b in range(B):
        assert rel_err(got[b, :N * N].reshape(N, N), Phi[b] @ Y[b].T / T) < 1e-12
        assert not got[b, N * N:N * N + N].any()
        assert rel_err(got[b, N * N + N:], dPhi[b].mean(axis=1)) < 1e-12
    records = dv.to_host(ws[0])[:B * 3 * (N * N + 2 * N)].reshape(B, 3, -1)
    for c, (a, z) in enumerate(((0, CHUNK), (CHUNK, 2 * CHUNK), (2 * CHUNK, T))):
        want = np.einsum("bnt,bmt->bnm", Phi[:, :, a:z], Y[:, :, a:z]).reshape(B, -1)
        assert rel_err(records[:, c, :N * N], want) < 1e-12
    _ops.check_workspace_canaries()


def test_stats_pass_past_2_31_elements():
    """int64 indexing: the last samples of a (16, 2^27 + 3) mixture lie past element 2^31."""
    N, T = 16, 2 ** 27 + 3
    dev = dv.device()
    X = torch.zeros((1, N, T), dtype=torch.float64, device=dev)
    tail = np.random.default_rng(9).standard_normal((N, 40))
    X[0, :, T - 40:] = dv.to_device(tail)
    W = torch.eye(N, dtype=torch.float64, device=dev)[None].contiguous()
    ws = _ops.ica_workspace(1, N, T, dev)
    means = dv.empty((1, N * N + 2 * N), dv.f64, dev)
    _ops.ica_stats(X, W, ws, _lib.ICA_IDENTITY, _lib.ICA_RIGHT_X)
    _ops.ica_step(ws, W, T, _lib.ICA_FOLD_ONLY, means=means)
    got = dv.to_host(means)[0, :N * N].reshape(N, N) * T
    assert rel_err(got, tail @ tail.T) < 1e-12
    del X
    _ops.check_workspace_canaries()


# ---- the step kernel ------------------------------------------------------------------------------------
def _step_numpy(S, W, algorithm, holonomic, eta):
    N = len(W)
    M, dphi = S[:N * N].reshape(N, N), S[N * N + N:]
    if algorithm == _lib.ICA_FAST:
        out = np.zeros_like(W)
        for n in range(N):
            w = dphi[n] * W[n] - M[n]
            w = w - out[:n].T @ (out[:n] @ w)
            out[n] = w / np.sqrt(w @ w)
        return out
    D = M - np.eye(N) if holonomic else M - np.diag(np.diag(M))
    delta = D @ W if algorithm == _lib.ICA_NATURAL_GRAD else D @ np.linalg.inv(W).T
    return W - eta * delta


@pytest.mark.parametrize("N", [2, 4, 8, 16])
def test_step_kernel_matches_numpy(N):
    B, T = 3, 2 * CHUNK + 100  # three records per mixture
    rec = N * N + 2 * N
    rng = np.random.default_rng(70 + N)
    records = rng.standard_normal((B, 3, rec)) * T / 3
    W0 = np.eye(N) + 0.3 * rng.standard_normal((B, N, N))
    W0[1, 0, 0] = 0.0  # a zero leading entry: the factorisation has to pivot
    assert max(np.linalg.cond(W) for W in W0) < 1e3
    S = ((records[:, 0] + records[:, 1]) + records[:, 2]) / T  # chunk order
    dev = dv.device()
    ws = _ops.ica_workspace(B, N, T, dev)
    ws[0][:B * 3 * rec].copy_(dv.to_device(records.ravel()))
    info = dv.zeros((1,), dv.i32, dev)
    for algorithm in (_lib.ICA_GRAD, _lib.ICA_NATURAL_GRAD, _lib.ICA_FAST):
        for holonomic in (False, True):
            Wd = dv.to_device(W0)
            terms = dv.zeros((2, B), dv.f64, dev)
            means = dv.empty((B, rec), dv.f64, dev)
            _ops.ica_step(ws, Wd, T, algorithm, holonomic, 0.1, terms[0], terms[1], means, info)
            got, t, mh = dv.to_host(Wd), dv.to_host(terms), dv.to_host(means)
            assert int(info.item()) == 0
            assert rel_err(mh, S) < 1e-14
            np.testing.assert_allclose(t[0], S[:, N * N:N * N + N].sum(axis=1), rtol=1e-13)
            np.testing.assert_allclose(t[1], np.linalg.slogdet(W0)[1], rtol=1e-11, atol=1e-13)
            # eps N cond(W) < 4e-12 for the solve of GradICA
            errs = [rel_err(got[b], _step_numpy(S[b], W0[b], algorithm, holonomic, 0.1))
                    for b in range(B)]
            print("N={} algorithm={} holonomic={}: {:.1e}".format(N, algorithm, holonomic, max(errs)))
            assert max(errs) < 1e-11
            if algorithm == _lib.ICA_FAST:
                assert np.abs(got @ got.transpose(0, 2, 1) - np.eye(N)).max() < 1e-12
    _ops.check_workspace_canaries()


@pytest.mark.parametrize("N", [2, 4, 8, 16])
def test_singular_filter_raises_linalg_error(N):
    X = gen_sources(90 + N, N, 300)
    W0 = np.eye(N) + 0.1 * np.random.default_rng(N).standard_normal((N, N))
    W0[:, N - 1] = 0.0  # a zero column: an exactly zero pivot
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.inv(W0)
    m = ica.GradLaplaceICA()
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        m(X, n_iter=2, demix_filter=W0)
    # the step leaves the filters alone and flags the mixture: nothing infinite comes back
    Xd, Wd = dv.to_device(X[None]), dv.to_device(W0[None])
    ws = _ops.ica_workspace(1, N, 300, Xd.device)
    info = dv.zeros((1,), dv.i32, Xd.device)
    _ops.ica_stats(Xd, Wd, ws, _lib.ICA_LAPLACE, _lib.ICA_RIGHT_Y)
    _ops.ica_step(ws, Wd, 300, _lib.ICA_GRAD, False, 0.1, info=info)
    assert int(info.item()) == 1 and np.array_equal(dv.to_host(Wd)[0], W0)
    # the natural gradient needs no inverse: it runs, with a loss of +inf (log|det W| = -inf)
    mn = ica.NaturalGradLaplaceICA()
    mn(X, n_iter=1, demix_filter=W0)
    assert mn.loss[0] == np.inf and np.isfinite(mn.demix_filter).all()


# ---- properties of the classes ------------------------------------------------------------------------------
def _three_classes():
    g, s, d = ica.NAMED["logcosh"]
    return [lambda **kw: ica.GradLaplaceICA(step_size=0.05, **kw),
            lambda **kw: ica.NaturalGradICA(contrast_fn=g, score_fn=s, is_holonomic=True, **kw),
            lambda **kw: ica.FastICA(contrast_fn=g, score_fn=s, d_score_fn=d, **kw)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_batch_equals_single_runs_and_runs_are_bit_identical(which):
    make = _three_classes()[which]
    N, T = 4, CHUNK + 300
    X = np.stack([gen_sources(300 + b, N, T) for b in range(3)])
    mb = make()
    Yb = mb(X, n_iter=4)
    loss = np.array(mb.loss)
    assert Yb.shape == (3, N, T) and mb.demix_filter.shape == (3, N, N) and loss.shape == (5, 3)
    for b in range(3):
        ms = make()
        Ys = ms(X[b], n_iter=4)
        errs = (rel_err(Yb[b], Ys), rel_err(mb.demix_filter[b], ms.demix_filter))
        print("class {} mixture {}: output {:.1e} filter {:.1e}".format(which, b, *errs))
        assert max(errs) < 1e-10
        np.testing.assert_allclose(loss[:, b], ms.loss, rtol=1e-10)
    again = make()
    Ya = again(X, n_iter=4)
    assert np.array_equal(Ya, Yb) and np.array_equal(again.demix_filter, mb.demix_filter)
    assert np.array_equal(np.array(again.loss), loss)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_update_once_by_hand_equals_call(which):
    make = _three_classes()[which]
    X = gen_sources(400 + which, 3, 700)
    m = make()
    Y = m(X, n_iter=3)
    h = make()
    h(X, n_iter=0)
    assert len(h.loss) == 1
    for _ in range(3):
        h.update_once()
        h.loss.append(h.compute_loss())
    assert np.array_equal(h.demix_filter, m.demix_filter) and np.array_equal(h.output, Y)
    np.testing.assert_allclose(h.loss, m.loss, rtol=1e-14)
    # initial_call=False drops the first entry; record_loss=False keeps none; a device tensor is taken
    q = make()
    Yq = q(dv.to_device(X), n_iter=3, initial_call=False)
    assert np.array_equal(Yq, Y) and q.loss == m.loss[1:]
    r = make(record_loss=False)
    assert np.array_equal(r(X, n_iter=3), Y) and r.loss is None
    # a second call goes on from the filters of the first
    c = make()
    c(X, n_iter=1)
    c(X, n_iter=2)
    assert rel_err(c.demix_filter, m.demix_filter) < 1e-12


@pytest.mark.parametrize("which", [0, 1, 2])
def test_compatibility_route_matches_device_route(which):
    make = _three_classes()[which]
    X = gen_sources(500 + which, 4, CHUNK + 11)
    md = make()
    Yd = md(X, n_iter=4)
    mc = make()
    for name in ("contrast_fn", "score_fn", "d_score_fn"):
        fn = getattr(mc, name, None)
        if fn is not None:
            setattr(mc, name, lambda y, fn=fn: fn(y))
    assert ica.route(md)[0] == ica.DEVICE and ica.route(mc)[0] == ica.COMPATIBILITY
    Yc = mc(X, n_iter=4)
    errs = (rel_err(Yc, Yd), rel_err(mc.demix_filter, md.demix_filter))
    print("class {}: output {:.1e} filter {:.1e}".format(which, *errs))
    assert max(errs) < 1e-10
    np.testing.assert_allclose(mc.loss, md.loss, rtol=1e-10)
    # the route entry sends the named functions the same way
    with _routes.override(ica_named=False):
        mf = make()
        assert rel_err(mf(X, n_iter=4), Yd) < 1e-10


def test_fastica_whitening_and_orthogonality():
    N, T = 8, 3000
    X = gen_sources(600, N, T)
    seen = []
    m = ica.FastICA(*ica.NAMED["logistic"], callbacks=lambda s: seen.append(s.demix_filter.copy()))
    m(X, n_iter=5)
    err = rel_err(m.whitened_input, inp.whiten(X))
    print("whitened_input {:.1e}".format(err))
    assert err < 1e-10
    # (eps N cond(C) with cond(C) < 1e4)
    assert np.abs(m.whitened_input @ m.whitened_input.T / T - np.eye(N)).max() < 1e-10
    assert len(seen) == 6
    for k, W in enumerate(seen[1:]):
        dev = np.abs(W @ W.T - np.eye(N)).max()
        print("iteration {}: |W W^T - I| {:.1e}".format(k + 1, dev))
        assert dev < 1e-12
    # separate(): with and without whitening
    assert rel_err(m.separate(X, m.demix_filter), m.output) < 1e-12
    assert rel_err(m.separate(m.whitened_input, m.demix_filter, use_whitening=False), m.output) < 1e-12
    g = ica.GradLaplaceICA()
    g(X, n_iter=1)
    assert rel_err(g.separate(X, g.demix_filter), g.demix_filter @ X) < 1e-13
    assert np.isclose(g.compute_logdet(g.demix_filter), np.linalg.slogdet(g.demix_filter)[1])


@pytest.mark.parametrize("n_sources", [1, 17])
def test_limits(n_sources):
    with pytest.raises(NotImplementedError, match="2 to 16 sources"):
        ica.NaturalGradLaplaceICA()(np.zeros((n_sources, 50)), n_iter=1)
    with pytest.raises(NotImplementedError, match="2 to 16 sources"):
        ica.FastICA(*ica.NAMED["logcosh"])(np.zeros((n_sources, 50)), n_iter=1)
    dev = dv.device()
    X = dv.zeros((1, n_sources, 50), dv.f64, dev)
    W = dv.zeros((1, n_sources, n_sources), dv.f64, dev)
    with pytest.raises(NotImplementedError, match="2 to 16 sources"):
        _ops.ica_separate(X, W)
    with pytest.raises(ValueError):
        _ops.ica_workspace(1, n_sources, 50, dev)
