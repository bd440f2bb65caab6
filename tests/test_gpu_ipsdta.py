"""GaussIPSDTA / TIPSDTA and their kernels on the device.

Whole runs replay every reference fixture through the public classes (outputs and filters at 1e-8
relative Frobenius, losses within 1e-9 of the largest |loss| of the run, snapshots after iterations
1 and 2 through a callback); each kernel is checked on its own, elementwise, against
``numpy.longdouble`` (tests/ipsdta_numpy.py with the 80-bit types).

Error bars of the elementwise tests, u = 2^-53.  A Cholesky inverse of an L x L matrix of condition
kappa is off by at most ~ 4 L^2 kappa u relative to |R^-1| (Higham, Accuracy and Stability, thm 10.4
with the inverse's two triangular products); forming R from K terms adds K u before that, amplified
by kappa as well, and a mean over T frames adds T u.  Quantities quadratic in R^-1 (Q, the numerator)
take twice the bar.  So:  bar = 2 (4 L^2 + K) kappa u + (T + N L + 8) u, relative to the largest
|reference| entry of the array compared, with kappa = max cond(R) measured in longdouble.  Inputs
are drawn with kappa <= 1e4.

The three outputs that end in a contraction -- y^H u, u^H T u and tr(R^-1 T) -- also carry that
contraction's own rounding, which no fp64 evaluation avoids: n terms summed in any order are off by
at most (n + 2) u sum|terms| (Higham, section 3.1), per element, with the terms measured in
longdouble (n = 2 L, 4 L^2 + 4 and 2 L^2 real products).  On the well-conditioned draws sum|terms| is
the result itself and the addition is a few u; on the rank-deficient basis of the floored-route test
(T along the one large eigenvector of R, u dominated by the floored directions) the terms of
u^H T u are 1e7 x 1e-6 x 1e7 and cancel to ~1, and this term is the whole error: measured there
4.6e-10 of the largest numerator, against 2.9e-10 from the kappa term alone, which the first form of
this derivation had as the only term.
"""

import numpy as np
import pytest

import ipsdta_cases as ic
import ipsdta_numpy as rn
from conftest import load_golden

pytestmark = pytest.mark.gpu

OUT_TOL, LOSS_TOL = 1e-8, 1e-9
U = 2.0 ** -53
LD, CLD = np.longdouble, np.clongdouble


@pytest.fixture(scope="module")
def amd():
    import ssspy_amd.bss.ipsdta as ipsdta
    from ssspy_amd import _device as dv, _lib, _ops
    from ssspy_amd.bss import _update_spatial_model as usm
    from ssspy_amd.special import flooring
    return dict(ipsdta=ipsdta, dv=dv, lib=_lib, ops=_ops, flooring=flooring, usm=usm)


def build(amd, cfg, **over):
    kw = dict(n_basis=cfg["n_basis"], n_blocks=cfg["n_blocks"],
              flooring_fn=ic.flooring_for(cfg["flooring"], amd["flooring"]),
              source_normalization=cfg["source_normalization"],
              scale_restoration=cfg["scale_restoration"], reference_id=cfg["reference_id"],
              rng=np.random.default_rng(cfg["seed"] + 1))
    if cfg["cls"] == "TIPSDTA":
        kw["dof"] = cfg["dof"]
    kw.update(over)
    return getattr(amd["ipsdta"], cfg["cls"])(**kw)


def restated(cfg, rng=None):
    floor, threshold = ic.numpy_floor(cfg["flooring"])
    return rn.IPSDTA(cfg["n_basis"], cfg["n_blocks"], dof=cfg["dof"], floor=floor, threshold=threshold,
                     source_normalization=cfg["source_normalization"],
                     scale_restoration=cfg["scale_restoration"], reference_id=cfg["reference_id"],
                     rng=rng or np.random.default_rng(cfg["seed"] + 1))


def loss_close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return np.max(np.abs(got - want)) <= LOSS_TOL * np.max(np.abs(want))


# ------------------------------------------------------------------------------ whole runs
@pytest.mark.parametrize("name", sorted(ic.CASES))
def test_fixture_through_public_class(amd, name):
    g, cfg = load_golden(name), ic.CASES[name]
    n_iter = int(g["meta_n_iter"])
    first = {}

    class Snap(ic.Snapshots):
        def __call__(self, method):
            if self.calls == 0:
                first["basis"], first["activation"] = method.basis, np.array(method.activation)
                first["n_remains"] = method.n_remains
            super().__call__(method)

    snap = Snap()
    m = build(amd, cfg, callbacks=snap)
    Y = m(g["X"], n_iter=n_iter, **(ic.initial_state(cfg) if cfg["inject"] else {}))
    # the seeded draw (and the normalisation at reset) give the reference's initial parameters
    assert first["n_remains"] == cfg["shape"][1] % cfg["n_blocks"]
    assert (type(first["basis"]) is tuple) == (first["n_remains"] > 0)
    for got, key in zip(rn.as_parts(first["basis"]), ("basis0_low", "basis0_high")):
        assert got.shape == g[key].shape and ic.err(got, g[key]) <= 1e-13
    assert ic.err(first["activation"], g["activation0"]) <= 1e-13
    assert len(m.loss) == n_iter + 1 and loss_close(m.loss, g["loss"])
    for it in (1, 2):
        for what in ("output", "demix_filter"):
            key = "{}_it{}".format(what, it)
            assert ic.err(snap.store[key], g[key]) <= OUT_TOL, key
    assert ic.err(Y, g["final_output"]) <= OUT_TOL
    assert ic.err(m.demix_filter, g["final_demix_filter"]) <= OUT_TOL
    assert m.demix_filter.shape == g["final_demix_filter"].shape
    assert m.activation.shape == g["activation0"].shape and ic.err(m.output, Y) == 0


@pytest.mark.parametrize("cls,dof", [("GaussIPSDTA", None), ("TIPSDTA", 3)])
@pytest.mark.parametrize("shape,n_blocks,K", [((2, 5, 17), 2, 2), ((3, 9, 33), 3, 3),
                                              ((4, 17, 70), 4, 4)])
def test_fresh_input_against_restatement(amd, cls, dof, shape, n_blocks, K):
    cfg = ic._case(cls, shape, n_blocks, K, 700 + shape[0], dof=dof)
    X = ic.gen_mixture(cfg["seed"], *shape)
    ref = restated(cfg)
    Yr = ref.run(X, 3)
    m = build(amd, cfg)
    Y = m(X, n_iter=3)
    assert ic.err(Y, Yr) <= OUT_TOL and ic.err(m.demix_filter, ref.W) <= OUT_TOL
    assert loss_close(m.loss, ref.loss)


@pytest.mark.parametrize("name", ["ipsdta_gauss_f9_b4_rem1", "ipsdta_t3_inject"])
def test_batched_call_equals_per_mixture_calls(amd, name):
    cfg = ic.CASES[name]
    N, F, T = cfg["shape"]
    Xs = np.stack([ic.gen_mixture(cfg["seed"] + 10 * b, N, F, T) for b in range(3)])
    state = ic.initial_state(cfg)
    batched_state = {k: (tuple(np.stack([t] * 3) for t in v) if isinstance(v, tuple)
                         else np.stack([v] * 3)) for k, v in state.items()}
    mb = build(amd, cfg)
    Yb = mb(Xs, n_iter=2, **batched_state)
    assert Yb.shape == Xs.shape and np.asarray(mb.loss).shape == (3, 3)
    for b in range(3):
        m = build(amd, cfg)
        Y = m(Xs[b], n_iter=2, **state)
        assert np.array_equal(Y, Yb[b]) and np.array_equal(m.demix_filter, mb.demix_filter[b])
        assert np.array_equal(np.asarray(m.loss), np.asarray(mb.loss)[:, b])


@pytest.mark.parametrize("name", ["ipsdta_gauss_f31_b4_rem3", "ipsdta_t3_k1_ref1"])
def test_two_runs_are_bit_equal(amd, name):
    g, cfg = load_golden(name), ic.CASES[name]
    runs = []
    for _ in range(2):
        m = build(amd, cfg)
        Y = m(g["X"], n_iter=3)
        runs.append((Y, np.array(m.demix_filter), np.array(m.loss), np.array(m.activation)))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_limits_raise(amd):
    G = amd["ipsdta"].GaussIPSDTA
    with pytest.raises(NotImplementedError, match="2 to 8 sources, got 9"):
        G(2, 2)(ic.gen_mixture(1, 9, 4, 8), n_iter=1)
    with pytest.raises(NotImplementedError, match="block sizes up to 8, got 9"):
        G(2, 1)(ic.gen_mixture(1, 2, 9, 8), n_iter=1)
    with pytest.raises(NotImplementedError, match="n_basis 1 to 32, got 33"):
        G(33, 2)(ic.gen_mixture(1, 2, 4, 8), n_iter=1)
    with pytest.raises(NotImplementedError, match="fixed-point iteration is not supported"):
        G(2, 2, spatial_algorithm="FPI")(ic.gen_mixture(1, 2, 4, 8), n_iter=1)


# ------------------------------------------------------------------------------ kernels, elementwise
SHAPES = [  # (B, N, F, T, n_blocks, K)
    (1, 2, 3, 1, 3, 1),      # L = 1, n_blocks = F, one frame
    (3, 3, 4, 63, 2, 2),     # L = 2
    (1, 4, 7, 64, 2, 16),    # L = 3 with a high block of 4
    (1, 2, 11, 65, 2, 2),    # L = 5 with a high block of 6
    (1, 3, 8, 130, 1, 32),   # n_blocks = 1, L = 8, three chunks of frames
    (3, 8, 15, 65, 2, 2),    # 8 sources, L = 7 with a high block of 8
    (1, 4, 5, 130, 5, 2),    # L = 1, n_blocks = F
]


def draw_problem(seed, B, N, F, T, n_blocks, K, zeros=True):
    """Mixtures, filters, Hermitian positive definite bases and activations (some exactly zero) with
    cond(R) <= 1e4: every basis matrix is G G^H / L + 0.3 I."""
    rng = np.random.default_rng(seed)

    def cplx(*s):
        return rng.standard_normal(s) + 1j * rng.standard_normal(s)

    X = cplx(B, N, F, T)
    W = np.eye(N) + 0.3 * cplx(B, F, N, N)
    parts = rn.split_sizes(F, n_blocks)
    basis = []
    for _, _, C, L in parts:
        G = cplx(B, N, K, C, L, L)
        basis.append(G @ np.conj(np.swapaxes(G, -2, -1)) / L + 0.3 * np.eye(L))
    V = 0.2 + rng.random((B, N, K, T))
    if zeros and K > 1:
        V[..., 0, ::3] = 0.0
    pi = 0.5 + rng.random((B, N, T))
    return X, W, basis, V, pi, parts


def exact_frame(X, W, basis, V, parts):
    """Per partition (y, R^-1, u, log det R) in longdouble for one mixture, and max cond(R), also
    measured in longdouble (power iterations on R and R^-1; log det from Cholesky pivots)."""
    out, kappa = [], 1.0
    for T, part in zip(basis, parts):
        y, R, Rinv, u = rn.frame_quantities(X.astype(CLD), W.astype(CLD), T.astype(CLD),
                                            V.astype(LD), part, floored=False)
        kappa = max(kappa, float(np.max(rn.cond2_hpd(R, Rinv))))
        out.append((y, Rinv, u, rn.logdet_hpd(R)))
    return out, kappa


def bar(kappa, L, K, T, N):
    return 2 * (4 * L * L + K) * kappa * U + (T + N * L + 8) * U


def close(got, want, tol, rounding=None):
    """|got - want| <= tol max|want| (+ rounding, an array of absolute allowances per element)."""
    want = np.asarray(want)
    scale = float(np.max(np.abs(want))) or 1.0
    err = np.abs(np.asarray(got).astype(want.dtype) - want)
    allowed = tol * scale + (0 if rounding is None else rounding)
    print("   worst {:.2e} of bar {:.2e} (relative to the largest entry); worst error / allowance "
          "{:.3f}".format(float(np.max(err)) / scale, tol, float(np.max(err / allowed))))
    return bool(np.all(err <= allowed))


def device_parts(amd, basis, parts):
    return [(amd["dv"].to_device(T, dtype=np.complex128), f0, c0) for T, (f0, c0, _, _) in zip(basis, parts)]


def run_modes(amd, X, W, basis, V, pi, parts, n_blocks):
    """Every mode of the frame kernel on the device: host arrays and the route flags."""
    dv, ops = amd["dv"], amd["ops"]
    B, N, F, T = X.shape
    up = dv.to_device
    dX, dW, dV, dpi = up(X), up(W), up(V), up(pi)
    dparts = device_parts(amd, basis, parts)
    route = dv.zeros((B, N, n_blocks, T), dv.i32)
    quad, logdet = ops.ipsdta_quadratic(dX, dW, dparts, dV, n_blocks, route)
    num, den = ops.ipsdta_activation_terms(dX, dW, dparts, dV, dpi, n_blocks)
    stats = [tuple(dv.to_host(t) for t in ops.ipsdta_basis_statistics(dX, dW, p, dV, dpi, n_blocks))
             for p in dparts]
    covs = [dv.to_host(ops.ipsdta_weighted_covariance(dX, dW, p, dV, dpi, n_blocks)) for p in dparts]
    return dict(quad=dv.to_host(quad), logdet=dv.to_host(logdet), num=dv.to_host(num),
                den=dv.to_host(den), stats=stats, covs=covs, route=dv.to_host(route))


def check_modes(got, b, X, basis, V, pi, parts, exact, kappa):
    """Every output of mixture b, elementwise, against the longdouble (y, R^-1, u, log det R)."""
    N, F, T = X.shape
    K = V.shape[1]
    Vb, pib = V.astype(LD), pi.astype(LD)
    for p, ((f0, c0, C, L), (y, Rinv, u, ld)) in enumerate(zip(parts, exact)):
        tol = bar(kappa, L, K, T, N)
        Tb = basis[p].astype(CLD)
        sl = slice(c0, c0 + C)
        q = np.real(np.einsum("ntca,ntca->nct", np.conj(y), u))
        q_terms = np.einsum("ntca,ntca->nct", np.abs(y), np.abs(u))
        assert close(got["quad"][b][:, sl], q, tol, (2 * L + 2) * U * q_terms)
        assert close(got["logdet"][b][:, sl], ld.transpose(0, 2, 1), L * tol + L * U)
        nm = np.real(np.einsum("ntca,nkcab,ntcb,nt->nkct", np.conj(u), Tb, u, pib))
        dn = np.real(np.einsum("ntcab,nkcba->nkct", Rinv, Tb))
        nm_terms = np.einsum("ntca,nkcab,ntcb,nt->nkct", np.abs(u), np.abs(Tb), np.abs(u), pib)
        dn_terms = np.einsum("ntcab,nkcba->nkct", np.abs(Rinv), np.abs(Tb))
        assert close(got["num"][b][:, :, sl], nm, 2 * tol, (4 * L * L + 6) * U * nm_terms)
        assert close(got["den"][b][:, :, sl], dn, tol, (2 * L * L + 2) * U * dn_terms)
        P = np.einsum("nkt,ntcab->nkcab", Vb, Rinv) / T
        Q = np.einsum("nkt,nt,ntca,ntcb->nkcab", Vb, pib, u, np.conj(u)) / T
        assert close(got["stats"][p][0][b], P, tol)
        assert close(got["stats"][p][1][b], Q, 2 * tol)
        x = rn.blocks_of(X.astype(CLD), parts[p], 1)
        cov = np.einsum("nt,ntcba,pcat,qcbt->cabnpq", pib, Rinv, x, np.conj(x)) / T
        assert close(got["covs"][p][b], cov, tol)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B{}N{}F{}T{}C{}K{}".format(*s))
def test_frame_pass_elementwise(amd, shape):
    B, N, F, T, n_blocks, K = shape
    X, W, basis, V, pi, parts = draw_problem(31 + F, *shape)
    got = run_modes(amd, X, W, basis, V, pi, parts, n_blocks)
    assert int(got["route"].sum()) == 0  # cond(R) <= 1e4 with |R| ~ 1: nothing near the floor
    for b in range(B):
        exact, kappa = exact_frame(X[b], W[b], [t[b] for t in basis], V[b], parts)
        assert kappa <= 1e4
        check_modes(got, b, X[b], [t[b] for t in basis], V[b], pi[b], parts, exact, kappa)


def test_unweighted_pass_equals_unit_weight(amd):
    """pi = NULL (the Gaussian model) is weight 1, bit for bit."""
    dv, ops = amd["dv"], amd["ops"]
    shape = (1, 3, 7, 65, 2, 2)
    X, W, basis, V, _, parts = draw_problem(5, *shape)
    dX, dW, dV = dv.to_device(X), dv.to_device(W), dv.to_device(V)
    ones = dv.to_device(np.ones((1, 3, 65)))
    dparts = device_parts(amd, basis, parts)
    for p in dparts:
        for a, b in zip(ops.ipsdta_basis_statistics(dX, dW, p, dV, None, 2),
                        ops.ipsdta_basis_statistics(dX, dW, p, dV, ones, 2)):
            assert np.array_equal(dv.to_host(a), dv.to_host(b))


def test_floored_route_rank_deficient_basis(amd):
    """K = 1, T = a a^H scaled so that R's largest eigenvalue is ~1e-6: to_psd lifts the other
    eigenvalues to 1e-10, kappa after flooring ~1e4.  The floored matrix is known in closed form,
    R = lam a a^H + 1e-10 (I - a a^H) with |a| = 1, and so are its inverse and determinant; every mode
    of the kernel is compared with them (the packed LDS forms behind the repair included)."""
    B, N, F, T, n_blocks, K, L = 1, 2, 8, 65, 2, 1, 4
    rng = np.random.default_rng(77)
    X = 1e-3 * (rng.standard_normal((B, N, F, T)) + 1j * rng.standard_normal((B, N, F, T)))
    W = np.eye(N) + 0.3 * (rng.standard_normal((B, F, N, N)) + 1j * rng.standard_normal((B, F, N, N)))
    a = rng.standard_normal((B, N, K, n_blocks, L)) + 1j * rng.standard_normal((B, N, K, n_blocks, L))
    a /= np.linalg.norm(a, axis=-1, keepdims=True)
    basis = 1e-6 * a[..., :, None] * np.conj(a[..., None, :])
    V = 0.5 + 0.5 * rng.random((B, N, K, T))
    pi = 0.5 + rng.random((B, N, T))
    parts = rn.split_sizes(F, n_blocks)
    got = run_modes(amd, X, W, [basis], V, pi, parts, n_blocks)
    assert int(got["route"].sum()) == B * N * n_blocks * T  # every matrix took the eigenvalue route
    al = a[0, :, 0].astype(CLD)  # (N, C, L), re-normalised in longdouble
    al = al / np.sqrt(np.sum(np.abs(al) ** 2, axis=-1, keepdims=True))
    norm2 = np.sum(np.abs(a[0, :, 0].astype(CLD)) ** 2, axis=-1)  # (N, C), 1 to rounding
    lam = 1e-6 * V[0, :, 0].astype(LD)[:, :, None] * norm2[:, None, :]  # (N, T, C)
    floor = LD(1e-10)
    aa = al[:, None, :, :, None] * np.conj(al[:, None, :, None, :])  # (N, 1, C, L, L)
    eye = np.eye(L, dtype=CLD)
    Rinv = aa / lam[..., None, None] + (eye - aa) / floor  # (N, T, C, L, L)
    Y = np.einsum("fnm,mft->nft", W[0].astype(CLD), X[0].astype(CLD))
    y = np.transpose(rn.blocks_of(Y, parts[0], 1), (0, 3, 1, 2))  # (N, T, C, L)
    u = np.einsum("ntcab,ntcb->ntca", Rinv, y)
    ld = np.log(lam) + (L - 1) * np.log(floor)
    kappa = float(np.max(lam) / floor)
    assert 3e3 <= kappa <= 1.1e4
    check_modes(got, 0, X[0], [basis[0]], V[0], pi[0], parts, [(y, Rinv, u, ld)], kappa)


@pytest.mark.parametrize("delta,flag", [(1e-10 * (1 + 1e-3), 0), (1e-10 * (1 - 1e-3), 1),
                                        (1e-10 * (1 + 1e-12), None)])
def test_shortcut_takes_the_route_that_matches_to_psd(amd, delta, flag):
    """R = diag(1, delta): above the floor the Cholesky shortcut proves the floor idle, below it the
    eigenvalue route lifts delta to 1e-10; within rounding of the floor either route gives the same
    matrix (flag None: not asserted)."""
    dv, ops = amd["dv"], amd["ops"]
    B, N, F, T = 1, 2, 2, 3
    basis = np.zeros((B, N, 1, 1, 2, 2), dtype=complex)
    basis[..., 0, 0], basis[..., 1, 1] = 1.0, delta
    X = np.ones((B, N, F, T), dtype=complex)
    X[:, :, 1] = 1e-5
    W = np.tile(np.eye(N, dtype=complex), (B, F, 1, 1))
    route = dv.zeros((B, N, 1, T), dv.i32)
    quad, logdet = ops.ipsdta_quadratic(dv.to_device(X), dv.to_device(W), [(dv.to_device(basis), 0, 0)],
                                        dv.to_device(np.ones((B, N, 1, T))), 1, route)
    if flag is not None:
        assert set(dv.to_host(route).ravel().tolist()) == {flag}
    lifted = max(delta, 1e-10)
    np.testing.assert_allclose(dv.to_host(quad), 1.0 + 1e-10 / lifted, rtol=1e-12)
    np.testing.assert_allclose(dv.to_host(logdet), np.log(lifted), rtol=1e-12)


@pytest.mark.parametrize("model,dof", [("gauss", None), ("t", 3.0), ("t", 100.0)])
@pytest.mark.parametrize("n_low", [5, 3])
def test_weight_and_loss_elementwise(amd, model, dof, n_low):
    dv, ops, lib = amd["dv"], amd["ops"], amd["lib"]
    B, N, C, T, F = 3, 3, 5, 130, 23
    rng = np.random.default_rng(9)
    quad = rng.random((B, N, C, T)) * 3 - 0.02  # (a few negative: the floor at 0 acts)
    quad[:, :, :n_low, 5] = -rng.random((B, N, n_low))  # frame 5: the low partition's sum is negative,
    quad[:, :, n_low:, 7] = -rng.random((B, N, C - n_low))  # frame 7: the high one's (where there is one)
    logdet = rng.standard_normal((B, N, C, T))
    loss = dv.zeros((B,), dv.f64)
    pi = ops.ipsdta_weight_loss(dv.to_device(quad), dv.to_device(logdet), n_low, F,
                                lib.SOURCE_T if dof else lib.SOURCE_GAUSS, dof or 0.0,
                                want_pi=bool(dof), loss=loss)
    q, ld = quad.astype(LD), logdet.astype(LD)
    if dof:
        s = np.maximum(q, 0).sum(axis=2)
        want_pi = (dof + 2 * F) / (dof + 2 * s)
        assert close(dv.to_host(pi), want_pi, (C + 4) * U)
        data = np.sum((dof + 2 * F) / 2 * np.log(1 + 2 / LD(dof) * s), axis=1)
    else:
        assert pi is None
        low, high = q[:, :, :n_low].sum(axis=(1, 2)), q[:, :, n_low:].sum(axis=(1, 2))
        assert np.all(low[:, 5] < 0) and (n_low == C or np.all(high[:, 7] < 0))
        data = np.maximum(low, 0) + np.maximum(high, 0)
    want = np.mean(data + ld.sum(axis=(1, 2)), axis=-1)
    # N C T terms of size <= (nu + 2F) / 2 log(..) summed in any order
    scale = float(np.max(np.abs(data)) + np.max(np.abs(ld)) * N * C)
    assert np.max(np.abs(dv.to_host(loss).astype(LD) - want)) <= (N * C + T + 8) * U * scale


@pytest.mark.parametrize("B,N,K,C,T", [(1, 2, 1, 1, 1), (3, 3, 2, 5, 65), (1, 8, 32, 3, 130)])
def test_activation_update_elementwise(amd, B, N, K, C, T):
    dv, ops = amd["dv"], amd["ops"]
    rng = np.random.default_rng(4)
    V, num, den = rng.random((B, N, K, T)), rng.random((B, N, K, C, T)), 0.1 + rng.random((B, N, K, C, T))
    V[..., ::4] = 0.0
    got = dv.to_host(ops.ipsdta_activation(dv.to_device(V), dv.to_device(num), dv.to_device(den)))
    want = V.astype(LD) * np.sqrt(num.astype(LD).sum(axis=3) / den.astype(LD).sum(axis=3))
    assert close(got, want, (2 * C + 4) * U)
    assert np.all(got[..., ::4] == 0.0)


@pytest.mark.parametrize("C_low,L_low,C_high", [(3, 1, 0), (2, 3, 2), (1, 8, 0), (300, 2, 1)])
def test_normalisation_elementwise(amd, C_low, L_low, C_high):
    dv, ops = amd["dv"], amd["ops"]
    B, N, K, T = 2, 3, 2, 65
    rng = np.random.default_rng(6)

    def cplx(*s):
        return rng.standard_normal(s) + 1j * rng.standard_normal(s)

    low = cplx(B, N, K, C_low, L_low, L_low) + 3 * np.eye(L_low)
    high = cplx(B, N, K, C_high, L_low + 1, L_low + 1) + 3 * np.eye(L_low + 1) if C_high else None
    V = rng.random((B, N, K, T))
    dl, dh, dV = dv.to_device(low), (dv.to_device(high) if C_high else None), dv.to_device(V)
    ops.ipsdta_normalize(dl, dh, dV)
    tr = np.real(np.trace(low.astype(CLD), axis1=-2, axis2=-1)).sum(axis=-1)
    if C_high:
        tr = tr + np.real(np.trace(high.astype(CLD), axis1=-2, axis2=-1)).sum(axis=-1)
    n_terms = C_low * L_low + C_high * (L_low + 1)
    tol = (n_terms + 4) * U * float(np.max(np.abs(low))) * n_terms / float(np.min(np.abs(tr)))
    assert close(dv.to_host(dl), low.astype(CLD) / tr[..., None, None, None], tol)
    if C_high:
        assert close(dv.to_host(dh), high.astype(CLD) / tr[..., None, None, None], tol)
    assert close(dv.to_host(dV), V.astype(LD) * tr[..., None], tol)


@pytest.mark.parametrize("L", [1, 2, 3, 5, 8])
def test_matmul3_elementwise(amd, L):
    dv, ops = amd["dv"], amd["ops"]
    rng = np.random.default_rng(L)
    A, Bm, C = (rng.standard_normal((67, L, L)) + 1j * rng.standard_normal((67, L, L)) for _ in range(3))
    got = dv.to_host(ops.matmul3(dv.to_device(A), dv.to_device(Bm), dv.to_device(C)))
    want = (A.astype(CLD) @ Bm.astype(CLD)) @ C.astype(CLD)
    mag = (np.abs(A) @ np.abs(Bm)) @ np.abs(C)
    assert np.all(np.abs(got - want) <= (4 * L + 8) * U * mag)


def test_basis_step_products(amd):
    """T Q T and Q' T P T Q' as the class forms them are Hermitian to rounding for Hermitian inputs."""
    dv, ops = amd["dv"], amd["ops"]
    rng = np.random.default_rng(12)
    G = rng.standard_normal((2, 40, 5, 5)) + 1j * rng.standard_normal((2, 40, 5, 5))
    T, Q = (g @ np.conj(np.swapaxes(g, -2, -1)) for g in G)
    got = dv.to_host(ops.matmul3(dv.to_device(T), dv.to_device(Q), dv.to_device(T)))
    want = T.astype(CLD) @ Q.astype(CLD) @ T.astype(CLD)
    assert close(got, want, 64 * U)
    assert close(got, np.conj(np.swapaxes(got, -2, -1)), 64 * U)


# ------------------------------------------------------------------------------ VCD
@pytest.mark.parametrize("key", ["a", "b", "c", "d"])
def test_vcd_operator_against_reference(amd, key):
    g = load_golden(ic.VCD_FIXTURE)
    usm = amd["usm"]
    W, RXX = g["W_" + key], g["RXX_" + key]
    keep = W.copy()
    out = usm.update_by_block_decomposition_vcd(W, RXX, overwrite=False)
    assert np.array_equal(W, keep) and ic.err(out, g["out_" + key]) <= 1e-10
    out = usm.update_by_block_decomposition_vcd(W, RXX, singular_fn=usm.abs_below(1e-10))
    assert out is W and ic.err(W, g["out_floor_" + key]) <= 1e-10


def test_vcd_singular_branch(amd):
    """One bin per block: gamma = 0, so xi_hat is exactly 0.  singular_fn=None (x == 0) and any
    positive threshold take w = eta / sqrt(xi); threshold 0 (the identity flooring) never does and
    follows the regular formula into 0 / 0 like the reference."""
    usm, ops, dv = amd["usm"], amd["ops"], amd["dv"]
    rng = np.random.default_rng(3)
    C, L, N = 5, 1, 3
    W = np.eye(N) + 0.3 * (rng.standard_normal((C, L, N, N)) + 1j * rng.standard_normal((C, L, N, N)))
    G = rng.standard_normal((C, N, N, 2 * N)) + 1j * rng.standard_normal((C, N, N, 2 * N))
    RXX = (G @ np.conj(np.swapaxes(G, -2, -1)))[:, None, None]
    want = rn.vcd(W, RXX, threshold=5e-324)
    assert np.all(np.isfinite(want))
    for fn in (None, usm.abs_below(1e-10)):
        got = usm.update_by_block_decomposition_vcd(W, RXX, singular_fn=fn, overwrite=False)
        assert ic.err(got, want) <= 1e-12
    dW = dv.to_device(W.reshape(1, C * L, N, N))
    ops.ipsdta_vcd(dW, dv.to_device(RXX.reshape(1, C, L, L, N, N, N)), 0, 0.0)
    assert np.all(np.isnan(dv.to_host(dW)))
    # with more than one bin per block xi_hat is generic: threshold 0 and None agree, finite
    g = load_golden(ic.VCD_FIXTURE)
    W2, R2 = g["W_b"], g["RXX_b"]
    C2, L2, N2 = W2.shape[:3]
    dW2 = dv.to_device(W2.reshape(1, C2 * L2, N2, N2))
    ops.ipsdta_vcd(dW2, dv.to_device(R2.reshape(1, C2, L2, L2, N2, N2, N2)), 0, 0.0)
    assert ic.err(dv.to_host(dW2).reshape(W2.shape), g["out_b"]) <= 1e-10


def vcd_row_bar(d, L, N):
    """Error bar of one row update w = conj(coeff eta - eta_hat), relative to |w|_2, from the
    longdouble intermediates ``d`` of rn.vcd_row (per block), u = 2^-53.
      eta     = (W_i U)^-1 e_n: the product W_i U is off by N u |W||U| and the LU solve by ~ 4 N u
                backward, so |d eta| <= 8 N k(W_i U) u |eta|, k(.) = |A|_F |A^-1|_F;
      gamma   : (L - 1) N terms, |d gamma| <= L N u sum|terms| = L N g u |gamma|, g = sum|terms| / |gamma|;
      eta_hat = U^-1 gamma: |d eta_hat| <= (8 N + L N g) k(U) u |eta_hat|;
      xi      = eta^H U eta, xi_hat = eta^H U eta_hat: products of the above, relative errors
                a_xi (2 e_eta + N^2 u), a_xh (e_eta + e_hat + N^2 u), a_* = |eta||U||.| / |xi_*|;
      coeff   = f(xi, xi_hat), smooth: at most 2 (rel xi + rel xi_hat) + 16 u (sqrt, divisions);
      w       : |d w| <= |coeff||eta| (e_coeff + e_eta) + |eta_hat| e_hat.
    Every factor is measured in longdouble; a safety factor 4 covers the constants dropped."""
    def fro(A):
        return np.sqrt(np.sum(np.abs(A) ** 2, axis=tuple(range(1, A.ndim))))
    k_wu, k_u = fro(d["WU"]) * fro(d["WUinv"]), fro(d["U"]) * fro(d["Uinv"])
    n_eta, n_hat, n_u = fro(d["eta"]), fro(d["eta_hat"]), fro(d["U"])
    gsum = sum(fro(t) for t in d["terms"]) if d["terms"] else 0 * n_eta
    g = np.where(fro(d["gamma"]) > 0, gsum / np.where(fro(d["gamma"]) > 0, fro(d["gamma"]), 1), 0)
    e_eta = 8 * N * k_wu * U
    e_hat = (8 * N + L * N * g) * k_u * U
    a_xi = n_eta * n_u * n_eta / d["xi"]
    a_xh = np.where(d["sing"], 0, n_eta * n_u * n_hat / np.abs(d["xi_hat"]))
    e_coeff = 2 * (a_xi * (2 * e_eta + N * N * U) + a_xh * (e_eta + e_hat + N * N * U)) + 16 * U
    return 4 * (np.abs(d["coeff"]) * n_eta * (e_coeff + e_eta) + n_hat * e_hat)


@pytest.mark.parametrize("B,C,L,N", [(3, 70, 3, 4), (1, 5, 1, 2), (1, 3, 8, 3), (2, 4, 2, 8)])
def test_vcd_sweep_elementwise_against_longdouble(amd, B, C, L, N):
    """Row by row against numpy.longdouble.  A row's final value is the value its own update wrote,
    so the state the device saw at step (i, n) is known from its result: the final rows of the steps
    before, the initial rows of the others.  Each row is recomputed in longdouble from exactly that
    state and compared per element with the bar of vcd_row_bar -- no error is inherited from earlier
    rows, so the bar carries only the step's own cond(U) and cond(W_i U)."""
    ops, dv = amd["ops"], amd["dv"]
    rng = np.random.default_rng(8 + L)
    W = np.eye(N) + 0.3 * (rng.standard_normal((B, C, L, N, N)) + 1j * rng.standard_normal((B, C, L, N, N)))
    G = rng.standard_normal((B, C, N, L * N, 2 * L * N)) + 1j * rng.standard_normal((B, C, N, L * N, 2 * L * N))
    H = (G @ np.conj(np.swapaxes(G, -2, -1)) / (2 * L * N)).reshape(B, C, N, L, N, L, N)
    RXX = np.ascontiguousarray(H.transpose(0, 1, 3, 5, 2, 4, 6))
    # the sweep covers bins 2 .. 2 + C L of a longer filter bank and leaves the others alone
    bank = np.zeros((B, C * L + 5, N, N), dtype=complex)
    bank[:, 2:2 + C * L] = W.reshape(B, C * L, N, N)
    info = dv.zeros((1,), dv.i32)
    dW = dv.to_device(bank)
    ops.ipsdta_vcd(dW, dv.to_device(RXX), 2, 1e-10, info)
    got = dv.to_host(dW)
    assert int(info.item()) == 0 and np.all(got[:, :2] == 0) and np.all(got[:, 2 + C * L:] == 0)
    got = got[:, 2:2 + C * L].reshape(W.shape)
    worst = 0.0
    for b in range(B):
        state, R = W[b].astype(CLD), RXX[b].astype(CLD)
        for i in range(L):
            for n in range(N):
                d = {}
                want = rn.vcd_row(state, R, i, n, threshold=LD(1e-10), details=d)
                assert not np.any(d["sing"]) or L == 1
                tol = vcd_row_bar(d, L, N)
                err = np.abs(got[b, :, i, n].astype(CLD) - want)
                worst = max(worst, float(np.max(err / tol[:, None])))
                assert np.all(err <= tol[:, None]), (b, i, n, float(np.max(err / tol[:, None])))
                state[:, i, n] = got[b, :, i, n]  # the next steps saw the device's row
    print("   worst error / bar {:.3f}".format(worst))
