"""CACGMM on the device against the NumPy restatement (tests/cacgmm_numpy.py) and the reference's
fixtures.

Bars.  cACGMM collapses a few components per run onto single frames; their covariances reach the
eigenvalue floor and every later quantity inherits condition numbers of 1e10.  The bar of a quantity
is therefore 1000 x the largest movement of the restatement itself under three 1e-15 relative
perturbations of the input over all test mixtures (profiles/cacgmm_sensitivity.txt, written by
benchmarks/tools/cacgmm_sensitivity.py; the factor pays for the device summing the frames in another
order), capped at 1e-6 for parameters and outputs and 1e-5 for the loss:

    measured movement   output 5.28e-09  posterior 5.53e-09  mixing 4.12e-10  covariance 6.86e-11
                        loss 3.04e-09 (relative)
    bar                 output 1e-6 (cap)  posterior 1e-6 (cap)  mixing 4.1e-7  covariance 6.9e-8
                        loss 3.0e-6 (relative)

The covariance is compared on the (source, bin) pairs whose restatement condition number stayed
below 1e6 at every iteration (at most 25 % may be excluded); the others are checked for being
Hermitian, for trace 1 and for their smallest eigenvalue.
"""

import functools

import numpy as np
import pytest

import cacgmm_numpy as cn
from conftest import load_golden
from test_golden_cacgmm import golden_options

pytestmark = pytest.mark.gpu

BAR = dict(output=1e-6, posterior=1e-6, mixing=4.1e-7, covariance=6.9e-8, loss=3.0e-6)
FLOOR = 1e-10


def device_floor(spec):
    from ssspy_amd.special.flooring import add_flooring, max_flooring

    if spec is None:
        return None
    return functools.partial(max_flooring if spec[0] == "max" else add_flooring, eps=spec[1])


def make(opts, **more):
    from ssspy_amd.bss import CACGMM

    opts = dict(opts)
    flooring = opts.pop("flooring", ("max", FLOOR))
    opts.update(more)
    opts.setdefault("rng", np.random.default_rng(0))
    for key in ("global_iter", "local_iter"):
        if opts.get(key) == 1 or not opts.get("permutation_alignment", True) or \
                "correlation" in str(opts.get("permutation_alignment")):
            opts.pop(key, None)
    return CACGMM(flooring_fn=device_floor(flooring), **opts)


_reference = {}


def reference(case):
    if case not in _reference:
        X = cn.make_mixture(*case)
        r = cn.run(X, np.random.default_rng(0), n_sources=case[1])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        _reference[case] = (X, r)
    return _reference[case]


def check_run(m, Y, r, what=""):
    print(what, "output", np.abs(Y - r["output"]).max(),
          "posterior", np.abs(m.posterior - r["posterior"]).max(),
          "mixing", np.abs(m.mixing - r["final_mixing"]).max(),
          "loss", np.abs(np.array(m.loss) / r["loss"] - 1).max())
    assert np.abs(Y - r["output"]).max() <= BAR["output"]
    assert np.abs(m.posterior - r["posterior"]).max() <= BAR["posterior"]
    assert np.abs(m.mixing - r["final_mixing"]).max() <= BAR["mixing"]
    assert len(m.loss) == len(r["loss"])
    assert np.abs(np.array(m.loss) / r["loss"] - 1).max() <= BAR["loss"]
    keep = (np.linalg.cond(r["covariance"]) < 1e6).all(axis=0)
    if r["permutation"] is not None:  # the mask follows the components
        keep = np.take_along_axis(keep.T, r["permutation"], axis=1).T
    assert 1 - keep.mean() <= 0.25
    cov = np.asarray(m.covariance)
    diff = np.abs(cov - r["final_covariance"]).max(axis=(-2, -1))
    print(what, "covariance", diff[keep].max(), "excluded", 1 - keep.mean())
    assert diff[keep].max() <= BAR["covariance"]
    return cov, keep


@pytest.mark.parametrize("case", cn.CASES, ids=str)
def test_full_run_against_restatement(case):
    X, r = reference(case)
    m = make(dict(n_sources=case[1], permutation_alignment=False))
    Y = m(X, n_iter=cn.N_ITER)
    cov, keep = check_run(m, Y, r, str(case))
    assert np.abs(m.posterior.sum(axis=0) - 1).max() <= 1e-14
    # collapsed pairs: Hermitian, trace 1, smallest eigenvalue at the floor over the trace or above
    assert np.abs(cov - cov.swapaxes(-2, -1).conj()).max() <= 1e-15
    assert np.abs(np.trace(cov, axis1=-2, axis2=-1).real - 1).max() <= 1e-12
    # one more M step by hand: before the normalisation the eigenvalues are at the floor or above,
    # after it at the floor over the trace it was divided by
    # (float64 eigvalsh on the host returns an eigenvalue to about M u ||B||, which is 1e-5 of a
    #  floored 1e-10 beside eigenvalues of order 1: that absolute term is the checker's own error,
    #  allowed as 8 M u lambda_max beside the rtol of 1e-6)
    u, M = 2.0 ** -53, case[0]
    m.update_parameters()
    raw = np.asarray(m.covariance)
    lam = np.linalg.eigvalsh(raw)
    assert (lam[..., 0] >= FLOOR * (1 - 1e-6) - 8 * M * u * lam[..., -1]).all()
    trace = np.trace(raw, axis1=-2, axis2=-1).real
    m.normalize_covariance()
    lam = np.linalg.eigvalsh(np.asarray(m.covariance))
    assert (lam[..., 0] >= FLOOR / trace * (1 - 1e-6) - 8 * M * u * lam[..., -1]).all()


@pytest.mark.parametrize("name", sorted(cn.GOLDEN))
def test_fixture_with_alignment(name):
    g = load_golden(name)
    opts = golden_options(g)
    r = cn.run(g["input"], np.random.default_rng(0), **opts)
    m = make(opts)
    Y = m(g["input"], n_iter=cn.N_ITER)
    if opts["permutation_alignment"]:
        assert np.array_equal(m._applied_permutation, r["permutation"])
    check_run(m, Y, r, name)
    assert np.abs(Y - g["output"]).max() <= BAR["output"]
    assert np.abs(m.posterior - g["posterior"]).max() <= BAR["posterior"]
    np.testing.assert_allclose(m.loss, g["loss"], rtol=BAR["loss"])


@pytest.mark.parametrize("case", [c for c in cn.CASES if c[1] <= 4 and c[2] <= 64], ids=str)
@pytest.mark.parametrize("how", ["posterior_score", "amplitude_score", "amplitude_correlation"])
def test_alignment_permutations(case, how):
    X = cn.make_mixture(*case)
    r = cn.run(X, np.random.default_rng(0), n_sources=case[1], permutation_alignment=how)
    m = make(dict(n_sources=case[1], permutation_alignment=how))
    Y = m(X, n_iter=cn.N_ITER)
    assert np.array_equal(m._applied_permutation, r["permutation"])
    check_run(m, Y, r, str(case) + how)


CASE = (3, 4, 17, 80)


def run_once(**kw):
    X = cn.make_mixture(*CASE)
    m = make(dict(n_sources=CASE[1], permutation_alignment=False), **kw)
    Y = m(X, n_iter=cn.N_ITER)
    return m, Y


def test_bit_identical_runs_and_record_loss():
    a, Ya = run_once()
    b, Yb = run_once()
    c, Yc = run_once(record_loss=False)
    for other, Yo in ((b, Yb), (c, Yc)):
        assert np.array_equal(Ya, Yo)
        assert np.array_equal(a.covariance, other.covariance)
        assert np.array_equal(a.mixing, other.mixing)
        assert np.array_equal(a.posterior, other.posterior)
    assert a.loss == b.loss and len(a.loss) == cn.N_ITER + 1 and c.loss is None


def test_callback_reading_state_changes_nothing():
    seen = []

    def look(method):
        seen.append((None if method.posterior is None else method.posterior.copy(),
                     method.covariance.copy()))

    a, Ya = run_once()
    b, Yb = run_once(callbacks=look)
    assert len(seen) == cn.N_ITER + 1 and seen[0][0] is None
    assert np.abs(seen[1][0].sum(axis=0) - 1).max() <= 1e-14
    assert np.array_equal(Ya, Yb) and np.array_equal(a.covariance, b.covariance)
    assert a.loss == b.loss


def test_steps_by_hand_equal_update_once_equal_call():
    X = cn.make_mixture(*CASE)
    a, _ = run_once()
    ms = []
    for by_hand in (True, False):
        m = make(dict(n_sources=CASE[1], permutation_alignment=False))
        m(X, n_iter=0)
        for _ in range(cn.N_ITER):
            if by_hand:
                m.update_posterior()
                m.update_parameters()
                m.normalize_covariance()
            else:
                m.update_once()
        ms.append(m)
    for m in ms:
        assert np.array_equal(m.covariance, a.covariance) and np.array_equal(m.mixing, a.mixing)
    # separate() without a posterior: the E step of the current parameters, not stored
    m = ms[0]
    before = m.posterior.copy()
    Y = m.separate(X)
    m.update_posterior()
    assert np.array_equal(Y, m.posterior * X[m.reference_id])
    assert not np.array_equal(before, m.posterior)
    assert np.array_equal(a.posterior, m.posterior)


def test_batch_equals_single_runs_on_a_shared_generator():
    Xs = np.stack([cn.make_mixture(*CASE, seed=40 + b) for b in range(3)])
    batch = make(dict(n_sources=CASE[1], permutation_alignment=True))
    Yb = batch(Xs, n_iter=cn.N_ITER)
    assert np.array(batch.loss).shape == (cn.N_ITER + 1, 3)
    rng = np.random.default_rng(0)
    for b in range(3):
        m = make(dict(n_sources=CASE[1], permutation_alignment=True), rng=rng)
        Y = m(Xs[b], n_iter=cn.N_ITER)
        assert np.abs(Y - Yb[b]).max() <= 1e-10
        assert np.abs(np.array(m.loss) - np.array(batch.loss)[:, b]).max() <= 1e-10
        assert np.array_equal(m._applied_permutation, batch._applied_permutation[b])


@pytest.mark.parametrize("case", [(2, 1, 3, 70), (3, 2, 1, 65), (4, 3, 2, 257)], ids=str)
def test_edge_shapes(case):
    X = cn.make_mixture(*case)
    r = cn.run(X, np.random.default_rng(0), n_sources=case[1])
    m = make(dict(n_sources=case[1], permutation_alignment=False))
    Y = m(X, n_iter=cn.N_ITER)
    check_run(m, Y, r, str(case))


def test_batch_on_the_narrow_tile():
    """Two mixtures of 8 channels and 16 sources: the 128-frame tile of the pass, batched."""
    case = (8, 16, 3, 300)
    Xs = np.stack([cn.make_mixture(*case), cn.make_mixture(*case, seed=5)])
    m = make(dict(n_sources=16, permutation_alignment=False))
    Ys = m(Xs, n_iter=cn.N_ITER)
    rng = np.random.default_rng(0)
    for b in range(2):
        r = cn.run(Xs[b], rng, n_sources=16)
        assert np.abs(Ys[b] - r["output"]).max() <= BAR["output"]
        assert np.abs(m.posterior[b] - r["posterior"]).max() <= BAR["posterior"]
        assert np.abs(m.mixing[b] - r["final_mixing"]).max() <= BAR["mixing"]
        assert np.abs(np.array(m.loss)[:, b] / r["loss"] - 1).max() <= BAR["loss"]


def test_unsupported_cases_raise():
    from ssspy_amd.bss import CACGMM

    rng = np.random.default_rng(0)

    def mix(M):
        return rng.standard_normal((M, 3, 20)) + 1j * rng.standard_normal((M, 3, 20))

    with pytest.raises(NotImplementedError, match="channels"):
        CACGMM()(mix(1), n_iter=1)
    with pytest.raises(NotImplementedError, match="channels"):
        CACGMM(n_sources=2)(mix(9), n_iter=1)
    with pytest.raises(NotImplementedError, match="sources"):
        CACGMM(n_sources=17)(mix(4), n_iter=1)
    with pytest.raises(NotImplementedError, match="flooring"):
        CACGMM(flooring_fn=lambda x: np.maximum(x, 1e-3))(mix(4), n_iter=1)
    with pytest.raises(AssertionError, match="Only amplitude"):
        CACGMM(permutation_alignment="posterior_correlation")(mix(2), n_iter=1)


# ------------------------------------------------------------------------------------------------
# Single pass, tight: every kernel of the iteration alone through _ops, each element against an
# extended-precision (np.longdouble) evaluation of the SAME float64 inputs the kernel was given.
L, CL = np.longdouble, np.clongdouble
U = 2.0 ** -53


def unpack_hermitian(packed, M):
    """(..., M * M) [M diagonal][re, im of the upper triangle, row-major] -> (..., M, M) complex."""
    H = np.zeros(packed.shape[:-1] + (M, M), dtype=CL)
    e = M
    for a in range(M):
        H[..., a, a] = packed[..., a]
        for c in range(a + 1, M):
            H[..., a, c] = packed[..., e].astype(L) + 1j * packed[..., e + 1].astype(L)
            H[..., c, a] = np.conj(H[..., a, c])
            e += 2
    return H


def check_pass(Z, binv, logp, out, T):
    """The frame pass against longdouble; Z (M, F, T), binv (N, F, M*M), logp (N, F) as the kernel
    read them (float64), out = (sum_gamma, num, loss, posterior) as it wrote them.

    Error bars, u = 2^-53, all from the operation counts of the kernel:
      q      = sum_ac conj(z_a) H_ac z_c: M^2 complex products and as many additions, so
               |dq| <= (2 M + 6) u qabs with qabs = sum_ac |z_a| |H_ac| |z_c| (no cancellation is
               assumed away: for an ill-conditioned B, qabs / q carries its condition number).
      lg     = logp - M log q: dlg = M dq / q + 3 u M |log q| + 2 u |lg| + 2 u (a 1-2 ulp log).
      gamma  = exp(lg - max) / s: with E = max_n dlg, the exponent is off by 2 E + u |lg - max|, s by
               the largest of its terms' relative errors + N u, hence
               dgamma / gamma <= 4 E + u (|lg_n - max| + max_m |lg_m - max|) + (N + 8) u.
      lse    = log s + max: dlse <= 3 E + u max_m |lg_m - max| + (N + 4) u + 2 u (|log s| + |lse|).
      sums over the T frames: the summands' bars added, plus (T + 4) u sum |summand| for the additions
               in whatever order (the kernel's depth is below T).
      w      = gamma / q: dw / w <= dgamma / gamma + dq / q + u; a term w z_a conj(z_c) adds 6 u.
    Every bar is doubled before use."""
    M, F, _ = Z.shape
    N = logp.shape[0]
    sum_gamma, num, loss, posterior = out
    Zl = Z.astype(CL)
    H = unpack_hermitian(binv, M)
    q = np.einsum("aft,nfac,cft->nft", np.conj(Zl), H, Zl).real
    qabs = np.einsum("aft,nfac,cft->nft", np.abs(Zl), np.abs(H), np.abs(Zl))
    assert (q > 10 * FLOOR).all(), "a floor is active: not the case this test is about"
    dq = (2 * M + 6) * U * qabs
    lg = logp.astype(L)[:, :, None] - M * np.log(q)
    dlg = M * dq / q + 3 * U * M * np.abs(np.log(q)) + 2 * U * np.abs(lg) + 2 * U
    E = dlg.max(axis=0)
    vmax = lg.max(axis=0)
    spread = np.abs(lg - vmax)
    e = np.exp(lg - vmax)
    s = e.sum(axis=0)
    gamma = e / s
    rel_gamma = 4 * E + U * (spread + spread.max(axis=0)) + (N + 8) * U
    lse = np.log(s) + vmax
    dlse = 3 * E + U * spread.max(axis=0) + (N + 4) * U + 2 * U * (np.abs(np.log(s)) + np.abs(lse))

    worst = {}

    def compare(name, got, want, bar):
        err = np.abs(got.astype(want.dtype) - want)
        ratio = float((err / (2 * bar)).max())
        worst[name] = (float(err.max()), ratio)
        assert ratio <= 1.0, (name, worst[name])

    compare("posterior", posterior, gamma, rel_gamma * gamma)
    compare("sum_gamma", sum_gamma, gamma.sum(axis=-1),
            (rel_gamma * gamma).sum(axis=-1) + (T + 4) * U * gamma.sum(axis=-1))
    compare("loss", loss, -lse.sum(axis=-1) / T,
            (dlse.sum(axis=-1) + (T + 4) * U * np.abs(lse).sum(axis=-1)) / T + U)
    w = gamma / q
    rel_w = rel_gamma + dq / q + U
    want = np.einsum("nft,aft,cft->nfac", w, Zl, np.conj(Zl))
    size = np.einsum("nft,aft,cft->nfac", w, np.abs(Zl), np.abs(Zl))
    bar = np.einsum("nft,aft,cft->nfac", w * (rel_w + 6 * U), np.abs(Zl), np.abs(Zl)) \
        + (T + 4) * U * size
    compare("num", num, want, bar)
    return worst


def gauss_inverse_logdet(A):
    """Inverse and log-determinant of Hermitian positive definite matrices (..., M, M) by
    Gauss-Jordan elimination without pivoting, in longdouble."""
    M = A.shape[-1]
    W = np.concatenate([A.astype(CL), np.broadcast_to(np.eye(M, dtype=CL), A.shape).copy()], axis=-1)
    logdet = np.zeros(A.shape[:-2], dtype=L)
    for k in range(M):
        pivot = W[..., k, k].real
        logdet = logdet + np.log(pivot)
        W[..., k, :] = W[..., k, :] / pivot[..., None]
        for r in range(M):
            if r != k:
                W[..., r, :] = W[..., r, :] - W[..., r, k][..., None] * W[..., k, :]
    return W[..., M:], logdet


def check_prepare(cov, mixing, binv, logp, M):
    """B^-1 and log alpha - log det B against longdouble elimination.  Bars: the Cholesky route has
    the backward error 8 M^2 u ||B|| at most (Higham, Accuracy and Stability, Thm 10.3 with a
    generous constant), so |d B^-1| <= 8 M^2 u cond(B) ||B^-1||_2 per element and every pivot is
    relatively off by 8 M^2 u cond(B) at most: |d logdet| <= M of those + 4 u sum |log pivot|
    <= 8 M^3 u cond(B) + 4 u (|logdet| + M); the logarithm of alpha and the subtraction add
    2 u |log alpha| + u |logp|.  Doubled before use."""
    inv, logdet = gauss_inverse_logdet(cov)
    kappa = np.linalg.cond(cov)
    norm_inv = np.linalg.norm(inv.astype(np.complex128), 2, axis=(-2, -1))
    bar = 8 * M * M * U * kappa * norm_inv
    err = np.abs(unpack_hermitian(binv, M) - inv).max(axis=(-2, -1))
    assert (err <= 2 * bar).all(), ("binv", float((err / bar).max()))
    want = np.log(mixing.astype(L)) - logdet
    bar = 8 * M ** 3 * U * kappa + 4 * U * (np.abs(logdet) + M) \
        + 2 * U * np.abs(np.log(mixing)) + U * np.abs(want)
    err = np.abs(logp - want)
    assert (err <= 2 * bar).all(), ("logp", float((err / bar).max()))
    return float(kappa.max())


@pytest.mark.parametrize("case", cn.CASES, ids=str)
def test_single_pass_elementwise(case):
    """Unit input, staging, frame pass and parameter step alone, from the reference's initial
    parameters (diagonal B, no floor active), then the staging and the frame pass once more on the
    full Hermitian B the parameter step leaves -- the diagonal start cannot see a wrong
    off-diagonal term.  Bars: see check_pass, check_prepare and the comments below."""
    import torch

    from ssspy_amd import _device as dv
    from ssspy_amd import _ops
    from ssspy_amd.utils.flooring import device_flooring

    M, N, F, T = case
    floor = device_flooring(device_floor(("max", FLOOR)))
    X = cn.make_mixture(*case)
    Xd = dv.to_device(X[None], dtype=np.complex128)
    Zd = _ops.cacgmm_unit_input(Xd, floor)
    Z = dv.to_host(Zd)[0]
    # Z = x / ||x||: M squares and additions, a square root, a division: (M + 4) u per component
    norm = np.sqrt((np.abs(X.astype(CL)) ** 2).sum(axis=0))
    assert (norm > 10 * FLOOR).all()
    want = X.astype(CL) / norm
    assert (np.abs(Z - want) <= 2 * (M + 4) * U * np.abs(want)).all()

    alpha, B = cn.init_parameters(np.random.default_rng(0), N, F, M)
    assert np.linalg.eigvalsh(B).min() > 10 * FLOOR and np.linalg.cond(B).max() < 1e4

    def run_pass(cov, mixing):
        covd = dv.to_device(cov[None], dtype=np.complex128)
        mixd = dv.to_device(mixing[None], dtype=np.float64)
        binv, logp = _ops.cacgmm_prepare(covd, mixd)
        sg = dv.empty((1, N, F), dv.f64, Xd.device)
        num = dv.empty((1, N, F, M, M), dv.c128, Xd.device)
        loss = dv.empty((1, F), dv.f64, Xd.device)
        post = dv.empty((1, N, F, T), dv.f64, Xd.device)
        _ops.cacgmm_frame_pass(Zd, binv, logp, floor, sum_gamma=sg, num=num, loss=loss,
                               posterior=post)
        host = [dv.to_host(t)[0] for t in (binv, logp, sg, num, loss, post)]
        kappa = check_prepare(cov, mixing, host[0], host[1], M)
        worst = check_pass(Z, host[0], host[1], host[2:], T)
        print(case, "cond", kappa, {k: "%.1e (%.2f of the bar)" % v for k, v in worst.items()})
        assert np.abs(host[5].sum(axis=0) - 1).max() <= 1e-14
        return sg, num, host[2], host[3]

    sg, num, sg_h, num_h = run_pass(B, alpha)

    mixd, covd = _ops.cacgmm_parameter_step(sg, num.clone(), T, floor, True)
    torch.cuda.synchronize()
    mixing2, cov2 = dv.to_host(mixd)[0], dv.to_host(covd)[0]
    # alpha = sum_gamma / T: one division.  B = to_psd(M num / sum_gamma) / trace: two roundings
    # for the scaling; the Jacobi sweeps apply at most 8 sweeps of M (M - 1) / 2 rotations, each a
    # backward error of 4 u ||B||_F at most, and the rebuild P diag(lam) P^H sums M products per
    # element: (16 M^2 + 2 M + 8) u ||B||_F per element, then M + 2 roundings for the trace and the
    # division, which the same constant covers.  No floor may act (eigenvalues > 10 x the floor).
    assert (np.abs(mixing2 - sg_h.astype(L) / T) <= 2 * U * mixing2).all()
    B0 = M * (num_h.astype(CL) / sg_h.astype(L)[..., None, None])
    B0 = (B0 + np.conj(np.swapaxes(B0, -2, -1))) / 2
    assert np.linalg.eigvalsh(B0.astype(np.complex128)).min() > 10 * FLOOR
    trace = np.trace(B0, axis1=-2, axis2=-1).real
    want = B0 / trace[..., None, None]
    fro = np.sqrt((np.abs(B0) ** 2).sum(axis=(-2, -1)))
    bar = (16 * M * M + 2 * M + 8) * U * fro / trace
    err = np.abs(cov2 - want).max(axis=(-2, -1))
    print(case, "parameter step: covariance", float(err.max()), "%.2f of the bar" % float((err / (2 * bar)).max()))
    assert (err <= 2 * bar).all()
    assert np.abs(cov2 - np.conj(np.swapaxes(cov2, -2, -1))).max() == 0

    run_pass(cov2, mixing2)
