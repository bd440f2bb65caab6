"""The device forms behind the public-surface additions, element by element against ``np.longdouble``
evaluations of the same float64 inputs, and against the reference's fixtures
(tests/golden/make_golden_surface.py) with the same bars.  u = 2^-53; every bar is derived from the
operation counts below and doubled before use, none from the code under test.

pair update (update_by_ip2_one_pair; it shares k_ip2 / k_ip2_rows / k_ip2_rt with update_by_ip2, so
  against that function the comparison is BITWISE).  Against longdouble, per row and up to the
  unit-modulus factor of an eigenvector (the fixture is compared with its phase): P = (W U)^-1 E by
  LU loses 4 N^2 kappa(W U) u (Higham, thm 9.4 / 10.4); the 2 x 2 generalised problem through the
  Cholesky factor of P^H U_n P loses kappa of that matrix, and an eigenvector moves by the
  perturbation over the relative gap of the two eigenvalues (asserted >= 1e-6 on the host first);
  the products P h and the normalisation add 8 N u:
      |row - ref| <= (4 N^2 kappa(W U) + 16 kappa_pair / gap + 8 N) u |ref|   (2-norms over the row).
reconstruction.  S = sum_k v T_k by K fused multiply-adds: |dS| <= (K + 1) u sum_k |v| |T_k|
  elementwise; to_psd of S is within C["psd"] u ||ref||_F of the exact projection (the bar of
  tests/linalg_reference.py, g = 1) and is 1-Lipschitz in S, so per matrix
      ||R - ref||_F <= (C["psd"] ||ref||_F + (K + 1) ||sum_k |v| |T_k| ||_F) u.
log-determinant.  LU with partial pivoting computes the factors of W + dW, |dW| <= 4 N u |L| |U|
  (complex operations: twice the real gamma_N), and d log|det| = Re tr(W^-1 dW); the N logarithms
  add 2 u each on |log|u_kk||:
      |d| <= 4 N u sum(|W^-1|^T * (|L| |U|)) + 3 u sum_k |log |u_kk|| + N u.
quadratic.  n^2 complex fused products: |d| <= (2 n + 6) u sum_ac |x_a| |A_ac| |x_c| per part.
softmax / logsumexp.  x - max costs u |x - max|, exp two more roundings: a term is off by
  e_k = (|x_k - max| + 3) u relatively; the sum of len positive terms in any order adds (len + 2) u,
  so s is off by E = sum_k w_k e_k + (len + 2) u (w the softmax weights);
      |d softmax_k| <= (e_k + E + 2 u) softmax_k,
      |d logsumexp| <= E + 2 u |log s| + 2 u |out|.
"""

import functools

import numpy as np
import pytest

import linalg_reference as lr
import pass_reference as pr
from conftest import load_golden

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD, CLD = np.longdouble, np.clongdouble
FLOORS = {"none": (0, 0.0), "max": (1, 1e-10), "add": (2, 1e-10)}


@pytest.fixture(scope="module")
def amd():
    import torch

    import ssspy_amd.bss.ipsdta as ipsdta
    from ssspy_amd import _device as dv, _ops
    from ssspy_amd import linalg, special
    from ssspy_amd.bss import _update_spatial_model as usm
    from ssspy_amd.special import flooring
    return dict(torch=torch, dv=dv, ops=_ops, usm=usm, flooring=flooring, linalg=linalg,
                special=special, ipsdta=ipsdta)


def cgauss(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def floor_fn(amd, kind):
    if kind == "none":
        return None
    fn = amd["flooring"].max_flooring if kind == "max" else amd["flooring"].add_flooring
    return functools.partial(fn, eps=FLOORS[kind][1])


# ------------------------------------------------------------------------------ pair update
def pair_inputs(N, F, seed):
    rng = np.random.default_rng(seed)
    W = np.eye(N) + 0.3 * cgauss(rng, (F, N, N))
    A = cgauss(rng, (F, 2, N, 2 * N))
    return W, A @ A.conj().swapaxes(-1, -2) / (2 * N)


def pair_longdouble(W, Upair, pair, flooring):
    """(rows (F, 2, N), relative gap (F,), bar factor (F, 2)) of update_by_ip2_one_pair in longdouble
    (ref: ssspy/bss/_update_spatial_model.py:317-395)."""
    F, N, _ = W.shape
    m, n = pair
    Wl, Ul = W.astype(CLD), Upair.astype(CLD)
    E = np.zeros((F, N, 2), CLD)
    E[:, m, 0] = E[:, n, 1] = 1
    P, PUP, kappa = [], [], []
    for s in range(2):
        WU = Wl @ Ul[:, s]
        Ps, _ = pr.lu_solve(WU, E)
        P.append(Ps)
        PUP.append(lr.herm(np.conj(Ps.swapaxes(-1, -2)) @ Ul[:, s] @ Ps))
        kappa.append(np.linalg.cond((W @ Upair[:, s]).astype(np.complex128)))
    A, B = PUP
    det = (B[:, 0, 0] * B[:, 1, 1] - B[:, 0, 1] * B[:, 1, 0])[:, None, None]
    Binv = np.stack([np.stack([B[:, 1, 1], -B[:, 0, 1]], -1), np.stack([-B[:, 1, 0], B[:, 0, 0]], -1)], -2) / det
    M = Binv @ A  # its eigenvalues are those of A z = lam B z, real and positive
    tr, dt = (M[:, 0, 0] + M[:, 1, 1]).real, (M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]).real
    disc = np.sqrt(np.maximum(tr * tr / 4 - dt, 0))
    lam = np.stack([tr / 2 + disc, tr / 2 - disc], -1)  # h_m: the larger, h_n: the smaller
    gap = (lam[:, 0] - lam[:, 1]) / np.abs(lam).max(axis=-1)
    rows = np.empty((F, 2, N), CLD)
    for k in range(2):
        # an eigenvector of M for lam_k: (M - lam_k) h = 0, from the row of larger entries
        Mk = M - lam[:, k, None, None] * np.eye(2)
        use0 = (np.abs(Mk[:, 0]) ** 2).sum(-1) >= (np.abs(Mk[:, 1]) ** 2).sum(-1)
        r = np.where(use0[:, None], Mk[:, 0], Mk[:, 1])
        h = np.stack([-r[:, 1], r[:, 0]], -1)
        # (eigh2 hands out h^H B h = 1, and the floor acts on the norm of that eigenvector)
        hb = h / np.sqrt(np.einsum("fa,fab,fb->f", np.conj(h), B, h).real)[:, None]
        hUh = np.einsum("fa,fab,fb->f", np.conj(hb), PUP[k], hb).real
        denom = pr.floor(np.sqrt(np.maximum(hUh, 0)), flooring)
        rows[:, k] = np.conj(np.einsum("fab,fb->fa", P[k], hb / denom[:, None]))
    kpair = np.linalg.cond(B.astype(np.complex128))
    factor = np.stack([4 * N * N * kappa[k] + 16 * kpair / gap + 8 * N for k in range(2)], -1)
    return rows, gap, factor


def check_rows(got, ref, factor, phase_free):
    for k in range(2):
        g, r = got[:, k].astype(CLD), ref[:, k].astype(CLD)
        if phase_free:
            inner = np.sum(g * np.conj(r), axis=-1)
            g = g * np.conj(inner / np.abs(inner))[:, None]
        err = np.linalg.norm(g - r, axis=-1)
        bar = 2 * factor[:, k] * U * np.linalg.norm(r, axis=-1)
        assert (err <= bar).all(), (k, float((err / bar).max()))


PAIRS = {N: ((0, 1), (N - 2, N - 1), (N - 1, 0)) for N in (2, 3, 4, 5, 8, 9, 16)}


@pytest.mark.parametrize("N", sorted(PAIRS))
@pytest.mark.parametrize("kind", ["none", "max", "add"])
def test_pair_update(amd, N, kind):
    usm = amd["usm"]
    W, U2 = pair_inputs(N, 3, 100 + N)
    for pair in sorted(set(PAIRS[N])):
        if pair[0] == pair[1]:
            continue
        ref, gap, factor = pair_longdouble(W, U2, pair, FLOORS[kind])
        assert (gap >= 1e-6).all(), "precondition: separated generalised eigenvalues"
        keep = W.copy()
        out = usm.update_by_ip2_one_pair(W, U2, pair, flooring_fn=floor_fn(amd, kind))
        assert out.shape == (3, 2, N) and np.array_equal(W, keep)
        check_rows(out, ref, factor, phase_free=True)
        # the same kernel through update_by_ip2 with that single pair: the same bits
        full = np.zeros((3, N, N, N), complex)
        full[:, pair[0]], full[:, pair[1]] = U2[:, 0], U2[:, 1]
        whole = usm.update_by_ip2(W.copy(), full, flooring_fn=floor_fn(amd, kind),
                                  pair_selector=lambda n_sources: [pair], overwrite=False)
        assert np.array_equal(whole[:, list(pair)], out)
        other = [r for r in range(N) if r not in pair]
        assert np.array_equal(whole[:, other], W[:, other])


@pytest.mark.parametrize("name", ["n2_01", "n3_01", "n3_20", "n4_01", "n4_20", "n9_83"])
@pytest.mark.parametrize("kind", ["max", "add"])
def test_pair_update_fixture(amd, name, kind):
    g = load_golden("surface_ip2_pair_{}_{}".format(name, kind))
    W, U2, pair = g["demix_filter"], g["weighted_covariance_pair"], tuple(int(v) for v in g["pair"])
    _, gap, factor = pair_longdouble(W, U2, pair, FLOORS[kind])
    assert (gap >= 1e-6).all()
    out = amd["usm"].update_by_ip2_one_pair(W, U2, pair, flooring_fn=floor_fn(amd, kind))
    check_rows(out, g["out"], factor, phase_free=False)  # (the phases of LAPACK, as eigh2.hpp restates)


def test_pair_update_singular_raises(amd):
    W, U2 = pair_inputs(3, 3, 7)
    W[1, 2] = 0  # a zero row in one bin: W U is exactly singular in any arithmetic
    with pytest.raises(np.linalg.LinAlgError):
        amd["usm"].update_by_ip2_one_pair(W, U2, (0, 1))


# ------------------------------------------------------------------------------ reconstruction
def psd_basis(rng, shape):
    A = cgauss(rng, shape[:-1] + (shape[-1],))
    return A @ A.conj().swapaxes(-1, -2) / shape[-1]


def check_reconstruction(R, basis, act, flooring, fixture=None):
    """basis (N, K, C, L, L), act (N, K, T), R (N, T, C, L, L)."""
    N, K, C, L, _ = basis.shape
    assert R.shape == (N, act.shape[-1], C, L, L)
    assert np.array_equal(R, np.conj(R.swapaxes(-1, -2))), "not Hermitian to the last bit"
    S = np.einsum("nkcab,nkt->ntcab", basis.astype(CLD), act.astype(LD))
    Sabs = np.einsum("nkcab,nkt->ntcab", np.abs(basis).astype(LD), np.abs(act).astype(LD))
    ref, _ = lr.to_psd(S.reshape(-1, L, L), flooring)
    bar = 2 * U * (lr.C["psd"] * lr.fro(ref) + (K + 1) * lr.fro(Sabs.reshape(-1, L, L)))
    for other in (ref,) if fixture is None else (ref, fixture.reshape(-1, L, L).astype(CLD)):
        err = lr.fro(R.reshape(-1, L, L).astype(CLD) - other)
        assert (err <= bar).all(), float((err / bar).max())
    return ref.reshape(R.shape)


def model(amd, K, C, kind="max", **kw):
    return amd["ipsdta"].GaussIPSDTA(n_basis=K, n_blocks=C, flooring_fn=floor_fn(amd, kind), **kw)


@pytest.mark.parametrize("L", [1, 2, 8])
def test_block_reconstruction_fixture(amd, L):
    g = load_golden("surface_block_psdtf_l{}".format(L))
    m = model(amd, 3, 2)
    R = m.reconstruct_block_decomposition_psdtf(g["basis"], g["activation"])
    check_reconstruction(R, g["basis"], g["activation"], FLOORS["max"], g["out"])
    Rl = m.reconstruct_block_decomposition_psdtf(g["basis_last"], g["activation"], axis1=-3, axis2=-2)
    check_reconstruction(Rl, g["basis"], g["activation"], FLOORS["max"], g["out_last"])
    assert np.array_equal(R, m.reconstruct_block_decomposition_psdtf(g["basis"], g["activation"]))


def test_block_reconstruction_remainder(amd):
    g = load_golden("surface_block_psdtf_rem")
    m = model(amd, 3, 2)
    m.n_bins = int(g["meta_n_bins"])
    out = m.reconstruct_block_decomposition_psdtf((g["basis_low"], g["basis_high"]), g["activation"])
    assert type(out) is tuple and len(out) == 2
    check_reconstruction(out[0], g["basis_low"], g["activation"], FLOORS["max"], g["out_low"])
    check_reconstruction(out[1], g["basis_high"], g["activation"], FLOORS["max"], g["out_high"])


@pytest.mark.parametrize("N,K,T,C,L,kind", [(2, 1, 5, 2, 3, "max"), (2, 32, 5, 2, 4, "add"),
                                            (3, 3, 1, 1, 5, "none"), (2, 3, 70, 3, 7, "max")])
def test_block_reconstruction_shapes(amd, N, K, T, C, L, kind):
    rng = np.random.default_rng(1000 + 10 * K + L)
    basis, act = psd_basis(rng, (N, K, C, L, L)), rng.random((N, K, T))
    R = model(amd, K, C, kind).reconstruct_block_decomposition_psdtf(basis, act)
    check_reconstruction(R, basis, act, FLOORS[kind])


def test_block_reconstruction_floor_acts(amd):
    """One basis of rank 1 and tiny activations elsewhere: L - 1 eigenvalues of R sit below the floor
    1e-10 and come out at it; no matrix and no element is left out of the bar."""
    rng = np.random.default_rng(5)
    N, K, T, C, L = 2, 2, 3, 2, 4
    v = cgauss(rng, (N, K, C, L))
    basis = v[..., :, None] * np.conj(v[..., None, :])
    act = rng.random((N, K, T))
    R = model(amd, K, C).reconstruct_block_decomposition_psdtf(basis, act)
    ref = check_reconstruction(R, basis, act, FLOORS["max"])
    lam = np.linalg.eigvalsh(R)
    assert (np.abs(lam[..., : L - 2] - 1e-10) <= 1e-10 * 1e-3).all() and (lam[..., -1] > 1e-3).all()
    assert (np.linalg.eigvalsh(ref.astype(np.complex128))[..., 0] >= 0.99e-10).all()


def test_full_reconstruction(amd):
    g = load_golden("surface_psdtf_f4")
    m = amd["ipsdta"].IPSDTABase(n_basis=3)
    basis, act = g["basis"], g["activation"]
    R = m.reconstruct_psdtf(basis, act)
    check_reconstruction(R[:, :, None], basis[:, :, None], act, FLOORS["max"], g["out"][:, :, None])
    Rl = m.reconstruct_psdtf(g["basis_last"], act, axis1=-3, axis2=-2)
    check_reconstruction(Rl[:, :, None], basis[:, :, None], act, FLOORS["max"], g["out_last"][:, :, None])
    rng = np.random.default_rng(16)
    basis, act = psd_basis(rng, (2, 2, 16, 16)), rng.random((2, 2, 3))
    R = m.reconstruct_psdtf(basis, act)  # the largest size of the kernel
    check_reconstruction(R[:, :, None], basis[:, :, None], act, FLOORS["max"])


def test_full_reconstruction_host_route(amd):
    """18 bins: the sum on the host, then ssspy_amd.special.to_psd with the sizes it takes -- the
    method does what that function does with the same sum."""
    g = load_golden("surface_psdtf_f18")
    m = amd["ipsdta"].IPSDTABase(n_basis=3)
    S = np.einsum("nkab,nkt->ntab", g["basis"], g["activation"])
    try:
        want = amd["special"].to_psd(S)
    except NotImplementedError:
        with pytest.raises(NotImplementedError):
            m.reconstruct_psdtf(g["basis"], g["activation"])
        return
    R = m.reconstruct_psdtf(g["basis"], g["activation"])
    assert np.array_equal(R, want)
    check_reconstruction(R[:, :, None], g["basis"][:, :, None], g["activation"], FLOORS["max"],
                         g["out"][:, :, None])


def test_reconstruction_reproduces_recorded_loss(amd):
    """After two iterations the handed-out R gives, through y^H R^-1 y + log det R per (source,
    frame, block), the loss the class recorded; the bar of the loss tests of tests/test_gpu_ipsdta.py
    (1e-9 of the largest |loss| of the run)."""
    rng = np.random.default_rng(3)
    N, F, T, K, C = 2, 9, 33, 2, 2
    X = cgauss(rng, (N, F, T))
    m = model(amd, K, C, rng=np.random.default_rng(4), scale_restoration=False)
    Y = m(X, n_iter=2)
    R = m.reconstruct_block_decomposition_psdtf(m.basis, m.activation)
    assert type(R) is tuple
    total, first = np.zeros(T), 0
    for part in R:
        L = part.shape[-1]
        y = Y[:, first:first + part.shape[2] * L].reshape(N, part.shape[2], L, T).transpose(0, 3, 1, 2)
        quad = np.einsum("ntca,ntcab,ntcb->t", np.conj(y), np.linalg.inv(part), y).real
        total += np.maximum(quad, 0) + np.linalg.slogdet(part)[1].sum(axis=(0, 2))
        first += part.shape[2] * L
    loss = total.mean() - 2 * np.linalg.slogdet(m.demix_filter)[1].sum()
    assert abs(loss - m.loss[-1]) <= 1e-9 * np.max(np.abs(m.loss))


# ------------------------------------------------------------------------------ log-determinant
def logdet_longdouble(W):
    """(log|det W|, bar) per matrix by an LU with partial pivoting in longdouble."""
    n, N, _ = W.shape
    out, bar = np.empty(n, LD), np.empty(n, LD)
    for i in range(n):
        A = W[i].astype(CLD)
        Lm, Um, perm = np.eye(N, dtype=CLD), A.copy(), np.arange(N)
        singular = False
        for k in range(N):
            p = k + int(np.argmax(np.abs(Um[k:, k])))
            if Um[p, k] == 0:
                singular = True
                break
            Um[[k, p]], perm[[k, p]] = Um[[p, k]], perm[[p, k]]
            Lm[[k, p], :k] = Lm[[p, k], :k]
            f = Um[k + 1:, k] / Um[k, k]
            Lm[k + 1:, k] = f
            Um[k + 1:] -= f[:, None] * Um[k]
        if singular:
            out[i], bar[i] = -np.inf, 0
            continue
        d = np.abs(np.diag(Um))
        out[i] = np.log(d).sum()
        Ainv = np.linalg.inv(A.astype(np.complex128))  # (a weight of the bar only)
        LU = (np.abs(Lm) @ np.abs(np.triu(Um)))[np.argsort(perm)]
        bar[i] = 2 * U * (4 * N * (np.abs(Ainv).T * LU).sum() + 3 * np.abs(np.log(d)).sum() + N)
    return out, bar


@pytest.mark.parametrize("N", [1, 2, 8, 9, 16])
def test_logdet(amd, N):
    torch, dv, ops = amd["torch"], amd["dv"], amd["ops"]
    from ssspy_amd.bss.ilrma import GaussILRMA
    from ssspy_amd.bss.iva import AuxLaplaceIVA

    rng = np.random.default_rng(40 + N)
    W = cgauss(rng, (2, 35, N, N))
    W[0, 0, 0, 0] = 0            # pivoting needed (N == 1: singular)
    W[1, 4] = 0                  # exactly singular
    W[1, 5, :, -1] = 0           # exactly singular in its last column only
    ref, bar = logdet_longdouble(W.reshape(-1, N, N))
    ref, bar = ref.reshape(2, 35), bar.reshape(2, 35)
    sure = np.isfinite(ref)
    assert not sure[1, 4] and not sure[1, 5] and sure.sum() >= 2 * 35 - 3
    for cls in (GaussILRMA(n_basis=2), AuxLaplaceIVA()):
        dW = dv.to_device(W)
        out = cls.compute_logdet(dW)
        assert torch.is_tensor(out) and out.is_cuda and tuple(out.shape) == (2, 35)
        got = dv.to_host(out)
        assert (np.abs(got[sure] - ref[sure]) <= bar[sure]).all()
        assert (got[~sure] == -np.inf).all()
        one = dv.to_host(cls.compute_logdet(dW[0]))  # unbatched
        assert one.shape == (35,) and np.array_equal(one, got[0], equal_nan=True)
        host = cls.compute_logdet(W)  # the reference's line on the host copy
        assert (np.abs(got[sure] - host[sure]) <= 2 * bar[sure]).all()
    g = load_golden("surface_logdet")
    for key, cls in (("ilrma", GaussILRMA(n_basis=2)), ("iva", AuxLaplaceIVA())):
        Wg = g["W_" + key]
        got = dv.to_host(cls.compute_logdet(dv.to_device(Wg)))
        _, bar = logdet_longdouble(Wg)
        assert (np.abs(got - g["logdet_" + key]) <= 2 * bar).all()


# ------------------------------------------------------------------------------ quadratic
@pytest.mark.parametrize("n", [1, 2, 8, 9, 16])
@pytest.mark.parametrize("lead", [(), (1,), (3, 65)])
def test_quadratic(amd, n, lead):
    dv = amd["dv"]
    rng = np.random.default_rng(50 + n + len(lead))
    X, A = cgauss(rng, lead + (n,)), cgauss(rng, lead + (n, n))
    out = amd["linalg"].quadratic(dv.to_device(X), dv.to_device(A))
    assert out.is_cuda and tuple(out.shape) == lead
    got = dv.to_host(out).astype(CLD)
    ref = np.einsum("...a,...ab,...b->...", np.conj(X.astype(CLD)), A.astype(CLD), X.astype(CLD))
    terms = np.einsum("...a,...ab,...b->...", np.abs(X).astype(LD), np.abs(A).astype(LD), np.abs(X).astype(LD))
    bar = 2 * (2 * n + 6) * U * terms
    assert (np.abs((got - ref).real) <= bar).all() and (np.abs((got - ref).imag) <= bar).all()
    host = amd["linalg"].quadratic(X, A)
    assert (np.abs(got - host) <= 2 * np.sqrt(2) * bar).all()


def test_quadratic_fixture(amd):
    dv = amd["dv"]
    g = load_golden("surface_quadratic")
    got = dv.to_host(amd["linalg"].quadratic(dv.to_device(g["X"]), dv.to_device(g["A"])))
    terms = np.einsum("...a,...ab,...b->...", np.abs(g["X"]), np.abs(g["A"]), np.abs(g["X"]))
    assert (np.abs(got - g["out"]) <= 2 * np.sqrt(2) * (2 * 4 + 6) * U * terms).all()


# ------------------------------------------------------------------------------ softmax, logsumexp
def softmax_longdouble(X, axis):
    Xl = X.astype(LD)
    top = Xl.max(axis=axis, keepdims=True)
    w = np.exp(Xl - top)
    s = w.sum(axis=axis, keepdims=True)
    n = X.shape[axis]
    e = (np.abs(Xl - top) + 3) * U
    E = (w / s * e).sum(axis=axis, keepdims=True) + (n + 2) * U
    soft = w / s
    lse = np.log(s) + top
    return soft, 2 * (e + E + 2 * U) * soft, lse, 2 * (E + 2 * U * np.abs(np.log(s)) + 2 * U * np.abs(lse))


@pytest.mark.parametrize("length", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_softmax_logsumexp(amd, length, axis):
    dv, sp = amd["dv"], amd["special"]
    shape = [3, 5, 2]
    shape[axis] = length
    rng = np.random.default_rng(60 + length + axis)
    X = 4.0 * rng.standard_normal(shape)
    X[0, 0, 0], X[-1, -1, -1] = 700.0, -700.0  # exp(700) * len overflows, exp(-700 - 700) is 0
    dX = dv.to_device(X)
    soft, soft_bar, lse, lse_bar = softmax_longdouble(X, axis)
    out = sp.softmax(dX, axis=axis)
    assert out.is_cuda and tuple(out.shape) == tuple(shape)
    got = dv.to_host(out)
    assert np.isfinite(got).all() and (np.abs(got - soft) <= soft_bar).all()
    assert (np.abs(got.sum(axis=axis) - 1) <= (length + 4) * U).all()
    assert np.array_equal(got, dv.to_host(sp.softmax(dX, axis=axis - 3)))  # two runs, the same bits
    keep = sp.logsumexp(dX, axis=axis, keepdims=True)
    assert tuple(keep.shape) == tuple(lse.shape)
    got = dv.to_host(keep)
    assert np.isfinite(got).all() and (np.abs(got - lse) <= lse_bar).all()
    flat = sp.logsumexp(dX, axis=axis)
    assert tuple(flat.shape) == tuple(np.squeeze(lse, axis=axis).shape)
    assert np.array_equal(dv.to_host(flat), np.squeeze(got, axis=axis))
    host_soft, host_lse = sp.softmax(X, axis=axis), sp.logsumexp(X, axis=axis, keepdims=True)
    assert (np.abs(dv.to_host(out) - host_soft) <= 2 * soft_bar).all()
    assert (np.abs(got - host_lse) <= 2 * lse_bar).all()


def test_softmax_logsumexp_fixture(amd):
    dv, sp = amd["dv"], amd["special"]
    g = load_golden("surface_softmax")
    X = g["X"]
    dX = dv.to_device(X)
    for axis in (0, 1, 2):
        _, soft_bar, _, lse_bar = softmax_longdouble(X, axis)
        assert (np.abs(dv.to_host(sp.softmax(dX, axis=axis)) - g["softmax_{}".format(axis)])
                <= 2 * soft_bar).all()
        assert (np.abs(dv.to_host(sp.logsumexp(dX, axis=axis)) - g["logsumexp_{}".format(axis)])
                <= 2 * np.squeeze(lse_bar, axis=axis)).all()
