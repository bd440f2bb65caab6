"""Extended-precision restatement of the FastGaussMNMF entry points, with error bars.

TEST INFRASTRUCTURE ONLY.  One function per entry point (or per ``steps`` bit of
ssspy_fastmnmf_update) of include/ssspy_amd.h, written from the formula in the header comment and the
reference lines it cites, in ``np.longdouble`` / ``np.clongdouble``; with ``dtype=np.float64`` the SAME
formula runs in plain float64 NumPy (tests/test_mnmf_reference_cpu.py: the bars are attainable).
Nothing here calls into oracle/ or reads the kernels.

Shapes: X (B,M,F,T) c128, Q (B,F,M,M) c128, D (B,F,N,M), basis (B,N,F,K), activation (B,N,K,T),
C (B,F,M,M) c128.  Each function returns ``(value, bar)``, ``bar`` the elementwise absolute error in
the units and by the rules of tests/pass_reference.py.  What FastMNMF adds to them:

* lambda = T V carries K + 1 u; R~_ijm = sum_n lambda_nij d_inm is a positive sum of N such terms:
  N (K + 1) + N u, relative.  Every factor 1 / R~ carries that + 2 (the reciprocal), 1 / R~^2 twice
  that + 3.
* P_mij = |(Q x)_m|^2: 6 M u S |y| + 2 u P, S = sum_c |q_mc| |x_c| (pass_reference.power).  Read from
  the hand-over buffer it was stored once (1 u), is multiplied by pscale (1 u) and pscale = 1 / psi^2
  stands for a division of the rows of Q that the buffer never saw: 3 u on every q_mc, 6 u S |y| in P,
  and the 2 u of a product of two reciprocals -- ``HANDOVER_P``: (6, 4) more u on (S |y|, P).
* a term of the numerator, d P / R~^2: P's budget + 2 R~'s + 3 + 2 products; of the denominator,
  d / R~: R~'s + 2 + 1.  The sum over the M channels adds M, the sums over frames or bins (in any
  grouping: frame splits, bin chunks and their folds included) T + 1 or F + 1.
* the spatial step weighs with lambda instead of d: + K + 1 per term.  No floor, per the reference.
* the normalisation is pass_reference.ilrma_normalize_filter's psi with p = 2 on D.
* the losses are absolute, as ilrma_loss_data: n = M F T terms.
* the diagonaliser step and the Wiener filter are solves and get normwise bars (see the GPU test);
  where the eigenvalue floor of to_psd moves eigenvalues, R_ij is rebuilt from a long-double Jacobi
  eigendecomposition (eigh_jacobi).
"""

import numpy as np

import pass_reference as pr

LD, U = pr.LD, pr.U
BASIS, ACTIVATION, DIAGONALIZER, SPATIAL, NORMALIZE = 1, 2, 4, 8, 16
HANDOVER_P = (6.0, 4.0)
NO_EXTRA = (0.0, 0.0)


def _c(dtype):
    return np.clongdouble if dtype is LD else np.complex128


def rtilde(D, basis, activation, dtype=LD):
    """(lambda (B,N,F,T), R~ (B,M,F,T), relative budget of lambda in u, of R~ in u)."""
    N, K = basis.shape[1], basis.shape[-1]
    lam = np.einsum("bnik,bnkj->bnij", basis.astype(dtype), activation.astype(dtype))
    Rt = np.einsum("bnij,binm->bmij", lam, D.astype(dtype))
    return lam, Rt, K + 1, N * (K + 1) + N


def qx_power(X, Q, dtype=LD, extra=NO_EXTRA):
    """P (B,M,F,T) = |Q x|^2 and its relative budget in u per element (`extra`: see HANDOVER_P)."""
    c = _c(dtype)
    M = X.shape[1]
    Y = np.einsum("binm,bmij->bnij", Q.astype(c), X.astype(c))
    S = np.einsum("binm,bmij->bnij", np.abs(Q.astype(c)), np.abs(X.astype(c)))
    P = np.abs(Y) ** 2
    return P, (6 * M + extra[0]) * S * np.abs(Y) / P + 2 + extra[1]


def handover_buffer(X, Q, dtype=LD):
    """The hand-over as the product P pscale = |Q x|^2 of the CURRENT Q (the split between the two is
    the kernels' choice); bar as read by a pass."""
    P, Prel = qx_power(X, Q, dtype, HANDOVER_P)
    return P, U * P * Prel


def fastmnmf_weights(D, basis, activation, dtype=LD):
    """weights[b,m,i,j] = 1 / R~_ijm."""
    _, Rt, _, rel = rtilde(D, basis, activation, dtype)
    w = 1 / Rt
    return w, U * w * (rel + 2)


def fastmnmf_diagonalizer_covariance(X, D, basis, activation, dtype=LD):
    """U[b,i,m,a,c] = (1/T) sum_j x_a conj(x_c) / R~_ijm; (T + 6) u on the companion
    (1/T) sum_j |x_a| |x_c| / R~ plus the weights' budget."""
    c = _c(dtype)
    w, wbar = fastmnmf_weights(D, basis, activation, dtype)
    T = X.shape[-1]
    Xc = X.astype(c)
    Uo = np.einsum("bmij,baij,bcij->bimac", w.astype(c), Xc, Xc.conj()) / dtype(T)
    ax = np.abs(Xc)
    bar = np.einsum("bmij,baij,bcij->bimac", U * w * (T + 6) + wbar, ax, ax) / dtype(T)
    return Uo, bar


def _terms(X, Q, D, basis, activation, dtype, extra):
    """P / R~^2 and 1 / R~ per (b,m,i,j) with their relative budgets in u, and lambda."""
    lam, Rt, lrel, rel = rtilde(D, basis, activation, dtype)
    P, Prel = qx_power(X, Q, dtype, extra)
    rinv = 1 / Rt
    a = P * rinv * rinv
    return lam, lrel, a, Prel + 2 * rel + 3 + 1, rinv, rel + 2


def update_basis(X, Q, D, basis, activation, flooring, dtype=LD, extra=NO_EXTRA):
    """T <- floor(T sqrt(sum_jm v d P / R~^2 / sum_jm v d / R~))   (mnmf.py:1305-1360)."""
    _, _, a, au, rinv, ru = _terms(X, Q, D, basis, activation, dtype, extra)
    M, T = X.shape[1], X.shape[-1]
    Dd, V = D.astype(dtype), activation.astype(dtype)
    s = np.einsum("binm,bmij->bnij", Dd, a)
    s_eu = np.einsum("binm,bmij->bnij", Dd, a * (au + 1)) + M * s
    r = np.einsum("binm,bmij->bnij", Dd, rinv)
    r_eu = np.einsum("binm,bmij->bnij", Dd, rinv * (ru + 1)) + M * r
    num = np.einsum("bnkj,bnij->bnik", V, s)
    num_eu = (T + 1) * num + np.einsum("bnkj,bnij->bnik", V, s_eu)
    den = np.einsum("bnkj,bnij->bnik", V, r)
    den_eu = (T + 1) * den + np.einsum("bnkj,bnij->bnik", V, r_eu)
    return pr._finish(num, num_eu, den, den_eu, dtype(0.5), basis, flooring, dtype)


def update_activation(X, Q, D, basis, activation, flooring, dtype=LD, extra=NO_EXTRA):
    """V <- floor(V sqrt(sum_im t d P / R~^2 / sum_im t d / R~))   (mnmf.py:1362-1417)."""
    _, _, a, au, rinv, ru = _terms(X, Q, D, basis, activation, dtype, extra)
    M, F = X.shape[1], X.shape[2]
    Dd, Tm = D.astype(dtype), basis.astype(dtype)
    s = np.einsum("binm,bmij->bnij", Dd, a)
    s_eu = np.einsum("binm,bmij->bnij", Dd, a * (au + 1)) + M * s
    r = np.einsum("binm,bmij->bnij", Dd, rinv)
    r_eu = np.einsum("binm,bmij->bnij", Dd, rinv * (ru + 1)) + M * r
    num = np.einsum("bnik,bnij->bnkj", Tm, s)
    num_eu = (F + 1) * num + np.einsum("bnik,bnij->bnkj", Tm, s_eu)
    den = np.einsum("bnik,bnij->bnkj", Tm, r)
    den_eu = (F + 1) * den + np.einsum("bnik,bnij->bnkj", Tm, r_eu)
    return pr._finish(num, num_eu, den, den_eu, dtype(0.5), activation, flooring, dtype)


def update_spatial(X, Q, D, basis, activation, dtype=LD):
    """d_inm <- d_inm sqrt(sum_j lambda P / R~^2 / sum_j lambda / R~), no floor (mnmf.py:1635-1675)."""
    lam, lrel, a, au, rinv, ru = _terms(X, Q, D, basis, activation, dtype, NO_EXTRA)
    T = X.shape[-1]
    num = np.einsum("bnij,bmij->binm", lam, a)
    num_eu = (T + 1) * num + np.einsum("bnij,bmij->binm", lam, a * (au + lrel + 1))
    den = np.einsum("bnij,bmij->binm", lam, rinv)
    den_eu = (T + 1) * den + np.einsum("bnij,bmij->binm", lam, rinv * (ru + lrel + 1))
    return pr._finish(num, num_eu, den, den_eu, dtype(0.5), D, (pr.FLOOR_NONE, 0.0), dtype)


def normalize(Q, C, D, flooring, dtype=LD, D_rel_u=None):
    """psi_m = floor(sqrt((1/F) sum_i q_im^H C_i q_im)), Q <- Q / psi (rows), D <- D / psi^2
    (mnmf.py:632-678).  D_rel_u: the relative error D already carries (SPATIAL | NORMALIZE in one
    call).  Returns (Q, bar on |dQ|, D, bar_D, psi)."""
    B, F, M, _ = Q.shape
    dummy = np.ones((B, M, 1, 1))
    Qn, barQ, _, _, psi, rel = pr.ilrma_normalize_filter(Q, C, dummy, 2.0, flooring, dtype)
    Dd = D.astype(dtype)
    Dn = Dd / (psi ** 2)[:, None, None, :]
    own = 0 if D_rel_u is None else D_rel_u
    barD = U * Dn * (own + (2 * rel + 2 + 3)[:, None, None, :])
    return Qn, barQ, Dn, barD, psi


def loss_data(X, Q, D, basis, activation, dtype=LD, extra=NO_EXTRA):
    """out[b] = sum_i mean_j sum_m (P / R~ + log R~)   (mnmf.py:1240-1258), absolute bar."""
    _, Rt, _, rel = rtilde(D, basis, activation, dtype)
    P, Prel = qx_power(X, Q, dtype, extra)
    B, M, F, T = P.shape
    n = M * F * T
    data, du = P / Rt, Prel + rel + 2 + 1
    logR = np.log(Rt)
    ax = (1, 2, 3)
    val = (data.sum(axis=ax) + logR.sum(axis=ax)) / dtype(T)
    bar = U * ((n * data + data * du).sum(axis=ax)
               + (n + 4) * np.maximum(1, np.abs(logR).sum(axis=ax)) + n * rel) / dtype(T)
    return val, bar


def update_diagonalizer(X, Q, D, basis, activation, flooring, dtype=LD):
    """IP1 on the covariances above (mnmf.py:1449-1514): (Q_new, kappa (B,F) or None)."""
    Uc, _ = fastmnmf_diagonalizer_covariance(X, D, basis, activation, dtype)
    if dtype is LD:
        return pr.update_by_ip1(Q, Uc, flooring)
    return pr.update_by_ip1_float64(Q, np.ascontiguousarray(Uc), flooring), None


def ip1_yardstick(X, Q, D, basis, activation, flooring):
    """The float64 sweep (np.linalg.solve) fed the extended reference's own U, rounded once to
    complex128: what `c` of the normwise IP1 bar is 8 x the kappa-normalised error of."""
    Uc, _ = fastmnmf_diagonalizer_covariance(X, D, basis, activation, LD)
    return pr.update_by_ip1_float64(Q, np.ascontiguousarray(Uc.astype(np.complex128)), flooring)


def update_once(X, C, Q, D, basis, activation, flooring, normalization=True, dtype=LD):
    """update_once() in the reference's order (mnmf.py:1278-1303); values only."""
    b1, _ = update_basis(X, Q, D, basis, activation, flooring, dtype)
    a1, _ = update_activation(X, Q, D, b1, activation, flooring, dtype)
    Q1, _ = update_diagonalizer(X, Q, D, b1, a1, flooring, dtype)
    D1, _ = update_spatial(X, Q1, D, b1, a1, dtype)
    if normalization:
        Q1, _, D1, _, _ = normalize(Q1, C, D1, flooring, dtype)
    return Q1, D1, b1, a1


# ---------------------------------------------------------------------------------- Wiener filter
def eigh_jacobi(A, sweeps=10):
    """Eigendecomposition of a stack of Hermitian matrices A (n,M,M) in the dtype of A by cyclic
    Jacobi rotations (quadratically convergent; 10 sweeps reach the precision of the dtype for
    M <= 16): returns (w (n,M) unsorted, V (n,M,M)) with A = V diag(w) V^H."""
    A = A.copy()
    n, M, _ = A.shape
    rdt = A.real.dtype
    V = np.broadcast_to(np.eye(M, dtype=A.dtype), A.shape).copy()
    for _ in range(sweeps):
        for p in range(M - 1):
            for q in range(p + 1, M):
                apq = A[:, p, q]
                b = np.abs(apq)
                nz = b > 0
                bs = np.where(nz, b, 1)
                ph = np.where(nz, apq / bs, 1)          # e^{i phi}
                tau = (A[:, q, q].real - A[:, p, p].real) / (2 * bs)
                t = np.where(tau >= 0, 1, -1) / (np.abs(tau) + np.sqrt(1 + tau * tau))
                t = np.where(nz, t, rdt.type(0))
                c = 1 / np.sqrt(1 + t * t)
                sn = t * c
                # J = diag(.., e^{-i phi} at q) R(c, s): columns p, q of A J and V J, then rows of J^H A
                for Mx in (A, V):
                    cp, cq = Mx[:, :, p].copy(), Mx[:, :, q].copy() * ph.conj()[:, None]
                    Mx[:, :, p] = c[:, None] * cp - sn[:, None] * cq
                    Mx[:, :, q] = sn[:, None] * cp + c[:, None] * cq
                rp, rq = A[:, p, :].copy(), A[:, q, :].copy() * ph[:, None]
                A[:, p, :] = c[:, None] * rp - sn[:, None] * rq
                A[:, q, :] = sn[:, None] * rp + c[:, None] * rq
    return np.einsum("nmm->nm", A).real.copy(), V


def separate(X, Q, D, basis, activation, reference_id, flooring, dtype=LD, eig=False):
    """The multichannel Wiener filter (mnmf.py:1174-1217): R_n = Q^-1 diag(lambda_n d_n) Q^-H,
    R = to_psd(sum_n R_n), y_n = (R_n R^-1 x)_ref, by elimination in `dtype`.  to_psd
    (special/psd.py:11-71) floors the eigenvalues of R: with eig=False it is taken as the identity
    (MAX or NONE, for the caller to assert on the returned smallest eigenvalue that the floor is
    inactive) or as R + eps I (ADD); with eig=True R is rebuilt from eigh_jacobi with floored
    eigenvalues, whatever share of them the floor moves.  Returns (Y (B,N,F,T), kappa_2 of the floored
    R_ij (B,F,T), eigenvalues of the UNFLOORED R_ij: the smallest (B,F,T), or all (B,F,T,M) with
    eig=True)."""
    c = _c(dtype)
    B, M, F, T = X.shape
    lam, Rt, _, _ = rtilde(D, basis, activation, dtype)
    Qc = Q.astype(c).reshape(B * F, M, M)
    Qi = pr.lu_solve(Qc, np.broadcast_to(np.eye(M, dtype=c), Qc.shape).copy())[0].reshape(B, F, M, M)
    g = np.einsum("bnij,binm->bnijm", lam, D.astype(dtype)).astype(c)
    Rn = np.einsum("biam,bnijm,bicm->bnijac", Qi, g, Qi.conj())
    R = Rn.sum(axis=1)
    raw = None
    if eig:
        Rh = (R + np.swapaxes(R, -1, -2).conj()) / 2
        raw, V = eigh_jacobi(Rh.reshape(B * F * T, M, M))
        wf = pr.floor(raw, flooring)
        R = np.einsum("nam,nm,ncm->nac", V, wf.astype(c), V.conj()).reshape(B, F, T, M, M)
        raw = raw.reshape(B, F, T, M)
    elif flooring[0] == pr.FLOOR_ADD:
        R = R + dtype(flooring[1]) * np.eye(M, dtype=c)
    rhs = np.moveaxis(X.astype(c), 1, -1).reshape(B * F * T, M, 1)
    z = pr.lu_solve(R.reshape(B * F * T, M, M), rhs)[0].reshape(B, F, T, M)
    Y = np.einsum("bnijm,bijm->bnij", Rn[..., reference_id, :], z)
    ev = np.linalg.eigvalsh(R.astype(np.complex128))
    return Y, ev[..., -1] / ev[..., 0], (ev[..., 0] if raw is None else raw)


def separate_float64(X, Q, D, basis, activation, reference_id, flooring):
    """The filter as the reference composes it, in float64 NumPy: R_n = Q^-1 diag(lambda_n d_n) Q^-H,
    R = to_psd(sum_n R_n) (eigh, floored eigenvalues, rebuilt: special/psd.py:11-71),
    W_n = (R^-1 R_n)^H, y_n = (W_n x)_ref.  The yardstick of the normwise bar, and the only form that
    knows the eigenvalue floor.  Returns Y (B,N,F,T)."""
    lam = np.einsum("bnik,bnkj->bnij", basis, activation)
    Qi = np.linalg.inv(Q)                                                      # (B,F,M,M)
    g = np.einsum("bnij,binm->bnijm", lam, D)                                  # (B,N,F,T,M)
    Rn = np.einsum("biam,bnijm,bicm->bnijac", Qi, g, Qi.conj())
    R = Rn.sum(axis=1)
    R = (R + np.swapaxes(R, -1, -2).conj()) / 2
    w, V = np.linalg.eigh(R)
    w = pr.floor(w, flooring)
    R = np.einsum("bijam,bijm,bijcm->bijac", V, w, V.conj())
    WH = np.linalg.solve(R[:, None], Rn)                                       # R^-1 R_n
    W = np.swapaxes(WH, -1, -2).conj()
    return np.einsum("bnijm,bmij->bnij", W[..., reference_id, :], X)


def separate_error(Ya, Yref, X, kappa):
    """max over (b,i,j) of ||y - y_ref||_(over n) / (kappa_ij u ||x_ij||)."""
    num = np.linalg.norm((Ya.astype(np.clongdouble) - Yref).astype(np.complex128), axis=1)
    den = np.linalg.norm(X, axis=1) * kappa * U
    return float(np.max(num / den))


# ---------------------------------------------------------------------------------- generators
def gen_state(seed, B, N, M, F, T, K):
    """(X, C, Q, D, basis, activation) of moderate dynamic range, as pass_reference.gen_fused_inputs:
    unit-variance columns with per-element magnitudes over 1/2..2, every positive factor over
    2^-1..2^1, diagonalisers with rows over 2^-1..2^1 (so that kappa(Q U_m) stays below 1e3) and
    C = (1/T) sum_j x x^H in float64."""
    rng = np.random.default_rng(seed + 11)
    X = (rng.standard_normal((B, M, F, T)) + 1j * rng.standard_normal((B, M, F, T))) \
        * pr._log_uniform(rng, -1, 1, (B, M, F, T))
    basis = pr._log_uniform(rng, -1, 1, (B, N, F, K))
    act = pr._log_uniform(rng, -1, 1, (B, N, K, T))
    D = pr._log_uniform(rng, -1, 1, (B, F, N, M))
    Q = pr.gen_filters(seed, B, F, M, log2_range=1)
    C = np.asarray(pr.cross_covariance(X, X)[0], dtype=np.complex128)
    return X, C, Q, D, basis, act


def gen_floor_state(seed, B, N, M, F, T, K, eps=pr.EPS):
    """The same with (basis, activation) over eps 2^-6..eps 2^6 (a few exactly eps) and X scaled so
    that |Q x|^2 is of the order of R~: the updated values straddle eps."""
    X, C, Q, D, _, _ = gen_state(seed, B, N, M, F, T, K)
    basis, act = pr.gen_floor_nmf(seed, B, N, F, T, K, eps)
    s = eps * np.sqrt(N * K)
    return X * s, C * s * s, Q, D, basis, act


def gen_floor_rows(Q, C, eps=pr.EPS):
    """Q with the rows of even (b M + m) scaled so that psi_m = eps / 16 (floored) and the others so
    that psi_m = 16 eps: returns (Q, floored (B,M) bool)."""
    B, F, M, _ = Q.shape
    q = np.einsum("bink,bikl,binl->bin", Q, C, Q.conj()).real.mean(axis=1)
    even = (np.arange(B * M).reshape(B, M) % 2) == 0
    target = np.where(even, eps / 16, 16 * eps)
    return Q * (target / np.sqrt(q))[:, None, :, None], even


def gen_wiener_floor_state(seed, B, N, M, F, T, K, eps):
    """gen_state with D scaled so that the median eigenvalue of R_ij is eps: the MAX floor of to_psd
    moves about half of the eigenvalues (the caller asserts the share on the reference)."""
    X, C, Q, D, basis, act = gen_state(seed, B, N, M, F, T, K)
    lam = np.einsum("bnik,bnkj->bnij", basis, act)
    Qi = np.linalg.inv(Q)
    R = np.einsum("biam,bnij,binm,bicm->bijac", Qi, lam, D, Qi.conj())
    med = float(np.median(np.linalg.eigvalsh(R)))
    return X, C, Q, D * (eps / med), basis, act
