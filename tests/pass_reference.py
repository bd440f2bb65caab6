"""Extended-precision restatement of the ILRMA / AuxIVA hot-path entry points, with error bars.

TEST INFRASTRUCTURE ONLY.  One function per entry point of include/ssspy_amd.h, written from the
formula in the header comment (and the reference lines it cites) in ``np.longdouble`` /
``np.clongdouble`` (x87 extended: 64 mantissa bits, eps = 1.08e-19).  Every function takes
``dtype``: with ``np.float64`` the SAME formula is evaluated in plain float64 NumPy, which is what
tests/test_pass_reference_cpu.py uses to show that the bars are attainable.

Each function returns ``(value, bar)``: ``bar`` is the elementwise absolute error a float64
evaluation of the formula may make, ``m * u * companion`` with ``u = 2**-53``, composed from
first-order rounding analysis:

* a sum of n terms in any order (MFMA accumulation, frame splits, chunk and slot folds): n u times
  the sum of the magnitudes (the sum itself where all terms are positive);
* R = (T V): K terms, so a factor R^-s carries s (K + 1) u (K adds, one product rounding);
* a division, a square root, a Newton reciprocal (rcp_nr) or root (sqrt_nr): 2 u each;
* a power through exp2(e log2 x): (2 |e log2 x| + 4) u (two roundings inside an exponent of that
  size, plus the two functions); a correctly rounded pow(): 2 u, plus |e ln x| u where float64
  cannot hold e exactly (a rounded quotient such as 2 / p: its u moves x^e by that much; nothing
  is added for an exact exponent) -- ``fast_pow`` selects;
* the ratio num / den raised to `expo`: expo (rel num + rel den + 2) + 2 u (+ |expo ln ratio| u
  for an exponent other than 1/2 or 1, as above);
* y = W x: each component is 2 N products summed, 2 N u sum_m |w_nm| |x_m| per component,
  3 N u S in modulus (S = sum_m |w_nm| |x_m|); |y|^2 then carries (6 N) u S |y| + 2 u |y|^2;
* the MAX and ADD floors are 1-Lipschitz: the bar of the floored value is that of its argument
  (plus 1 u for ADD's addition).

Nothing here calls into oracle/ or reads the kernels.
"""

import numpy as np

LD = np.longdouble
U = float(2.0 ** -53)
FLOOR_NONE, FLOOR_MAX, FLOOR_ADD = 0, 1, 2
GAUSS, TMODEL, GGD, ME = 0, 1, 2, 0x100
EPS = 1e-10


def _c(dtype):
    return np.clongdouble if dtype is LD else np.complex128


def floor(x, flooring):
    kind, eps = flooring
    if kind == FLOOR_MAX:
        return np.maximum(x, x.dtype.type(eps))
    if kind == FLOOR_ADD:
        return x + x.dtype.type(eps)
    return x


def _pow(x, e, dtype, fast_pow):
    """x**e and its rounding budget in u (array).  float64 evaluates the form the kernels use."""
    x = np.asarray(x, dtype=dtype)
    e = dtype(e)
    if e == 1:
        return x, np.zeros(x.shape, dtype)
    if e == -1:
        return 1 / x, np.full(x.shape, 2, dtype)
    if e in (2, -2, 3, -3):  # products of a reciprocal: 2 u for it, 1 u per product
        v = x ** int(e)
        return v, np.full(x.shape, (2 if e < 0 else 0) + abs(int(e)) - 1, dtype)
    if e == dtype(0.5):
        return np.sqrt(x), np.full(x.shape, 2, dtype)
    if e == dtype(0.25):
        return np.sqrt(np.sqrt(x)), np.full(x.shape, 3, dtype)
    if fast_pow:
        l2 = np.log2(x)
        v = np.exp2(e * l2) if dtype is not LD else x ** e
        return v, 2 * np.abs(e * l2) + 4
    # a correctly rounded pow(): 2 u; an exponent that float64 cannot hold exactly (2 / p, ...) is
    # itself rounded, and its u moves x^e by |e ln x| u
    exact = LD(np.float64(e)) == LD(e)
    return x ** e, 2 + (0 if exact else np.abs(e * np.log(x)))


# ---------------------------------------------------------------------------------- shared operators
def separate(X, W, dtype=LD):
    """Y[b,n,i,j] = sum_m W[b,i,n,m] X[b,m,i,j]; bar on |dY| = 3 N u S, S = sum_m |W| |X|."""
    c = _c(dtype)
    N = X.shape[1]
    Y = np.einsum("binm,bmij->bnij", W.astype(c), X.astype(c))
    S = np.einsum("binm,bmij->bnij", np.abs(W.astype(c)), np.abs(X.astype(c)))
    return Y, 3 * N * U * S


def power(X, W=None, dtype=LD):
    """P = |y|^2, y = W x (or x), and its bar: 6 N u S |y| + 2 u P (2 u P without a filter)."""
    c = _c(dtype)
    if W is None:
        P = np.abs(X.astype(c)) ** 2
        return P, 2 * U * P
    N = X.shape[1]
    Y = np.einsum("binm,bmij->bnij", W.astype(c), X.astype(c))
    S = np.einsum("binm,bmij->bnij", np.abs(W.astype(c)), np.abs(X.astype(c)))
    P = np.abs(Y) ** 2
    return P, U * (6 * N * S * np.abs(Y) + 2 * P)


def weighted_covariance(A, weight, kind, S, dtype=LD):
    """U[b,i,s,a,c] = (1/T) sum_j w x_a conj(x_c); companion A_ac = (1/T) sum_j w |x_a| |x_c|.
    m = T + 6: T for the sum, 4 for a weighted complex product in modulus, 2 for the 1/T."""
    c = _c(dtype)
    B, N, F, T = A.shape
    Ac = A.astype(c)
    if kind == 0:
        w = np.ones((B, S, F, T), dtype)
    elif kind == 1:
        w = np.broadcast_to(weight.astype(dtype)[:, :, None, :], (B, S, F, T))
    else:
        w = weight.astype(dtype)
    Uo = np.einsum("bsij,baij,bcij->bisac", w.astype(c), Ac, Ac.conj()) / dtype(T)
    comp = np.einsum("bsij,baij,bcij->bisac", w, np.abs(Ac), np.abs(Ac)) / dtype(T)
    return Uo, (T + 6) * U * comp


def cross_covariance(A, Bm, dtype=LD):
    """C[b,i,a,c] = (1/T) sum_j A_a conj(Bm_c); m = T + 5."""
    c = _c(dtype)
    T = A.shape[-1]
    Ac, Bc = A.astype(c), Bm.astype(c)
    C = np.einsum("baij,bcij->biac", Ac, Bc.conj()) / dtype(T)
    comp = np.einsum("baij,bcij->biac", np.abs(Ac), np.abs(Bc)) / dtype(T)
    return C, (T + 5) * U * comp


def covariance_congruence(C, G, dtype=LD):
    """Cout = G C G^H per bin and set; two complex dot products in a row: m = 6 N + 2 on
    sum_kl |g_ak| |c_kl| |g_cl|.  C (B,F,N,N) or (B,F,S,N,N)."""
    c = _c(dtype)
    N = G.shape[-1]
    Cc, Gc = C.astype(c), G.astype(c)
    if C.ndim == 4:
        out = np.einsum("biak,bikl,bicl->biac", Gc, Cc, Gc.conj())
        comp = np.einsum("biak,bikl,bicl->biac", np.abs(Gc), np.abs(Cc), np.abs(Gc))
    else:
        out = np.einsum("biak,biskl,bicl->bisac", Gc, Cc, Gc.conj())
        comp = np.einsum("biak,biskl,bicl->bisac", np.abs(Gc), np.abs(Cc), np.abs(Gc))
    return out, (6 * N + 2) * U * comp


def compose_filters(G, W, dtype=LD):
    """out = G W per bin; m = 3 N on sum_k |g_ak| |w_kc|."""
    c = _c(dtype)
    N = G.shape[-1]
    out = np.einsum("biak,bikc->biac", G.astype(c), W.astype(c))
    comp = np.einsum("biak,bikc->biac", np.abs(G.astype(c)), np.abs(W.astype(c)))
    return out, 3 * N * U * comp


def lu_solve(A, Bm):
    """Batched Gaussian elimination with partial pivoting in the dtype of A (NumPy's LAPACK wrappers
    have no extended precision).  A (n,N,N), Bm (n,N,r) -> X (n,N,r), det (n,)."""
    A = A.copy()
    X = Bm.copy()
    n, N, _ = A.shape
    idx = np.arange(n)
    det = np.ones(n, A.dtype)
    for k in range(N):
        piv = k + np.argmax(np.abs(A[:, k:, k]), axis=1)
        swap = piv != k
        rk, rp = A[idx, k].copy(), A[idx, piv].copy()
        A[idx, k], A[idx, piv] = rp, rk
        xk, xp = X[idx, k].copy(), X[idx, piv].copy()
        X[idx, k], X[idx, piv] = xp, xk
        det = det * np.where(swap, -1, 1) * A[:, k, k]
        f = A[:, k + 1:, k] / A[:, k, k][:, None]
        A[:, k + 1:, :] -= f[:, :, None] * A[:, k, :][:, None, :]
        X[:, k + 1:, :] -= f[:, :, None] * X[:, k, :][:, None, :]
    for k in range(N - 1, -1, -1):
        X[:, k, :] = (X[:, k, :] - np.einsum("nm,nmr->nr", A[:, k, k + 1:], X[:, k + 1:, :])) \
            / A[:, k, k][:, None]
    return X, det


def sum_logdet(W, dtype=LD):
    """out[b] = sum_i log|det W_i| (absolute bar).  An LU leaves det(W + dW), |dW| <= N u |L||U|,
    so log|det| moves by at most N u || |W^-1| |L||U| ||, bounded here by 3 N^2 u skeel_i with
    skeel_i = || |W_i^-1| |W_i| ||_inf (row-scaling invariant) and the factor 3 N for |L||U| against
    |W|; the F logs and their sum add (F + 4) u max(1, sum |log|det||)."""
    c = _c(dtype)
    B, F, N, _ = W.shape
    Wc = W.astype(c).reshape(B * F, N, N)
    eye = np.broadcast_to(np.eye(N, dtype=c), Wc.shape).copy()
    Winv, det = lu_solve(Wc, eye)
    ld = np.log(np.abs(det)).reshape(B, F)
    skeel = np.max(np.sum(np.einsum("nab,nbc->nac", np.abs(Winv), np.abs(Wc)), axis=-1), axis=-1)
    bar = U * (3 * N * N * skeel.reshape(B, F).sum(axis=1)
               + (F + 4) * np.maximum(1, np.abs(ld).sum(axis=1)))
    return ld.sum(axis=1), bar


def fold_scalar_slots(slots, dtype=LD):
    """out[e] = sum_s slots[s, e]; m = nslots on sum_s |slots|."""
    s = slots.astype(dtype)
    return s.sum(axis=0), slots.shape[0] * U * np.abs(s).sum(axis=0)


# ---------------------------------------------------------------------------------- ILRMA passes
def _model(model):
    return model[0] & 0xff, bool(model[0] & ME), model[1]


def _tv(basis, activation, dtype, basis_rel_u=0.0):
    """R = T V and its relative budget in u: K + 1 (+ what the inputs already carry)."""
    K = basis.shape[-1]
    R = np.einsum("bnik,bnkj->bnij", basis.astype(dtype), activation.astype(dtype))
    return R, K + 1 + basis_rel_u


def _mm_terms(P, Prel, R, Rrel, domain, model, dtype, fast_pow):
    """numerator factor a, 1 / R, their relative budgets in u, and the exponent of the ratio.
    GAUSS a = P / R^((p+2)/p); T a = P / (R~ R), R~ = nu/(nu+2) R^(2/p) + 2/(nu+2) P;
    GGD a = (beta/2) P^(beta/2) / R^((beta+p)/p)."""
    kind, me, param = _model(model)
    p = dtype(domain)
    rinv, rinv_u = 1 / R, Rrel + 2
    if kind == GAUSS:
        e = -(p + 2) / p
        f, fu = _pow(R, e, dtype, fast_pow)
        a, au = P * f, Prel + abs(e) * Rrel + fu + 1
        expo = p / (p + 2)
    elif kind == TMODEL:
        nu = dtype(param)
        w = nu / (nu + 2)
        f, fu = _pow(R, 2 / p, dtype, fast_pow)
        Rt = w * f + (1 - w) * P
        # R~ is a positive combination: its relative error is at most the larger of its terms' (+ 3)
        a = P / (Rt * R)
        au = Prel + 2 * Rrel * max(1, float(2 / p)) + fu + 3 + 2 + 2 + 2
        expo = p / (p + 2)
    else:
        beta = dtype(param)
        if p == 2:  # (P / R)^(beta/2) / R, the form that needs one power
            f, fu = _pow(P * rinv, beta / 2, dtype, fast_pow)
            a = (beta / 2) * f * rinv
            au = (beta / 2) * (Prel + rinv_u + 1) + fu + rinv_u + 2
        else:
            f1, f1u = _pow(P, beta / 2, dtype, fast_pow)
            f2, f2u = _pow(R, -(beta + p) / p, dtype, fast_pow)
            a = (beta / 2) * f1 * f2
            au = (beta / 2) * Prel + f1u + (beta + p) / p * Rrel + f2u + 2
        expo = p / (beta + p)
    if me:
        expo = dtype(1)
    return a, au, rinv, rinv_u, expo


def _finish(num, num_eu, den, den_eu, expo, old, flooring, dtype):
    """floor(old * (num / den)^expo) and its bar; *_eu: absolute error budgets in u."""
    rel = num_eu / num + den_eu / den + 2
    ratio = num / den
    eu = 0
    if expo == dtype(0.5):
        g = np.sqrt(ratio)
    elif expo == 1:
        g = ratio
    else:
        g = ratio ** expo
        eu = 0 if LD(np.float64(expo)) == LD(expo) else np.abs(expo * np.log(ratio))
    pre = old.astype(dtype) * g
    out = floor(pre, flooring)
    # (the ADD floor's own addition rounds relative to its result, not to its argument)
    bar = U * pre * (expo * rel + eu + 2 + 1) + (U * out if flooring[0] == FLOOR_ADD else 0)
    return out, bar


def ilrma_update_basis(X, W, basis, activation, domain, model, flooring, dtype=LD, fast_pow=True):
    """T <- floor(T (sum_j V a / sum_j V / R)^expo); sums of n = T terms."""
    P, Pbar = power(X, W, dtype)
    Prel = Pbar / (U * P)
    R, Rrel = _tv(basis, activation, dtype)
    a, au, rinv, ru, expo = _mm_terms(P, Prel, R, Rrel, domain, model, dtype, fast_pow)
    V = activation.astype(dtype)
    T = X.shape[-1]
    num = np.einsum("bnkj,bnij->bnik", V, a)
    num_eu = (T + 1) * num + np.einsum("bnkj,bnij->bnik", V, a * au)
    den = np.einsum("bnkj,bnij->bnik", V, rinv)
    den_eu = (T + 1) * den + np.einsum("bnkj,bnij->bnik", V, rinv * ru)
    return _finish(num, num_eu, den, den_eu, expo, basis, flooring, dtype)


def ilrma_update_activation(X, W, basis, activation, domain, model, flooring, dtype=LD,
                            fast_pow=True, basis_rel_u=0.0):
    """V <- floor(V (sum_i T a / sum_i T / R)^expo) with the basis given (the NEW one in an
    iteration); sums of n = F terms.  basis_rel_u: relative error the given basis already carries
    (the fused update hands over its own new basis), in u."""
    P, Pbar = power(X, W, dtype)
    Prel = Pbar / (U * P)
    R, Rrel = _tv(basis, activation, dtype, basis_rel_u)
    a, au, rinv, ru, expo = _mm_terms(P, Prel, R, Rrel, domain, model, dtype, fast_pow)
    Tm = basis.astype(dtype)
    F = X.shape[2]
    num = np.einsum("bnik,bnij->bnkj", Tm, a)
    num_eu = (F + 1 + basis_rel_u) * num + np.einsum("bnik,bnij->bnkj", Tm, a * au)
    den = np.einsum("bnik,bnij->bnkj", Tm, rinv)
    den_eu = (F + 1 + basis_rel_u) * den + np.einsum("bnik,bnij->bnkj", Tm, rinv * ru)
    return _finish(num, num_eu, den, den_eu, expo, activation, flooring, dtype)


def ilrma_weight(P, Prel, basis, activation, domain, model, flooring, dtype=LD, fast_pow=True,
                 basis_rel_u=0.0):
    """varphi = 1 / R~ per (b,n,i,j) and its relative budget in u:
    GAUSS 1 / R^(2/p); T 1 / (nu/(nu+2) R^(2/p) + 2/(nu+2) P);
    GGD 1 / ((2/beta) floor(P^((2-beta)/2)) R^(beta/p))."""
    kind, _, param = _model(model)
    p = dtype(domain)
    R, Rrel = _tv(basis, activation, dtype, basis_rel_u)
    if kind == GAUSS:
        f, fu = _pow(R, -2 / p, dtype, fast_pow)
        return f, (2 / p) * Rrel + fu
    if kind == TMODEL:
        nu = dtype(param)
        w = nu / (nu + 2)
        f, fu = _pow(R, 2 / p, dtype, fast_pow)
        return 1 / (w * f + (1 - w) * P), np.maximum((2 / p) * Rrel + fu, Prel) + 3 + 2
    beta = dtype(param)
    q, qu = _pow(P, (2 - beta) / 2, dtype, fast_pow)
    f, fu = _pow(R, beta / p, dtype, fast_pow)
    den = (2 / beta) * floor(q, flooring) * f
    return 1 / den, (2 - beta) / 2 * Prel + qu + 1 + (beta / p) * Rrel + fu + 2 + 2


def ilrma_iss_weight(Y, basis, activation, domain, model, flooring, dtype=LD, Ypow=None):
    """varphi (B,N,F,T) from the separated spectrogram, or from its power Ypow = |y|^2."""
    if Ypow is not None:
        P = Ypow.astype(dtype)
        Prel = np.zeros(P.shape, dtype)
    else:
        P, Pbar = power(Y, None, dtype)
        Prel = Pbar / (U * P)
    v, vu = ilrma_weight(P, Prel, basis, activation, domain, model, flooring, dtype, False)
    return v, U * v * vu


def ilrma_weighted_covariance(X, W, basis, activation, domain, model, flooring, dtype=LD,
                              fast_pow=True, basis_rel_u=0.0):
    """U[b,i,n] = (1/T) sum_j varphi_nij x x^H; bar on the modulus against
    A_ac = (1/T) sum_j varphi |x_a| |x_c|: (T + 6) u A plus the weights' own budgets."""
    c = _c(dtype)
    kind, _, _ = _model(model)
    if kind == GAUSS:
        P = Prel = np.zeros((), dtype)
    else:
        P, Pbar = power(X, W, dtype)
        Prel = Pbar / (U * P)
    v, vu = ilrma_weight(P, Prel, basis, activation, domain, model, flooring, dtype, fast_pow,
                         basis_rel_u)
    T = X.shape[-1]
    Xc = X.astype(c)
    Uo = np.einsum("bnij,baij,bcij->binac", v.astype(c), Xc, Xc.conj()) / dtype(T)
    ax = np.abs(Xc)
    bar = U * np.einsum("bnij,baij,bcij->binac", v * (T + 6 + vu), ax, ax) / dtype(T)
    return Uo, bar


def ilrma_loss_data(X, W, basis, activation, domain, model, dtype=LD, fast_pow=True):
    """out[b] = sum_{n,i} mean_j (data term + (2/p) log R) (absolute bar).  n = N F T terms:
    data part (n + budget) u sum data / T; log part (2/p)/T ((n + 4) max(1, sum |log R|) + n (K+1)) u
    -- the (K + 1) u relative error of R moves each log by that much absolutely."""
    kind, _, param = _model(model)
    p = dtype(domain)
    P, Pbar = power(X, W, dtype)
    Prel = Pbar / (U * P)
    R, Rrel = _tv(basis, activation, dtype)
    B, N, F, T = P.shape
    n = N * F * T
    if kind == GAUSS:
        f, fu = _pow(R, -2 / p, dtype, fast_pow)
        data, du = P * f, Prel + (2 / p) * Rrel + fu + 1
    elif kind == TMODEL:
        nu = dtype(param)
        f, fu = _pow(R, -2 / p, dtype, fast_pow)
        z = (2 / nu) * P * f
        # log(1 + z) moves by at most rel(z) log(1 + z): z / (1 + z) <= log(1 + z)
        data, du = (1 + nu / 2) * np.log1p(z), Prel + (2 / p) * Rrel + fu + 2 + 1 + 2 + 1
    else:
        beta = dtype(param)
        f1, f1u = _pow(P, beta / 2, dtype, fast_pow)
        f2, f2u = _pow(R, -beta / p, dtype, fast_pow)
        data, du = f1 * f2, (beta / 2) * Prel + f1u + (beta / p) * Rrel + f2u + 1
    logR = np.log(R)
    ax = (1, 2, 3)
    val = (data.sum(axis=ax) + (2 / p) * logR.sum(axis=ax)) / dtype(T)
    bar = U * ((n * data + data * du).sum(axis=ax)
               + (2 / p) * ((n + 4) * np.maximum(1, np.abs(logR).sum(axis=ax)) + n * Rrel)) / dtype(T)
    return val, bar


def ilrma_normalize_filter(W, C, basis, domain, flooring, dtype=LD):
    """psi_n = floor(sqrt(mean_i w_in^H C_i w_in)); W[:, n, :] / psi_n; basis[n] / psi_n^p.
    q_in = w^H C w: (6 N + 2) u on sum_kl |w_k| |c_kl| |w_l|; mean over F: + F + 1; sqrt halves and
    adds 2.  Returns (W, barW on the modulus, basis, bar_basis, psi, rel_psi_u)."""
    c = _c(dtype)
    B, F, N, _ = W.shape
    Wc, Cc = W.astype(c), C.astype(c)
    # (the filter of source n is row n of W: y_n = sum_m W[n, m] x_m, so its power is W C W^H)
    q = np.einsum("bink,bikl,binl->bin", Wc, Cc, Wc.conj()).real
    qa = np.einsum("bink,bikl,binl->bin", np.abs(Wc), np.abs(Cc), np.abs(Wc))
    m = q.mean(axis=1)
    m_eu = (6 * N + 2) * qa.mean(axis=1) + (F + 1) * m
    pre = np.sqrt(m)
    psi = floor(pre, flooring)
    rel = (0.5 * m_eu / m + 2) * pre / psi + (1 if flooring[0] == FLOOR_ADD else 0)
    Wn = Wc / psi[:, None, :, None]
    barW = U * np.abs(Wn) * (rel[:, None, :, None] + 3)
    p = dtype(domain)
    bn = basis.astype(dtype) / (psi ** p)[:, :, None, None]
    barb = U * bn * (p * rel + 2 + 3)[:, :, None, None]
    return Wn, barW, bn, barb, psi, rel


def ilrma_normalize_output(Y, basis, domain, flooring, dtype=LD, frame_power=None, logdet=None):
    """psi_n = floor(sqrt(mean_ij |y_nij|^2)) (or from frame_power (B,N,T) = sum_i |y|^2);
    Y / psi, basis / psi^p; logdet[b] -= F sum_n log psi_n.  Positive sums of F T (or T) terms."""
    c = _c(dtype)
    B, N, F, T = Y.shape
    Yc = Y.astype(c)
    if frame_power is None:
        m = (np.abs(Yc) ** 2).mean(axis=(2, 3))
        m_rel = F * T + 1 + 2
    else:
        m = frame_power.astype(dtype).sum(axis=2) / dtype(F * T)
        m_rel = T + 2
    pre = np.sqrt(m)
    psi = floor(pre, flooring)
    rel = (0.5 * m_rel + 2) * pre / psi + (1 if flooring[0] == FLOOR_ADD else 0)
    Yn = Yc / psi[:, :, None, None]
    barY = U * np.abs(Yn) * (rel[:, :, None, None] + 3)
    p = dtype(domain)
    bn = basis.astype(dtype) / (psi ** p)[:, :, None, None]
    barb = U * bn * (p * rel + 2 + 3)[:, :, None, None]
    out = [Yn, barY, bn, barb]
    if logdet is not None:
        lp = np.log(psi)
        ld = logdet.astype(dtype) - F * lp.sum(axis=1)
        out += [ld, U * (F * (rel + 2 * np.abs(lp) + 1).sum(axis=1)
                         + (N + 1) * (np.abs(logdet.astype(dtype)) + F * np.abs(lp).sum(axis=1)))]
    return out


def update_by_ip1(W, Ucov, flooring, dtype=LD):
    """One IP1 sweep: w = (W U_n)^-1 e_n, row n <- conj(w) / floor(sqrt(max(Re w^H U_n w, 0))).
    Returns (W_new, kappa (B,F): the largest 2-norm condition number of W U_n over the sweep)."""
    c = _c(dtype)
    B, F, N, _ = W.shape
    Wc = W.astype(c).reshape(B * F, N, N).copy()
    Uc = Ucov.astype(c).reshape(B * F, N, N, N)
    kappa = np.zeros(B * F)
    for n in range(N):
        A = np.einsum("fab,fbc->fac", Wc, Uc[:, n])
        e = np.zeros((B * F, N, 1), c)
        e[:, n, 0] = 1
        w = lu_solve(A, e)[0][:, :, 0]
        if dtype is LD:  # (the inverse in extended precision; its norm needs no more than float64)
            Ainv = lu_solve(A, np.broadcast_to(np.eye(N, dtype=c), A.shape).copy())[0]
            kappa = np.maximum(kappa, np.linalg.norm(A.astype(np.complex128), 2, axis=(1, 2))
                               * np.linalg.norm(Ainv.astype(np.complex128), 2, axis=(1, 2)))
        q = np.einsum("fa,fab,fb->f", w.conj(), Uc[:, n], w).real
        d = floor(np.sqrt(np.maximum(q, 0)), flooring)
        Wc[:, n, :] = w.conj() / d[:, None]
    return Wc.reshape(B, F, N, N), kappa.reshape(B, F)


def update_by_ip1_float64(W, Ucov, flooring):
    """The same sweep with np.linalg.solve in float64: the yardstick of the normwise bar."""
    B, F, N, _ = W.shape
    Wc = W.reshape(B * F, N, N).copy()
    Uc = Ucov.reshape(B * F, N, N, N)
    for n in range(N):
        e = np.zeros((B * F, N, 1), np.complex128)
        e[:, n, 0] = 1
        w = np.linalg.solve(Wc @ Uc[:, n], e)[:, :, 0]
        q = np.einsum("fa,fab,fb->f", w.conj(), Uc[:, n], w).real
        d = floor(np.sqrt(np.maximum(q, 0)), flooring)
        Wc[:, n, :] = w.conj() / d[:, None]
    return Wc.reshape(B, F, N, N)


def ip1_row_error(Wa, Wref, kappa):
    """max over rows and bins of ||w - w_ref|| / (kappa u ||w_ref||)."""
    num = np.linalg.norm((Wa.astype(np.clongdouble) - Wref).astype(np.complex128), axis=-1)
    den = np.linalg.norm(Wref.astype(np.complex128), axis=-1) * kappa[:, :, None] * U
    return float(np.max(num / den))


# ---------------------------------------------------------------------------------- AuxIVA passes
def iva_frame_power(X, W=None, dtype=LD):
    """r2[b,n,j] = sum_i |y_nij|^2: a positive sum of F terms over the per-element power bars."""
    P, Pbar = power(X, W, dtype)
    F = X.shape[2]
    r2 = P.sum(axis=2)
    return r2, F * U * r2 + Pbar.sum(axis=2)


def iva_weight(r2, variance, n_bins, contrast, flooring, dtype=LD):
    """weight = G'(r) / floor(2 r), r = sqrt(r2): LAPLACE G' = 2; GAUSS refreshes variance = r2 / F,
    G' = 2 r / variance; GAUSS_FIXED uses the variance given.  sqrt 2 u, product 1, divisions 2 each.
    Returns (weight, bar, variance_out, bar_variance)."""
    p = r2.astype(dtype)
    r = np.sqrt(p)
    pre = 2 * r
    den = floor(pre, flooring)
    den_rel = 2 * pre / den + (1 if flooring[0] == FLOOR_ADD else 0)
    if contrast == 0:
        w = 2 / den
        return w, U * w * (den_rel + 2), None, None
    if contrast == 1:
        var = p / dtype(n_bins)
        w = (2 * r / var) / den
        return w, U * w * (2 + 2 + 2 + den_rel + 2), var, 2 * U * var
    var = variance.astype(dtype)
    w = (2 * r / var) / den
    return w, U * w * (2 + 2 + den_rel + 2), var, 0 * var


def iva_loss_data(r2, variance, n_bins, contrast, dtype=LD):
    """out[b] = sum_n mean_j G: LAPLACE 2 r; GAUSS F log(variance) + r2 / variance (absolute bar,
    n = N T terms in any order on the sum of magnitudes, each log 2 u of itself)."""
    p = r2.astype(dtype)
    B, N, T = p.shape
    if contrast == 0:
        g = 2 * np.sqrt(p)
        mag, gu = g, 2 * g
    else:
        var = variance.astype(dtype)
        lg = n_bins * np.log(var)
        g = lg + p / var
        mag, gu = np.abs(lg) + p / var, 3 * np.abs(lg) + 3 * p / var
    val = g.sum(axis=(1, 2)) / dtype(T)
    return val, U * ((N * T + 2) * mag + gu).sum(axis=(1, 2)) / dtype(T)


# ---------------------------------------------------------------------------------- generators
def _log_uniform(rng, lo, hi, shape):
    return np.exp2(rng.uniform(lo, hi, shape))


def gen_spectrogram(seed, B, N, F, T):
    """|X| log-uniform in 2^-20..2^20 per (bin, frame) -- the scale of a column, shared by its
    channels, times a per-channel factor in [1/2, 2) -- with random phase."""
    rng = np.random.default_rng(seed)
    scale = _log_uniform(rng, -19, 19, (B, 1, F, T))
    mag = scale * _log_uniform(rng, -1, 1, (B, N, F, T))
    return (mag * np.exp(2j * np.pi * rng.random((B, N, F, T)))).astype(np.complex128)


def gen_nmf(seed, B, N, F, T, K):
    """basis (B,N,F,K) and activation (B,N,K,T), every entry log-uniform in 2^-12..2^12."""
    rng = np.random.default_rng(seed + 1)
    return _log_uniform(rng, -12, 12, (B, N, F, K)), _log_uniform(rng, -12, 12, (B, N, K, T))


def gen_filters(seed, B, F, N, log2_range=8):
    """W (B,F,N,N): diag(d) Q, Q random unitary, d log-uniform in 2^-r..2^r (rows scaled, as the
    power normalisation scales them; kappa_2 <= 2^(2 r))."""
    rng = np.random.default_rng(seed + 2)
    A = rng.standard_normal((B, F, N, N)) + 1j * rng.standard_normal((B, F, N, N))
    Q, _ = np.linalg.qr(A)
    d = _log_uniform(rng, -log2_range, log2_range, (B, F, N, 1))
    return np.ascontiguousarray(d * Q)


def gen_weights(seed, shape):
    """positive weights, log-uniform in 2^-12..2^12."""
    return _log_uniform(np.random.default_rng(seed + 3), -12, 12, shape)


def gen_floor_nmf(seed, B, N, F, T, K, eps=EPS):
    """(basis, activation) scaled so that the UPDATED values straddle eps: the update multiplies by
    a ratio near sqrt(P / R^2)-ish of order one for matched scales, so old values log-uniform in
    eps 2^-6..eps 2^6, with a few exactly eps."""
    rng = np.random.default_rng(seed + 4)
    basis = eps * _log_uniform(rng, -6, 6, (B, N, F, K))
    act = eps * _log_uniform(rng, -6, 6, (B, N, K, T))
    basis.reshape(-1)[::7] = eps
    act.reshape(-1)[::5] = eps
    return basis, act


def gen_ip1_inputs(seed, B, F, N, T=24):
    """(W, U): filters with rows in 2^-1..2^1 and U_n = (1/T) sum_j w_nj x x^H of a well-spread x with
    weights in [1/2, 2], so that kappa(W U_n) <= 1e3."""
    rng = np.random.default_rng(seed + 5)
    W = gen_filters(seed, B, F, N, log2_range=1)
    T = max(T, 6 * N)
    x = rng.standard_normal((B, N, F, T)) + 1j * rng.standard_normal((B, N, F, T))
    w = _log_uniform(rng, -1, 1, (B, N, F, T))
    Uc = np.einsum("bnij,baij,bcij->binac", w, x, x.conj()) / T
    return W, np.ascontiguousarray(Uc)


# ---- guard bands: inputs are followed by NaN in the same allocation (a read past the end that is
# USED poisons the result); outputs sit between two sentinel bands that must come back untouched
BAND = 4096
SENTINEL = -7.25e300


def with_nan_band(a):
    """flat float64 view of `a` followed by BAND NaNs; returns (flat, n_doubles)."""
    flat = np.ascontiguousarray(a).view(np.float64).reshape(-1)
    return np.concatenate([flat, np.full(BAND, np.nan)]), flat.size


def sentinel_buffer(n_doubles, fill=None):
    """BAND sentinels, n_doubles of payload (`fill` flat float64, or sentinels too), BAND sentinels."""
    buf = np.full(n_doubles + 2 * BAND, SENTINEL)
    if fill is not None:
        buf[BAND:BAND + n_doubles] = np.ascontiguousarray(fill).view(np.float64).reshape(-1)
    return buf


def bands_intact(buf):
    buf = np.asarray(buf)
    return bool(np.all(buf[:BAND] == SENTINEL) and np.all(buf[-BAND:] == SENTINEL))


# ---------------------------------------------------------------------------------- fused update
def gen_fused_inputs(seed, B, N, F, T, K):
    """Inputs of one whole update_once() whose per-bin systems stay well conditioned
    (kappa(W U_n) <= 1e3): a spectrogram of unit-variance columns with per-element magnitudes over
    1/2..2, NMF factors over 2^-1..2^1, filters with rows over 2^-1..2^1, and the mixture's covariance
    C = (1/T) sum_j x x^H in float64."""
    rng = np.random.default_rng(seed + 6)
    X = (rng.standard_normal((B, N, F, T)) + 1j * rng.standard_normal((B, N, F, T))) \
        * _log_uniform(rng, -1, 1, (B, N, F, T))
    basis = _log_uniform(rng, -1, 1, (B, N, F, K))
    act = _log_uniform(rng, -1, 1, (B, N, K, T))
    W = gen_filters(seed, B, F, N, log2_range=1)
    C = np.asarray(cross_covariance(X, X)[0], dtype=np.complex128)
    return X, W, basis, act, C


def ilrma_ip1_update(X, C, W, basis, activation, domain, model, normalize, flooring, dtype=LD,
                     fast_pow=True):
    """The composition of the references in the order of update_once(): basis, activation WITH THE NEW
    BASIS, weighted covariance, IP1, power normalisation.  The elementwise bars of basis and activation
    are those of their passes (the activation's with the new basis's own error handed in); W and psi
    come from solves and have no elementwise bar (kappa is returned for the normwise one)."""
    b1, bar_b = ilrma_update_basis(X, W, basis, activation, domain, model, flooring, dtype, fast_pow)
    rel_b = float(np.max(bar_b / (U * b1)))
    a1, bar_a = ilrma_update_activation(X, W, b1, activation, domain, model, flooring, dtype,
                                        fast_pow, basis_rel_u=rel_b)
    rel_a = float(np.max(bar_a / (U * a1)))
    U1, _ = ilrma_weighted_covariance(X, W, b1, a1, domain, model, flooring, dtype, fast_pow,
                                      basis_rel_u=rel_b + rel_a)
    if dtype is LD:
        W1, kappa = update_by_ip1(W, U1, flooring)
    else:
        W1, kappa = update_by_ip1_float64(W, np.ascontiguousarray(U1), flooring), None
    out = {"basis": b1, "bar_basis": bar_b, "activation": a1, "bar_activation": bar_a, "W": W1,
           "kappa": kappa, "psi": None}
    if normalize:
        Wn, _, bn, _, psi, _ = ilrma_normalize_filter(W1, C, b1, domain, flooring, dtype)
        out.update(W=Wn, basis=bn, psi=psi)
    return out
