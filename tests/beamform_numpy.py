"""NumPy restatement of the mask-based beamformers (ssspy_amd.beamform), literally as defined:

  S_n = sum_t m_nt x_t x_t^H, a_n = sum_t m_nt, N_n = sum_t u_nt x_t x_t^H, b_n = sum_t u_nt
  (u = noise_mask, or 1 - m), Phi_s = S_n / max(a_n, eps),
  Phi_v = N_n / max(b_n, eps) + loading (tr(N_n / max(b_n, eps)) / M) I, eps = 1e-10
  MVDR  A = Phi_v^-1 Phi_s (Cholesky), w = A e_ref / max(Re tr A, eps)
  MWF   w = (Phi_s + mu Phi_v)^-1 Phi_s e_ref
  GEV   Phi_v = L L^H, C = L^-1 Phi_s L^-H, v the unit eigenvector of its largest eigenvalue,
        w0 = L^-H v, a = L v; "reference": w = w0 conj(a_ref); "ban": w = w0 p ||a|| / sqrt(M),
        p = conj(a_ref) / |a_ref| (1 where a_ref = 0)
  y_nt = w_n^H x_t, demix_filter[f, n, :] = w_n^H
  A Phi_s that is zero in every entry gives w = 0; so does a Phi_v whose Cholesky factorisation
  meets a pivot that is not positive and finite (counted in "failed").

Dtype-generic: float64 goes through numpy.linalg.cholesky / eigh; longdouble, for which NumPy has
neither, through the hand-written factorisation and the cyclic Jacobi iteration below.
"""

import numpy as np

EPS = 1e-10
KINDS = ("mvdr", "gev", "mwf")


def _ctype(dtype):
    return np.clongdouble if np.dtype(dtype) == np.longdouble else np.complex128


def cholesky(A):
    """Lower factor of a Hermitian positive definite matrix; LinAlgError on a pivot that is not
    positive and finite."""
    if A.dtype == np.complex128:
        L = np.linalg.cholesky(A)
        if not np.all(np.isfinite(L)):
            raise np.linalg.LinAlgError("pivot not finite")
        return L
    n = A.shape[0]
    L = np.zeros_like(A)
    for c in range(n):
        d = A[c, c].real - np.sum(np.abs(L[c, :c]) ** 2)
        if not (d > 0 and np.isfinite(d)):
            raise np.linalg.LinAlgError("pivot not positive and finite")
        L[c, c] = np.sqrt(d)
        for r in range(c + 1, n):
            L[r, c] = (A[r, c] - np.sum(L[r, :c] * np.conj(L[c, :c]))) / L[c, c]
    return L


def lower_solve(L, Bm):
    """L^-1 Bm by forward substitution, in the dtype of L."""
    n = L.shape[0]
    Z = np.array(Bm, dtype=L.dtype, copy=True)
    for r in range(n):
        Z[r] = (Z[r] - L[r, :r] @ Z[:r]) / L[r, r]
    return Z


def upper_solve(U, Bm):
    """U^-1 Bm by back substitution."""
    n = U.shape[0]
    Z = np.array(Bm, dtype=U.dtype, copy=True)
    for r in range(n - 1, -1, -1):
        Z[r] = (Z[r] - U[r, r + 1:] @ Z[r + 1:]) / U[r, r]
    return Z


def jacobi_eigh(A, sweeps=30):
    """Eigenvalues (unsorted) and unit eigenvectors (columns) of a Hermitian matrix by cyclic complex
    Jacobi rotations, in the dtype of A."""
    A = np.array(A, copy=True)
    n = A.shape[0]
    real = A.real.dtype.type
    P = np.eye(n, dtype=A.dtype)
    tiny = np.finfo(real).eps ** 2
    for _ in range(sweeps):
        off = sum(abs(A[p, q]) ** 2 for p in range(n) for q in range(p + 1, n))
        diag = sum(A[p, p].real ** 2 for p in range(n))
        if off <= tiny * tiny * diag:
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                mag = abs(A[p, q])
                if mag == 0:
                    continue
                u = A[p, q] / mag
                tau = (A[q, q].real - A[p, p].real) / (2 * mag)
                t = (1 if tau >= 0 else -1) / (abs(tau) + np.sqrt(1 + tau * tau))
                c = 1 / np.sqrt(1 + t * t)
                s = t * c
                G = np.eye(n, dtype=A.dtype)  # A <- G^H A G annihilates A[p, q]
                G[p, p] = c
                G[q, q] = c
                G[p, q] = s * u
                G[q, p] = -s * np.conj(u)
                A = np.conj(G.T) @ A @ G
                A = (A + np.conj(A.T)) / 2
                P = P @ G
    return A.diagonal().real.copy(), P


def eigh_principal(C):
    """Unit eigenvector of the largest eigenvalue of a Hermitian matrix."""
    C = (C + np.conj(C.T)) / 2
    if C.dtype == np.complex128:
        _, vecs = np.linalg.eigh(C)
        return vecs[:, -1]
    lam, P = jacobi_eigh(C)
    v = P[:, int(np.argmax(lam))]
    return v / np.sqrt(np.sum(np.abs(v) ** 2))


def bin_sums(Xf, mask_f, noise_f=None):
    """S (N, M, M), Nv (N, M, M), a (N), b (N) of one bin: Xf (M, T), mask_f (N, T), noise_f (N, T),
    (T,) or None; in the dtype of Xf."""
    real = Xf.real.dtype
    m = np.asarray(mask_f, dtype=real)
    one = np.ones((), dtype=real)
    u = one - m if noise_f is None else np.broadcast_to(np.asarray(noise_f, dtype=real), m.shape)
    S = np.einsum("nt,it,jt->nij", m, Xf, np.conj(Xf))
    Nv = np.einsum("nt,it,jt->nij", u, Xf, np.conj(Xf))
    return S, Nv, m.sum(axis=1), u.sum(axis=1)


def covariances(S, Nv, a, b, loading):
    """Phi_s and Phi_v (loading included) from the sums of one source."""
    M = S.shape[-1]
    real = S.real.dtype.type
    Phi_s = S / max(a, real(EPS))
    Phi_v = Nv / max(b, real(EPS))
    Phi_v = Phi_v + real(loading) * (np.trace(Phi_v).real / M) * np.eye(M, dtype=S.dtype)
    return Phi_s, Phi_v


def filter_from_covariances(Phi_s, Phi_v, kind, ref=0, mu=1.0, normalization="reference", phase=None):
    """(w, failed) of one (bin, source).  ``phase``: a unit-modulus factor put on the eigenvector of
    GEV (the tests of its invariance)."""
    M = Phi_s.shape[0]
    real = Phi_s.real.dtype.type
    w = np.zeros(M, dtype=Phi_s.dtype)
    if not np.any(Phi_s):
        return w, False
    V = Phi_s + real(mu) * Phi_v if kind == "mwf" else Phi_v
    try:
        L = cholesky(V)
    except np.linalg.LinAlgError:
        return w, True
    LH = np.conj(L.T)
    if kind in ("mvdr", "mwf"):
        A = upper_solve(LH, lower_solve(L, Phi_s))
        if kind == "mvdr":
            return A[:, ref] / max(np.trace(A).real, real(EPS)), False
        return A[:, ref], False
    assert kind == "gev", kind
    Z = lower_solve(L, Phi_s)                      # L^-1 Phi_s
    C = np.conj(lower_solve(L, np.conj(Z.T)).T)    # (L^-1 Z^H)^H = Z L^-H
    v = eigh_principal(C)
    if phase is not None:
        v = v * phase
    w0 = upper_solve(LH, v)
    a = L @ v
    if normalization == "reference":
        return w0 * np.conj(a[ref]), False
    assert normalization == "ban", normalization
    mag = abs(a[ref])
    p = np.conj(a[ref]) / mag if mag > 0 else 1
    return w0 * p * np.sqrt(np.sum(np.abs(a) ** 2)) / np.sqrt(real(M)), False


def run(X, mask, noise_mask=None, kind="mvdr", ref=0, loading=0.0, mu=1.0, normalization="reference",
        dtype=np.float64):
    """The whole beamformer: X (M, F, T) or (B, M, F, T), mask (N, F, T) or (B, N, F, T), noise_mask of
    the mask's shape or (F, T) / (B, F, T).  Returns output, demix_filter (F, N, M),
    signal_covariance, noise_covariance (F, N, M, M), S, Nv, a, b (the raw sums) and failed."""
    ctype = _ctype(dtype)
    X, mask = np.asarray(X), np.asarray(mask)
    batched = X.ndim == 4
    X4 = (X if batched else X[None]).astype(ctype)
    m4 = (mask if batched else mask[None]).astype(dtype)
    n4 = None
    if noise_mask is not None:
        noise_mask = np.asarray(noise_mask)
        n4 = (noise_mask if batched else noise_mask[None]).astype(dtype)
    B, M, F, T = X4.shape
    N = m4.shape[1]
    out = {"output": np.zeros((B, N, F, T), ctype), "demix_filter": np.zeros((B, F, N, M), ctype),
           "signal_covariance": np.zeros((B, F, N, M, M), ctype),
           "noise_covariance": np.zeros((B, F, N, M, M), ctype),
           "S": np.zeros((B, F, N, M, M), ctype), "Nv": np.zeros((B, F, N, M, M), ctype),
           "a": np.zeros((B, F, N), dtype), "b": np.zeros((B, F, N), dtype)}
    failed = 0
    for b in range(B):
        for f in range(F):
            Xf = X4[b, :, f, :]
            noise_f = None if n4 is None else (n4[b, f] if n4.ndim == 3 else n4[b, :, f, :])
            S, Nv, a, bb = bin_sums(Xf, m4[b, :, f, :], noise_f)
            out["S"][b, f], out["Nv"][b, f], out["a"][b, f], out["b"][b, f] = S, Nv, a, bb
            for n in range(N):
                Phi_s, Phi_v = covariances(S[n], Nv[n], a[n], bb[n], loading)
                w, bad = filter_from_covariances(Phi_s, Phi_v, kind, ref, mu, normalization)
                failed += bool(bad)
                out["signal_covariance"][b, f, n], out["noise_covariance"][b, f, n] = Phi_s, Phi_v
                out["demix_filter"][b, f, n] = np.conj(w)
                out["output"][b, n, f, :] = np.conj(w) @ Xf
    if not batched:
        out = {k: v[0] for k, v in out.items()}
    out["failed"] = failed
    return out
