"""Plain NumPy restatement of IVA with joint dereverberation as ssspy_amd.bss.ConvLaplaceIVA /
ConvGaussIVA define it (Nakatani et al., Interspeech 2020, the source-wise factorisation): loops over
mixtures, bins and sources, ``numpy.linalg.cholesky`` / ``solve``.  With ``dtype=numpy.longdouble`` the
LAPACK calls are replaced by the hand-written Cholesky factorisation and triangular solves of
wpe_numpy and a Gaussian elimination with partial pivoting, so the whole iteration runs in extended
precision.

Per mixture, M channels and sources, K taps, delay D, L = K M, Lb = (K + 1) M, xb_t as wpd_numpy.stack:
    W (F, M, Lb), y_nft = sum_l W[f, n, l] xb_ft[l], W[f, n, :M] = e_n first
    r_nt^2 = sum_f |y_nft|^2
    laplace  phi = 2 / floor(2 r)                      (the weights of AuxLaplaceIVA)
    gauss    alpha = r^2 / F, phi = (2 r / alpha) / floor(2 r)  (AuxGaussIVA; alpha is kept for the loss)
    Rb = (1 / T) sum_t phi_nt xb_t xb_t^H, C = Rb[:M, :M], P = Rb[M:, :M],
    R = Rb[M:, M:] + loading (Re tr R / L) I, G_n = R^-1 P (R = U^H U), Sigma_n = C - P^H G_n
    IP1 on Q = W[f, :, :M] for n = 0..M-1: w = (Q Sigma_n)^-1 e_n, Q[n] = conj(w) / floor(sqrt(w^H Sigma_n w))
    W[f, n] = conj([q_n; -G_n q_n]), q_n = conj(Q[n])
    loss = sum_n mean_t G(r_nt) - 2 sum_f log|det Q_f|
A Cholesky pivot that is not positive and finite is counted in "failed" once per (mixture, bin,
source): G_n and Sigma_n of that iteration are not formed, the sweep runs with the Sigma_n the triple
last had (the identity before its first success), and the triple keeps its row of W.
"""

import numpy as np

import wpd_numpy
import wpe_numpy

MAX_FLOOR = ("max", 1e-10)  # the default of the classes: functools.partial(max_flooring, eps=1e-10)


def _complex(dtype):
    return np.clongdouble if np.dtype(dtype) == np.dtype(np.longdouble) else np.complex128


def solve_vector(A, rhs):
    """A^-1 rhs by Gaussian elimination with partial pivoting, in A's dtype."""
    A = np.array(A, copy=True)
    x = np.array(rhs, dtype=A.dtype, copy=True)
    n = A.shape[0]
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        if A[p, j] == 0:
            raise np.linalg.LinAlgError("Singular matrix")
        if p != j:
            A[[j, p]] = A[[p, j]]
            x[[j, p]] = x[[p, j]]
        for i in range(j + 1, n):
            m = A[i, j] / A[j, j]
            A[i, j:] -= m * A[j, j:]
            x[i] -= m * x[j]
    for j in range(n - 1, -1, -1):
        x[j] = (x[j] - A[j, j + 1:] @ x[j + 1:]) / A[j, j]
    return x


def weights(r2, n_bins, contrast, flooring):
    """(phi, alpha) from the frame powers (M, T); alpha is None for the Laplace contrast."""
    real = r2.dtype.type
    r = np.sqrt(r2)
    denom = wpe_numpy.floor(real(2) * r, flooring)
    if contrast == "laplace":
        return real(2) / denom, None
    if contrast != "gauss":
        raise ValueError(contrast)
    alpha = r2 / real(n_bins)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (real(2) * r / alpha) / denom, alpha


def data_term(r2, alpha, n_bins, contrast):
    """sum_n mean_t G(r_nt)."""
    real = r2.dtype.type
    if contrast == "laplace":
        return np.sum(real(2) * np.sqrt(r2)) / r2.shape[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sum(real(n_bins) * np.log(alpha) + r2 / alpha) / r2.shape[-1]


def logabsdet(Q):
    if Q.dtype == np.clongdouble:
        # log|det| through the pivots of the elimination
        A = np.array(Q, copy=True)
        n = A.shape[0]
        total = np.longdouble(0)
        for j in range(n):
            p = j + int(np.argmax(np.abs(A[j:, j])))
            if p != j:
                A[[j, p]] = A[[p, j]]
            total += np.log(np.abs(A[j, j]))
            for i in range(j + 1, n):
                A[i, j:] -= (A[i, j] / A[j, j]) * A[j, j:]
        return total
    return np.linalg.slogdet(Q)[1]


def statistics(xb, phi, M, loading, extended):
    """(Sigma, G, {"Rb", "U", "cond"}) of one (bin, source) from xb (Lb, T) and phi (T,).  Raises
    LinAlgError on a pivot that is not positive and finite."""
    Lb, T = xb.shape
    L = Lb - M
    real = xb.real.dtype.type
    Rb = (xb * phi[None, :]) @ np.conj(xb.T) / real(T)
    Rb[np.diag_indices(Lb)] = np.diagonal(Rb).real
    if L == 0:
        return Rb.copy(), np.zeros((0, M), dtype=xb.dtype), {
            "Rb": Rb, "U": np.zeros((0, 0), dtype=xb.dtype), "cond": 1.0}
    Rb[M:, M:] += real(loading) * (np.trace(Rb[M:, M:]).real / L) * np.eye(L, dtype=xb.dtype)
    C, P, R = Rb[:M, :M], Rb[M:, :M], Rb[M:, M:]
    if extended:
        U = wpe_numpy.cholesky_upper(R)
        G = wpe_numpy.solve_cholesky(U, P)
    else:
        if not np.all(np.isfinite(R)):
            raise np.linalg.LinAlgError("R is not finite")
        U = np.conj(np.linalg.cholesky(R).T)
        if not np.all(np.isfinite(U)):
            raise np.linalg.LinAlgError("pivot not finite")
        G = np.linalg.solve(U, np.linalg.solve(np.conj(U.T), P))
    Sigma = C - np.conj(P.T) @ G
    Sigma = (np.triu(Sigma) + np.conj(np.triu(Sigma, 1).T))
    Sigma[np.diag_indices(M)] = np.diagonal(Sigma).real
    with np.errstate(all="ignore"):
        cond = float(np.linalg.cond(R.astype(np.complex128)))
    return Sigma, G, {"Rb": Rb, "U": U, "cond": cond}


def ip1_sweep(Q, Sigma, flooring, extended):
    """update_by_ip1 on one bin: Q (M, M) rows, Sigma (M, M, M); a new Q."""
    Q = np.array(Q, copy=True)
    M = Q.shape[0]
    for n in range(M):
        e = np.zeros(M, dtype=Q.dtype)
        e[n] = 1
        A = Q @ Sigma[n]
        w = solve_vector(A, e) if extended else np.linalg.solve(A, e)
        q = (np.conj(w) @ Sigma[n] @ w).real
        d = wpe_numpy.floor(np.sqrt(np.maximum(q, q.dtype.type(0)))[None], flooring)[0]
        Q[n] = np.conj(w) / d
    return Q


def compose(Qrow, G):
    """conj([q; -G q]) with q = conj(Qrow): the row of W."""
    return np.concatenate([Qrow, -np.conj(G) @ Qrow])


def run(X, taps, delay, n_iter=3, contrast="laplace", loading=0.0, flooring=MAX_FLOOR,
        dtype=np.float64, convolutional_filter=None, scale_restoration=True, reference_id=0):
    """X (M, F, T) or (B, M, F, T).  Returns ``output`` (M, F, T), ``convolutional_filter``
    (F, M, K + 1, M), ``demix_filter`` (F, M, M), ``prediction_filter`` (F, M, K, M, M) (all with the
    leading mixture axis of X), ``loss``: n_iter + 1 entries (before scale restoration), floats or
    (B,) arrays, ``failed`` and ``max_cond``, the largest cond R met."""
    ctype = _complex(dtype)
    extended = ctype is np.clongdouble
    X = np.asarray(X)
    batched = X.ndim == 4
    X4 = (X if batched else X[None]).astype(ctype)
    B, M, F, T = X4.shape
    K, L, Lb = taps, taps * M, (taps + 1) * M
    W = np.zeros((B, F, M, Lb), dtype=ctype)
    if convolutional_filter is None:
        W[:, :, :, :M] = np.eye(M, dtype=ctype)
    else:
        W[...] = np.asarray(convolutional_filter).reshape(B, F, M, Lb)
    G = np.zeros((B, F, M, L, M), dtype=ctype)
    Sigma = np.tile(np.eye(M, dtype=ctype), (B, F, M, 1, 1))
    Y = np.zeros((B, M, F, T), dtype=ctype)
    loss = np.zeros((n_iter + 1, B), dtype=dtype)
    ever_failed = np.zeros((B, F, M), dtype=bool)
    max_cond = 0.0
    for b in range(B):
        xb = [wpd_numpy.stack(X4[b, :, f, :], K, delay) for f in range(F)]
        alpha = np.ones((M, T), dtype=dtype)

        def separate():
            for f in range(F):
                Y[b, :, f, :] = W[b, f] @ xb[f]
            return np.sum(Y[b].real ** 2 + Y[b].imag ** 2, axis=1)

        def logdet():
            return sum(logabsdet(W[b, f, :, :M]) for f in range(F))

        r2 = separate()
        for it in range(n_iter):
            loss[it, b] = data_term(r2, alpha, F, contrast) - 2 * logdet()
            phi, new_alpha = weights(r2, F, contrast, flooring)
            if new_alpha is not None:
                alpha = new_alpha
            for f in range(F):
                failed_now = np.zeros(M, dtype=bool)
                for n in range(M):
                    try:
                        Sigma[b, f, n], G[b, f, n], st = statistics(xb[f], phi[n], M, loading,
                                                                    extended)
                        max_cond = max(max_cond, st["cond"])
                    except np.linalg.LinAlgError:
                        failed_now[n] = ever_failed[b, f, n] = True
                Q = ip1_sweep(W[b, f, :, :M], Sigma[b, f], flooring, extended)
                for n in range(M):
                    if not failed_now[n]:
                        W[b, f, n] = compose(Q[n], G[b, f, n])
            r2 = separate()
        loss[n_iter, b] = data_term(r2, alpha, F, contrast) - 2 * logdet()
        if scale_restoration:
            for f in range(F):
                Q = W[b, f, :, :M]
                if extended:
                    scale = np.array([solve_vector(Q, np.eye(M, dtype=ctype)[n])[reference_id]
                                      for n in range(M)])
                else:
                    scale = np.linalg.inv(Q)[reference_id, :]
                for n in range(M):
                    W[b, f, n] = compose(Q[n] * scale[n], G[b, f, n])
            separate()
    result = {"output": Y, "convolutional_filter": W.reshape(B, F, M, K + 1, M),
              "demix_filter": W[..., :M].copy(), "prediction_filter": G.reshape(B, F, M, K, M, M)}
    if not batched:
        result = {k: v[0] for k, v in result.items()}
    result["loss"] = [row.copy() if batched else row[0] for row in loss]
    result["failed"] = int(ever_failed.sum())
    result["max_cond"] = max_cond
    return result
