"""Plain NumPy restatement of WPE dereverberation as ssspy_amd.dereverb.WPE defines it (Nakatani et
al., IEEE TASLP 18(7), 2010): one loop over the bins, ``numpy.linalg.cholesky`` / ``solve``.  With
``dtype=numpy.longdouble`` the LAPACK calls are replaced by a hand-written Cholesky factorisation and
triangular solves, so the whole iteration runs in extended precision.

Per bin, with x_t in C^M, K taps, delay D and L = K M:
    xs_t[k M + m] = x[m, t - D - k] (zero before the first frame),  y_t = x_t - G^H xs_t,  G = 0 first
    lambda_t = floor(mean_m |y_mt|^2);  R = sum_t xs_t xs_t^H / lambda_t;  P = sum_t xs_t x_t^H / lambda_t
    G = R^-1 P (Cholesky);  loss = (1 / T) sum_f sum_t [M log lambda_ft + sum_m |y_mft|^2 / lambda_ft]
"""

import numpy as np

MAX_FLOOR = ("max", 1e-10)  # the default of the class: functools.partial(max_flooring, eps=1e-10)


def _complex(dtype):
    return np.clongdouble if np.dtype(dtype) == np.dtype(np.longdouble) else np.complex128


def floor(x, flooring):
    if flooring is None:
        return x
    kind, eps = flooring
    if kind == "max":
        return np.maximum(x, x.dtype.type(eps))
    if kind == "add":
        return x + x.dtype.type(eps)
    raise ValueError(kind)


def stack_history(Xf, taps, delay):
    """(M, T) -> (L, T): row k M + m holds x[m, t - delay - k], zeros where that is negative."""
    M, T = Xf.shape
    xs = np.zeros((taps * M, T), dtype=Xf.dtype)
    for k in range(taps):
        shift = delay + k
        if shift < T:
            xs[k * M:(k + 1) * M, shift:] = Xf[:, :T - shift]
    return xs


def cholesky_upper(R):
    """U upper triangular with a real positive diagonal, R = U^H U; right-looking, in R's dtype."""
    A = np.array(R, copy=True)
    L = A.shape[0]
    U = np.zeros_like(A)
    for j in range(L):
        d = A[j, j].real
        if not (d > 0) or not np.isfinite(d):
            raise np.linalg.LinAlgError("Matrix is not positive definite")
        root = np.sqrt(d)
        U[j, j] = root
        U[j, j + 1:] = A[j, j + 1:] / root
        A[j + 1:, j + 1:] -= np.conj(U[j, j + 1:])[:, None] * U[j, j + 1:][None, :]
    return U


def solve_cholesky(U, P):
    """G with U^H U G = P by forward and back substitution."""
    L = U.shape[0]
    Z = np.array(P, copy=True)
    for j in range(L):
        Z[j] = (Z[j] - np.conj(U[:j, j]) @ Z[:j]) / U[j, j].real
    for j in range(L - 1, -1, -1):
        Z[j] = (Z[j] - U[j, j + 1:] @ Z[j + 1:]) / U[j, j].real
    return Z


def apply_filter(Xf, G, taps, delay):
    """y = x - G^H xs for one bin: Xf (M, T), G (L, M)."""
    return Xf - np.conj(G.T) @ stack_history(Xf, taps, delay)


def variance(Yf, flooring):
    M = Yf.shape[0]
    power = np.sum(Yf.real ** 2 + Yf.imag ** 2, axis=0)
    return floor(power / M, flooring), power


def bin_loss(Yf, flooring):
    """sum_t [M log lambda_t + sum_m |y_mt|^2 / lambda_t] / T of one bin."""
    M, T = Yf.shape
    lam, power = variance(Yf, flooring)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sum(M * np.log(lam) + power / lam) / T


def bin_step(Xf, G, taps, delay, flooring, extended):
    """One iteration on one bin: the new G and what it was formed from."""
    Yf = apply_filter(Xf, G, taps, delay)
    lam, _ = variance(Yf, flooring)
    xs = stack_history(Xf, taps, delay)
    with np.errstate(divide="ignore", invalid="ignore"):
        weighted = xs / lam[None, :]
    R = weighted @ np.conj(xs.T)
    P = weighted @ np.conj(Xf.T)
    if extended:
        U = cholesky_upper(R)
        G_new = solve_cholesky(U, P)
    else:
        U = np.conj(np.linalg.cholesky(R).T)
        Z = np.linalg.solve(np.conj(U.T), P)
        G_new = np.linalg.solve(U, Z)
    return G_new, {"lambda": lam, "R": R, "P": P, "U": U}


def run(X, taps, delay, n_iter=3, flooring=MAX_FLOOR, dtype=np.float64, prediction_filter=None,
        statistics=False):
    """X (M, F, T) or (B, M, F, T).  Returns ``output`` (as X), ``prediction_filter`` (F, K, M, M)
    (with the leading mixture axis of X), ``loss``: n_iter + 1 entries, floats or (B,) arrays; with
    ``statistics`` also lambda (F, T), R (F, L, L), P (F, L, M), U (F, L, L) of the LAST iteration."""
    ctype = _complex(dtype)
    extended = ctype is np.clongdouble
    X = np.asarray(X)
    batched = X.ndim == 4
    X4 = (X if batched else X[None]).astype(ctype)
    B, M, F, T = X4.shape
    L = taps * M
    if prediction_filter is None:
        G = np.zeros((B, F, L, M), dtype=ctype)
    else:
        G = np.array(prediction_filter, dtype=ctype).reshape(B, F, L, M)
    Y = np.empty_like(X4)
    loss = np.zeros((n_iter + 1, B), dtype=dtype)
    stats = {"lambda": np.zeros((B, F, T), dtype), "R": np.zeros((B, F, L, L), ctype),
             "P": np.zeros((B, F, L, M), ctype), "U": np.zeros((B, F, L, L), ctype)}
    for b in range(B):
        for f in range(F):
            Xf = X4[b, :, f, :]
            Gf = G[b, f]
            loss[0, b] += bin_loss(apply_filter(Xf, Gf, taps, delay), flooring)
            for it in range(n_iter):
                Gf, st = bin_step(Xf, Gf, taps, delay, flooring, extended)
                loss[it + 1, b] += bin_loss(apply_filter(Xf, Gf, taps, delay), flooring)
                if it == n_iter - 1:
                    for key in stats:
                        stats[key][b, f] = st[key]
            G[b, f] = Gf
            Y[b, :, f, :] = apply_filter(Xf, Gf, taps, delay)
    G = G.reshape(B, F, taps, M, M)
    result = {
        "output": Y if batched else Y[0],
        "prediction_filter": G if batched else G[0],
        "loss": [row.copy() if batched else row[0] for row in loss],
    }
    if statistics:
        result.update({k: (v if batched else v[0]) for k, v in stats.items()})
    return result
