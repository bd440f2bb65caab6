"""Plain NumPy restatement of the WPD convolutional beamformer as ssspy_amd.beamform.WPD defines it
(Nakatani & Kinoshita, IEEE SPL 26(6), 2019; Boeddeker et al., ICASSP 2020): one loop over mixtures,
bins and sources, ``numpy.linalg.cholesky`` / ``solve``.  With ``dtype=numpy.longdouble`` the LAPACK
calls are replaced by the hand-written Cholesky factorisation and triangular solves of wpe_numpy, so
the whole iteration runs in extended precision.

Per (bin, source), with x_t in C^M, K taps, delay D and Lb = (K + 1) M:
    xb_t: block 0 = x_t, block j = 1..K = x_{t - D - (j - 1)} (zero before the first frame)
    y_t = wb^H xb_t,  wb = e_ref first;  Phi_s = sum_t m_t x_t x_t^H / max(sum_t m_t, 1e-10)
    lambda_t = floor(|y_t|^2);  R = (1 / T) sum_t xb_t xb_t^H / lambda_t + loading (tr R / Lb) I
    mask form      A = (R^-1)[:, :M] Phi_s,  wb = A[:, ref] / Re tr(A[:M, :])
    steering form  vb = [v; 0],  a = R^-1 vb,  wb = a conj(v_ref) / (vb^H a)
    a denominator that is zero or not finite gives wb = 0
    loss = (1 / T) sum_n sum_f sum_t [log lambda_t + |y_t|^2 / lambda_t]
    convolutional_filter[f, n, j, m] = conj(wb[j M + m])
A Cholesky pivot that is not positive and finite ends the iterations of the (bin, source), which keeps
the filter the iteration started from, and is counted in "failed".
"""

import numpy as np

import wpe_numpy

EPS = 1e-10
MAX_FLOOR = ("max", 1e-6)  # the default of the class: functools.partial(max_flooring, eps=1e-6)
LOADING = 1e-6             # the default diagonal_loading of the class


def _complex(dtype):
    return np.clongdouble if np.dtype(dtype) == np.dtype(np.longdouble) else np.complex128


def stack(Xf, taps, delay):
    """(M, T) -> (Lb, T): rows 0..M-1 hold x_t, row j M + m (j >= 1) holds x[m, t - delay - (j - 1)],
    zeros where that is negative."""
    M, T = Xf.shape
    xb = np.zeros(((taps + 1) * M, T), dtype=Xf.dtype)
    xb[:M] = Xf
    for j in range(1, taps + 1):
        shift = delay + j - 1
        if shift < T:
            xb[j * M:(j + 1) * M, shift:] = Xf[:, :T - shift]
    return xb


def masked_covariance(Xf, m):
    """Phi_s of one (bin, source): Xf (M, T), m (T,), in the dtype of Xf."""
    real = Xf.real.dtype.type
    m = np.asarray(m, dtype=Xf.real.dtype)
    S = (Xf * m[None, :]) @ np.conj(Xf.T)
    return S / max(m.sum(), real(EPS))


def power(y, flooring):
    pw = y.real ** 2 + y.imag ** 2
    return wpe_numpy.floor(pw, flooring), pw


def bin_loss(y, flooring):
    """sum_t [log lambda_t + |y_t|^2 / lambda_t] / T of one (bin, source)."""
    lam, pw = power(y, flooring)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sum(np.log(lam) + pw / lam) / y.shape[0]


def weighted_covariance(xb, lam, loading):
    """R of one iteration, loading included."""
    Lb, T = xb.shape
    real = xb.real.dtype.type
    with np.errstate(divide="ignore", invalid="ignore"):
        R = (xb / lam[None, :]) @ np.conj(xb.T) / real(T)
    return R + real(loading) * (np.trace(R).real / Lb) * np.eye(Lb, dtype=xb.dtype)


def _usable(den):
    return bool(np.isfinite(den.real) and np.isfinite(den.imag) and den != 0)


def bin_step(xb, wb, M, flooring, loading, extended, Phi_s=None, v=None, ref=0):
    """One iteration on one (bin, source): (the new wb, what it was formed from).  Raises
    LinAlgError on a pivot that is not positive and finite."""
    ctype = xb.dtype
    Lb = xb.shape[0]
    lam, _ = power(np.conj(wb) @ xb, flooring)
    R = weighted_covariance(xb, lam, loading)
    if v is None:
        rhs = np.zeros((Lb, M), dtype=ctype)
        rhs[:M] = np.eye(M, dtype=ctype)
    else:
        rhs = np.zeros((Lb, 1), dtype=ctype)
        rhs[:M, 0] = v
    if extended:
        U = wpe_numpy.cholesky_upper(R)
        Z = wpe_numpy.solve_cholesky(U, rhs)
    else:
        if not np.all(np.isfinite(R)):
            raise np.linalg.LinAlgError("R is not finite")
        U = np.conj(np.linalg.cholesky(R).T)
        if not np.all(np.isfinite(U)):
            raise np.linalg.LinAlgError("pivot not finite")
        Z = np.linalg.solve(U, np.linalg.solve(np.conj(U.T), rhs))
    new = np.zeros(Lb, dtype=ctype)
    if v is None:
        A = Z @ Phi_s
        den = np.trace(A[:M]).real
        if _usable(den):
            new = A[:, ref] / den
    else:
        a = Z[:, 0]
        den = np.conj(v) @ a[:M]
        if _usable(den):
            new = a * np.conj(v[ref]) / den
    return new, {"lambda": lam, "R": R, "U": U}


def run(X, mask=None, taps=5, delay=3, n_iter=3, ref=0, loading=LOADING, flooring=MAX_FLOOR,
        steering_vector=None, dtype=np.float64, convolutional_filter=None, statistics=False):
    """X (M, F, T) or (B, M, F, T), mask (N, F, T) or (B, N, F, T), steering_vector (F, N, M) or
    (B, F, N, M).  Returns ``output`` (N, F, T), ``convolutional_filter`` (F, N, K + 1, M),
    ``signal_covariance`` (F, N, M, M) (mask form), ``loss``: n_iter + 1 entries, floats or (B,)
    arrays, and ``failed``; with ``statistics`` also lambda (F, N, T), R and U (F, N, Lb, Lb) of the
    LAST iteration.  All with the leading mixture axis of X."""
    ctype = _complex(dtype)
    extended = ctype is np.clongdouble
    X = np.asarray(X)
    batched = X.ndim == 4
    X4 = (X if batched else X[None]).astype(ctype)
    B, M, F, T = X4.shape
    V4 = m4 = None
    if steering_vector is not None:
        V4 = np.asarray(steering_vector)
        V4 = (V4 if batched else V4[None]).astype(ctype)
        N = V4.shape[2]
    else:
        m4 = np.asarray(mask)
        m4 = (m4 if batched else m4[None]).astype(dtype)
        N = m4.shape[1]
    Lb = (taps + 1) * M
    W = np.zeros((B, F, N, Lb), dtype=ctype)  # conj(wb)
    if convolutional_filter is None:
        W[..., ref] = 1
    else:
        W[...] = np.asarray(convolutional_filter).reshape(B, F, N, Lb)
    Y = np.zeros((B, N, F, T), dtype=ctype)
    Phi = np.zeros((B, F, N, M, M), dtype=ctype)
    loss = np.zeros((n_iter + 1, B), dtype=dtype)
    stats = {"lambda": np.zeros((B, F, N, T), dtype), "R": np.zeros((B, F, N, Lb, Lb), ctype),
             "U": np.zeros((B, F, N, Lb, Lb), ctype)}
    failed = 0
    for b in range(B):
        for f in range(F):
            Xf = X4[b, :, f, :]
            xb = stack(Xf, taps, delay)
            for n in range(N):
                wb = np.conj(W[b, f, n])
                v = Phi_s = None
                if V4 is not None:
                    v = V4[b, f, n]
                else:
                    Phi_s = Phi[b, f, n] = masked_covariance(Xf, m4[b, n, f])
                loss[0, b] += bin_loss(np.conj(wb) @ xb, flooring)
                alive = True
                for it in range(n_iter):
                    if alive:
                        try:
                            wb, st = bin_step(xb, wb, M, flooring, loading, extended, Phi_s, v, ref)
                            if it == n_iter - 1:
                                for key in stats:
                                    stats[key][b, f, n] = st[key]
                        except np.linalg.LinAlgError:
                            alive = False
                            failed += 1
                    loss[it + 1, b] += bin_loss(np.conj(wb) @ xb, flooring)
                W[b, f, n] = np.conj(wb)
                Y[b, n, f, :] = np.conj(wb) @ xb
    result = {"output": Y, "convolutional_filter": W.reshape(B, F, N, taps + 1, M),
              "signal_covariance": Phi}
    result.update(stats if statistics else {})
    if not batched:
        result = {k: v[0] for k, v in result.items()}
    result["loss"] = [row.copy() if batched else row[0] for row in loss]
    result["failed"] = failed
    return result
