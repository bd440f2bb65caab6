"""Extended-precision reference of ``prox.neg_logdet``: a one-sided (Hestenes) complex Jacobi in
``np.clongdouble`` (80-bit on x86), written for this project -- what tests/pass_reference.py is for
the passes.  ``prox(X) = sum_k g_k (f(sigma_k) / sigma_k) v_k^H`` with ``G = X V`` of orthogonal
columns, ``sigma_k = |g_k|`` and ``f(s) = (s + sqrt(s^2 + 4 mu)) / 2``; a vanishing column is replaced
by a unit vector orthogonal to the others (the result is not determined there; it is finite and has
the singular values ``f(sigma)``).  ``dtype=np.complex128`` runs the same statements in fp64."""

import numpy as np

MAX_SWEEPS = 60


def _real(dtype):
    return np.zeros(1, dtype=dtype).real.dtype.type


def neg_logdet_one(X, step_size=1, dtype=np.clongdouble):
    """One N x N matrix."""
    real = _real(dtype)
    eps = np.finfo(real).eps
    A = np.array(X, dtype=dtype)
    N = A.shape[0]
    mu = real(step_size)
    amax = max(np.max(np.abs(A.real)), np.max(np.abs(A.imag))) if A.size else real(0)
    ex = int(np.frexp(np.float64(amax))[1]) if amax > 0 and np.isfinite(amax) else 0
    A = A * real(2.0) ** (-ex)
    V = np.eye(N, dtype=dtype)
    tol2 = (8 * eps) ** 2
    for _ in range(MAX_SWEEPS):
        rotated = False
        for p in range(N - 1):
            for q in range(p + 1, N):
                gp, gq = A[:, p].copy(), A[:, q].copy()
                alpha, beta = np.vdot(gp, gp).real, np.vdot(gq, gq).real
                gamma = np.vdot(gp, gq)  # g_p^H g_q
                mag = np.abs(gamma)
                if not (mag * mag > tol2 * alpha * beta and mag > 0):
                    continue
                rotated = True
                u = gamma / mag
                tau = (beta - alpha) / (2 * mag)
                t = np.sign(tau) / (np.abs(tau) + np.sqrt(1 + tau * tau)) if tau != 0 else real(1)
                c = 1 / np.sqrt(1 + t * t)
                s = t * c
                # g_p' = c g_p - s conj(u) g_q ; g_q' = s u g_p + c g_q, and the same on V
                A[:, p], A[:, q] = c * gp - s * np.conj(u) * gq, s * u * gp + c * gq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * np.conj(u) * vq, s * u * vp + c * vq
        if not rotated:
            break
    sv = np.sqrt(np.sum(np.abs(A) ** 2, axis=0))
    stands = sv >= real(1e-70)
    U = np.zeros_like(A)
    U[:, stands] = A[:, stands] / sv[stands]
    for k in np.nonzero(~stands)[0]:
        res = 1 - np.sum(np.abs(U[:, stands]) ** 2, axis=1)
        w = np.zeros(N, dtype=dtype)
        w[int(np.argmax(res))] = 1
        for _ in range(2):
            for c in np.nonzero(stands)[0]:
                w = w - U[:, c] * np.vdot(U[:, c], w)
        U[:, k] = w / np.sqrt(np.vdot(w, w).real)
        sv[k] = 0
        stands[k] = True
    s = sv * real(2.0) ** ex
    f = (s + np.sqrt(s * s + 4 * mu)) / 2
    return (U * f) @ V.conj().T


def neg_logdet(X, step_size=1, dtype=np.clongdouble):
    """Batches (..., N, N); returns the extended dtype."""
    X = np.asarray(X)
    flat = X.reshape((-1,) + X.shape[-2:])
    out = np.stack([neg_logdet_one(x, step_size, dtype) for x in flat]) if len(flat) else \
        np.zeros(flat.shape, dtype=dtype)
    return out.reshape(X.shape)


def neg_logdet_svd(X, step_size=1):
    """The fp64 SVD form of the reference's statement (numpy.linalg.svd)."""
    U, s, Vh = np.linalg.svd(X)
    f = (s + np.sqrt(s**2 + 4 * step_size)) / 2
    return (U * f[..., None, :]) @ Vh


def with_singular_values(rng, N, sigma):
    """A random complex N x N matrix with the singular values ``sigma``."""
    def unitary():
        Q, R = np.linalg.qr(rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)))
        d = np.diagonal(R)
        return Q * (d / np.abs(d))
    return (unitary() * np.asarray(sigma, dtype=np.float64)) @ unitary().conj().T


def graded(kappa, N):
    """N singular values from 1 down to 1 / kappa, geometrically spaced."""
    return np.ones(1) if N == 1 else kappa ** (-np.arange(N) / (N - 1.0))
