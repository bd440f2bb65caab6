"""NumPy restatement of CACGMM and of the two permutation solvers, and the shared test mixtures.

Written from the algorithm (Ito, Araki, Nakatani, EUSIPCO 2016; Sawada et al. 2010; Murata et al.
2001) and the documented behaviour of the reference, in the plainest form: every quantity of an
iteration is an explicit array, the solvers score one permutation at a time.  It is the CPU stand-in
for the reference in the GPU tests (tests/test_golden_cacgmm.py pins it to the reference's
fixtures).
"""

import functools
import itertools

import numpy as np

# (M, N, F, T) of the test mixtures
CASES = [(2, 2, 1025, 37), (2, 3, 9, 40), (3, 3, 17, 60), (3, 4, 17, 80), (4, 2, 1, 50),
         (4, 4, 33, 100), (5, 3, 7, 64), (6, 3, 9, 120), (7, 5, 5, 130), (8, 8, 5, 200),
         (8, 16, 3, 300)]

# the fixtures of tests/golden/make_golden_cacgmm.py: name -> (case, options).  There is none for
# permutation_alignment="posterior_correlation": the reference accepts the value and then fails in
# solve_permutation_by_correlation ("Only amplitude is supported as target.").
GOLDEN = {
    "cacgmm_noperm_m3_n3": ((3, 3, 17, 60), dict(permutation_alignment=False)),
    "cacgmm_true_m2_n2": ((2, 2, 33, 37), dict(permutation_alignment=True)),
    "cacgmm_pscore_m3_n4": ((3, 4, 17, 80), dict(permutation_alignment="posterior_score")),
    "cacgmm_pscore_g2l2_m4_n4": ((4, 4, 33, 100), dict(permutation_alignment="posterior_score",
                                                         global_iter=2, local_iter=2)),
    "cacgmm_ascore_m2_n3": ((2, 3, 9, 40), dict(permutation_alignment="amplitude_score")),
    "cacgmm_acorr_m5_n3": ((5, 3, 7, 64), dict(permutation_alignment="amplitude_correlation")),
    "cacgmm_nonorm_m4_n2": ((4, 2, 1, 50), dict(permutation_alignment=False, normalization=False)),
    "cacgmm_addfloor_m6_n3": ((6, 3, 9, 120), dict(permutation_alignment="amplitude_correlation",
                                                    flooring=("add", 1e-8))),
    "cacgmm_nofloor_m2_n3": ((2, 3, 9, 40), dict(permutation_alignment=False, flooring=None)),
    "cacgmm_ref1_m7_n5": ((7, 5, 5, 130), dict(permutation_alignment="amplitude_correlation",
                                                reference_id=1)),
    "cacgmm_m8_n8": ((8, 8, 5, 200), dict(permutation_alignment=False)),
}

N_ITER = 5


def make_mixture(M, N, F, T, seed=None):
    """The test mixture of a case: sparse sources through random mixing, plus noise."""
    rng = np.random.default_rng(700 + 10 * M + N if seed is None else seed)

    def cn(shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)

    S = cn((N, F, T)) * rng.gamma(1.0, 1.0, (N, F, T))
    A = cn((F, M, N))
    return np.einsum("fmn,nft->mft", A, S) + 0.5 * cn((M, F, T))


def max_flooring(x, eps=1e-10):
    return np.maximum(x, eps)


def add_flooring(x, eps=1e-10):
    return x + eps


def flooring_of(spec):
    """("max" | "add", eps) or None -> callable or None."""
    if spec is None:
        return None
    kind, eps = spec
    return functools.partial(max_flooring if kind == "max" else add_flooring, eps=eps)


# ---------------------------------------------------------------------------- the solvers
def correlation_solver(Y, *args, flooring_fn=functools.partial(max_flooring, eps=1e-10)):
    """Murata et al.: bins from the least to the most self-correlated, each permuted to correlate
    best with the running sum of the aligned envelopes.  Returns copies."""
    floor = (lambda x: x) if flooring_fn is None else flooring_fn
    Y = Y.copy()
    args = [a.copy() for a in args]
    F, N, _ = Y.shape
    P = np.abs(Y)
    P = P / floor(np.sqrt(np.sum(P ** 2, axis=1, keepdims=True)))
    order = np.argsort(np.sum(P @ P.transpose(0, 2, 1), axis=(1, 2)))
    criterion = P[order[0]]
    for f in order[1:]:
        best, best_perm = None, None
        for perm in itertools.permutations(range(N)):
            value = np.sum(criterion * P[f, perm, :])
            if best is None or value > best:
                best, best_perm = value, perm
        criterion = criterion + P[f, best_perm, :]
        Y[f] = Y[f, best_perm]
        for a in args:
            a[f] = a[f, best_perm]
    return Y, args


def _score(block, anchors, denom):
    """Score of one ordering: block (N, T) against anchors (K, N, T)."""
    corr = np.mean(block[np.newaxis, :, np.newaxis, :] * anchors[:, np.newaxis, :, :], axis=-1)
    corr = corr / denom  # (N, 1): the row of the permuted component
    eye = np.eye(block.shape[0])
    return np.sum(eye * corr - (1 - eye) * corr)


def score_solver(seq, *args, global_iter=1, local_iter=1,
                 flooring_fn=functools.partial(max_flooring, eps=1e-10)):
    """Sawada et al.: global alignment to the centroid, then local alignment to neighbours and
    (sub)harmonics.  Returns copies."""
    floor = (lambda x: x) if flooring_fn is None else flooring_fn
    seq = seq.copy()
    args = [a.copy() for a in args]
    F, N, _ = seq.shape
    perms = list(itertools.permutations(range(N)))
    Z = (seq - seq.mean(axis=-1, keepdims=True)) / seq.std(axis=-1, keepdims=True)
    for _ in range(global_iter):
        centroid = Z.mean(axis=0)
        denom = floor(centroid.std(axis=-1, keepdims=True))
        for f in range(F):
            scores = [_score(Z[f, perm, :], centroid[np.newaxis], denom) for perm in perms]
            perm = perms[int(np.argmax(scores))]
            Z[f], seq[f] = Z[f, perm], seq[f, perm]
            for a in args:
                a[f] = a[f, perm]
    for _ in range(local_iter):
        for f in range(F):
            idx = set(range(max(0, f - 3), f)) | set(range(f + 1, min(F - 1, f + 3) + 1))
            idx |= set(range(max(0, f // 2 - 1), min(F - 1, f // 2 + 1) + 1))
            idx |= set(range(max(0, 2 * f - 1), min(F - 1, 2 * f + 1) + 1))
            anchors = Z[sorted(idx)]
            scores = [_score(Z[f, perm, :], anchors, denom) for perm in perms]
            perm = perms[int(np.argmax(scores))]
            Z[f], seq[f] = Z[f, perm], seq[f, perm]
            for a in args:
                a[f] = a[f, perm]
    return seq, args


# ---------------------------------------------------------------------------- the model
def unit_input(X, flooring_fn):
    floor = (lambda x: x) if flooring_fn is None else flooring_fn
    return X / floor(np.linalg.norm(X, axis=0))


def init_parameters(rng, N, F, M):
    """alpha, then the diagonals, from the same generator (the reference's draw order)."""
    alpha = rng.random((N, F))
    alpha = alpha / alpha.sum(axis=0)
    diag = rng.random((N, F, M))
    diag = diag / diag.sum(axis=-1, keepdims=True)
    return alpha, diag[..., np.newaxis] * np.eye(M, dtype=np.complex128)


def quadratic(Z, B, flooring_fn):
    """floor(max(Re z^H B^-1 z, 0)), (N, F, T)."""
    floor = (lambda x: x) if flooring_fn is None else flooring_fn
    Binv = np.linalg.inv(B)
    q = np.einsum("mft,nfmk,kft->nft", Z.conj(), Binv, Z).real
    return floor(np.maximum(q, 0))


def log_posterior(Z, alpha, B, flooring_fn):
    M = Z.shape[0]
    q = quadratic(Z, B, flooring_fn)
    _, logdet = np.linalg.slogdet(B)
    return (np.log(alpha) - logdet)[:, :, np.newaxis] - M * np.log(q), q


def e_step(Z, alpha, B, flooring_fn):
    lg, _ = log_posterior(Z, alpha, B, flooring_fn)
    e = np.exp(lg - lg.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def to_psd(B, flooring_fn):
    floor = (lambda x: x) if flooring_fn is None else flooring_fn
    B = (B + B.swapaxes(-2, -1).conj()) / 2
    lam, P = np.linalg.eigh(B)
    B = (P * floor(lam)[..., np.newaxis, :]) @ P.swapaxes(-2, -1).conj()
    return (B + B.swapaxes(-2, -1).conj()) / 2


def m_step(Z, B, gamma, flooring_fn):
    M, _, T = Z.shape
    q = quadratic(Z, B, flooring_fn)
    w = gamma / q
    num = np.einsum("nft,mft,kft->nfmk", w, Z, Z.conj())
    denom = gamma.sum(axis=-1)
    B = to_psd(M * (num / denom[:, :, np.newaxis, np.newaxis]), flooring_fn)
    return gamma.mean(axis=-1), B


def normalize(B):
    return B / np.trace(B, axis1=-2, axis2=-1).real[..., np.newaxis, np.newaxis]


def loss_of(Z, alpha, B, flooring_fn):
    lg, _ = log_posterior(Z, alpha, B, flooring_fn)
    vmax = lg.max(axis=0, keepdims=True)
    lse = np.log(np.exp(lg - vmax).sum(axis=0)) + vmax[0]
    return float((-lse).mean(axis=-1).sum())


def align(X, alpha, B, gamma, how, reference_id=0, global_iter=1, local_iter=1, flooring_fn=None,
          score=score_solver, correlation=correlation_solver):
    """Permutation alignment of a finished run; returns (alpha, B, gamma, perm (F, N))."""
    N, F = alpha.shape
    if how is True:
        how = "posterior_score"
    a, c, g = alpha.T, B.transpose(1, 0, 2, 3), gamma.transpose(1, 0, 2)
    index = np.tile(np.arange(N), (F, 1))
    Y = g * X[reference_id][:, np.newaxis, :]
    kw = dict(flooring_fn=flooring_fn)
    if how == "posterior_score":
        g, (a, c, index) = score(g, a, c, index, global_iter=global_iter, local_iter=local_iter, **kw)
    elif how == "amplitude_score":
        _, (a, c, g, index) = score(np.abs(Y), a, c, g, index, global_iter=global_iter,
                                    local_iter=local_iter, **kw)
    elif how == "posterior_correlation":
        raise AssertionError("Only amplitude is supported as target.")
    elif how == "amplitude_correlation":
        _, (a, c, g, index) = correlation(Y, a, c, g, index, **kw)
    else:
        raise ValueError(how)
    return a.T, c.transpose(1, 0, 2, 3), g.transpose(1, 0, 2), index


def run(X, rng, n_sources=None, n_iter=N_ITER, flooring=("max", 1e-10), normalization=True,
        permutation_alignment=False, reference_id=0, global_iter=1, local_iter=1, initial_call=True):
    """A CACGMM call.  Returns a dict: per-iteration ``mixing`` / ``covariance`` snapshots (index 0
    the initial parameters), ``loss`` list, and the final ``posterior``, ``output``, ``permutation``
    (None without alignment) and the aligned ``mixing`` / ``covariance`` as ``final_*``."""
    fn = flooring_of(flooring)
    M, F, T = X.shape
    N = M if n_sources is None else n_sources
    Z = unit_input(X, fn)
    alpha, B = init_parameters(rng, N, F, M)
    mixing, covariance, loss = [alpha], [B], []
    if initial_call:
        loss.append(loss_of(Z, alpha, B, fn))
    for _ in range(n_iter):
        gamma = e_step(Z, alpha, B, fn)
        alpha, B = m_step(Z, B, gamma, fn)
        if normalization:
            B = normalize(B)
        mixing.append(alpha)
        covariance.append(B)
        loss.append(loss_of(Z, alpha, B, fn))
    gamma = e_step(Z, alpha, B, fn)
    perm = None
    if permutation_alignment:
        alpha, B, gamma, perm = align(X, alpha, B, gamma, permutation_alignment, reference_id,
                                      global_iter, local_iter, fn)
    return dict(mixing=np.stack(mixing), covariance=np.stack(covariance), loss=np.array(loss),
                posterior=gamma, output=gamma * X[reference_id], permutation=perm,
                final_mixing=alpha, final_covariance=B)
