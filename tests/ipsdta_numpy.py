"""NumPy restatement of block-decomposed IPSDTA (GaussIPSDTA, TIPSDTA; MM + VCD), from the equations.

    R_ntc = psd(sum_k v_nkt T_nkc)                 psd: Hermitise, floor the eigenvalues at 1e-10
    pi_nt = (nu + 2F) / (nu + 2 sum_c max(y^H R^-1 y, 0))            (t model; 1 for the Gaussian)
    P = mean_t v R^-1,  Q = mean_t v pi u u^H,  u = R^-1 y
    Gauss: T <- psd_f(psd_f(P)^-1 # psd_f(T Q T));   t: T <- psd_f(T Q' (Q' T P T Q')^-1/2 Q' T)
    v <- v sqrt(sum_c pi Re(u^H T u) / sum_c Re tr(R^-1 T)),  then (T, v) <- (T / tr, v tr)
    VCD row updates from mean_t pi R^-1[b, a] x_a x_b^H,  loss as in the papers.

Shared by the CPU replay of the fixtures and the GPU tests.  ``dtype`` arguments allow the 80-bit
types for the kernel-by-kernel comparisons (no LAPACK there: Gauss-Jordan inverses).
"""

import numpy as np

PSD_EPS = 1e-10


def herm(A):
    return (A + np.conj(np.swapaxes(A, -2, -1))) / 2


def psd(A, floor=None):
    """Hermitise, floor the eigenvalues (default: at 1e-10), rebuild, Hermitise."""
    lam, P = np.linalg.eigh(herm(A))
    lam = np.maximum(lam, PSD_EPS) if floor is None else floor(lam)
    return herm((P * lam[..., None, :]) @ np.conj(np.swapaxes(P, -2, -1)))


def herm_fn(A, fn):
    lam, P = np.linalg.eigh(A)
    return (P * fn(lam)[..., None, :]) @ np.conj(np.swapaxes(P, -2, -1))


def gmean_inv_a(A, B):
    """A^-1 # B = A^-1/2 (A^1/2 B A^1/2)^1/2 A^-1/2."""
    Ah = herm_fn(A, np.sqrt)
    Aih = herm_fn(A, lambda x: 1 / np.sqrt(x))
    return Aih @ herm_fn(herm(Ah @ B @ Ah), np.sqrt) @ Aih


def inverse(A):
    """Inverse of stacks of small matrices in the dtype of A (Gauss-Jordan, partial pivoting)."""
    if A.dtype in (np.complex128, np.float64):
        return np.linalg.inv(A)
    n = A.shape[-1]
    M = np.concatenate([A, np.broadcast_to(np.eye(n, dtype=A.dtype), A.shape)], axis=-1).copy()
    M = M.reshape((-1, n, 2 * n))
    idx = np.arange(M.shape[0])
    for k in range(n):
        p = k + np.argmax(np.abs(M[:, k:, k]), axis=1)
        rk, rp = M[idx, k].copy(), M[idx, p].copy()
        M[idx, k], M[idx, p] = rp, rk
        M[:, k] = M[:, k] / M[:, k, k][:, None]
        for r in range(n):
            if r != k:
                M[:, r] = M[:, r] - M[:, r, k][:, None] * M[:, k]
    return M[:, :, n:].reshape(A.shape)


def logdet_hpd(A):
    """log det of Hermitian positive definite stacks in the dtype of A (Cholesky pivots)."""
    n = A.shape[-1]
    M = A.copy()
    total = 0
    for k in range(n):
        d = np.real(M[..., k, k])
        total = total + np.log(d)
        col = M[..., k + 1:, k] / d[..., None]
        M[..., k + 1:, k + 1:] = M[..., k + 1:, k + 1:] - col[..., :, None] * M[..., k, k + 1:][..., None, :]
    return total


def cond2_hpd(A, Ainv, sweeps=80):
    """lam_max(A) lam_max(A^-1) of Hermitian positive definite stacks by power iterations in the
    dtype of A (approached from below)."""
    def top(M):
        v = np.ones(M.shape[:-1], dtype=M.dtype)
        for _ in range(sweeps):
            v = np.einsum("...ab,...b->...a", M, v)
            v = v / np.sqrt(np.sum(np.abs(v) ** 2, axis=-1, keepdims=True))
        return np.real(np.einsum("...a,...ab,...b->...", np.conj(v), M, v))
    return top(A) * top(Ainv)


def split_sizes(n_bins, n_blocks):
    """[(first bin, first block, number of blocks, block size)] of the low and the high partition."""
    L, rem = n_bins // n_blocks, n_bins % n_blocks
    parts = [(0, 0, n_blocks - rem, L)]
    if rem:
        parts.append(((n_blocks - rem) * L, n_blocks - rem, rem, L + 1))
    return parts


def as_parts(basis):
    return list(basis) if isinstance(basis, tuple) else [basis]


def blocks_of(A, part, axis):
    """The bins of a partition along ``axis`` reshaped to (blocks, size)."""
    f0, _, C, L = part
    A = np.take(A, np.arange(f0, f0 + C * L), axis=axis)
    return A.reshape(A.shape[:axis] + (C, L) + A.shape[axis + 1:])


def frame_quantities(X, W, T, V, part, floored=True):
    """y (N, t, C, L), R, R^-1 (N, t, C, L, L), u = R^-1 y of one partition; T (N, K, C, L, L)."""
    Y = np.einsum("fnm,mft->nft", W, X)
    y = np.transpose(blocks_of(Y, part, 1), (0, 3, 1, 2))
    R = np.einsum("nkcab,nkt->ntcab", T, V)
    R = psd(R) if floored else herm(R)
    Rinv = inverse(R)
    u = np.einsum("ntcab,ntcb->ntca", Rinv, y)
    return y, R, Rinv, u


def quadratic_forms(X, W, basis, V, parts):
    """[Re(y^H R^-1 y)] and [log det R], each (N, t, C) per partition."""
    quads, logdets = [], []
    for T, part in zip(as_parts(basis), parts):
        y, R, _, u = frame_quantities(X, W, T, V, part)
        quads.append(np.real(np.einsum("ntca,ntca->ntc", np.conj(y), u)))
        logdets.append(np.linalg.slogdet(R)[1])
    return quads, logdets


def t_weight(quads, dof, n_bins):
    s = sum(np.maximum(q, 0).sum(axis=-1) for q in quads)
    return (dof + 2 * n_bins) / (dof + 2 * s), s


def vcd_row(W, RXX, i, n, threshold=0.0, details=None):
    """Row (bin i of every block, source n) of the VCD sweep from the state W (C, L, N, M), in the
    dtype of W; the solves go through ``inverse`` (80-bit capable).  ``details``: a dict that
    receives the intermediate quantities."""
    C, L, N, M = W.shape
    U = RXX[:, i, i, n]
    terms = [np.einsum("cab,cb->ca", RXX[:, i, l, n], np.conj(W[:, l, n])) for l in range(L) if l != i]
    gamma = sum(terms) if terms else np.zeros((C, M), dtype=W.dtype)
    WU = W[:, i] @ U
    WUinv, Uinv = inverse(WU), inverse(U)
    eta = WUinv[:, :, n]
    eta_hat = np.einsum("cab,cb->ca", Uinv, gamma)
    eU = np.einsum("ca,cab->cb", np.conj(eta), U)
    xi = np.maximum(np.real(np.sum(eU * eta, axis=-1)), 0)
    xi_hat = np.sum(eU * eta_hat, axis=-1)
    sing = np.abs(xi_hat) < threshold
    xi_hat = np.where(sing, 1, xi_hat)
    with np.errstate(all="ignore"):
        coeff = xi_hat / (2 * xi) * (1 - np.sqrt(1 + 4 * xi / np.abs(xi_hat) ** 2))
        coeff = np.where(sing, 1 / np.sqrt(xi), coeff)
    if details is not None:
        details.update(U=U, Uinv=Uinv, WU=WU, WUinv=WUinv, gamma=gamma, terms=terms, eta=eta,
                       eta_hat=eta_hat, xi=xi, xi_hat=xi_hat, coeff=coeff, sing=sing)
    return np.conj(coeff[:, None] * eta - eta_hat)


def vcd(W, RXX, threshold=0.0):
    """The VCD sweep on W (C, L, N, M) from RXX (C, L, L, N, M, M); returns the new W."""
    W = W.copy()
    C, L, N, M = W.shape
    for i in range(L):
        for n in range(N):
            U = RXX[:, i, i, n]
            gamma = np.zeros((C, M), dtype=W.dtype)
            for l in range(L):
                if l != i:
                    gamma += np.einsum("cab,cb->ca", RXX[:, i, l, n], np.conj(W[:, l, n]))
            e = np.zeros((C, N, 1), dtype=W.dtype)
            e[:, n] = 1
            eta = np.linalg.solve(W[:, i] @ U, e)[..., 0]
            eta_hat = np.linalg.solve(U, gamma[..., None])[..., 0]
            eU = np.einsum("ca,cab->cb", np.conj(eta), U)
            xi = np.maximum(np.real(np.sum(eU * eta, axis=-1)), 0)
            xi_hat = np.sum(eU * eta_hat, axis=-1)
            sing = np.abs(xi_hat) < threshold
            xi_hat = np.where(sing, 1, xi_hat)
            with np.errstate(all="ignore"):
                coeff = xi_hat / (2 * xi) * (1 - np.sqrt(1 + 4 * xi / np.abs(xi_hat) ** 2))
                coeff = np.where(sing, 1 / np.sqrt(xi), coeff)
            W[:, i, n] = np.conj(coeff[:, None] * eta - eta_hat)
    return W


class IPSDTA:
    """One separator: ``dof=None`` is GaussIPSDTA, a number TIPSDTA."""

    def __init__(self, n_basis, n_blocks, dof=None, floor=None, threshold=PSD_EPS,
                 source_normalization=True, scale_restoration=True, reference_id=0, rng=None):
        self.n_basis, self.n_blocks, self.dof = n_basis, n_blocks, dof
        # floor: the flooring function on eigenvalues / activations; threshold: flooring_fn(0)
        self.floor = (lambda x: np.maximum(x, PSD_EPS)) if floor is None else floor
        self.threshold = threshold
        self.source_normalization = source_normalization
        self.scale_restoration, self.reference_id = scale_restoration, reference_id
        self.rng = np.random.default_rng() if rng is None else rng

    # -- state
    def reset(self, X, demix_filter=None, basis=None, activation=None):
        self.X = np.array(X, dtype=np.complex128)
        N, F, T = self.X.shape
        self.parts = split_sizes(F, self.n_blocks)
        self.W = (np.tile(np.eye(N, dtype=np.complex128), (F, 1, 1)) if demix_filter is None
                  else np.array(demix_filter, dtype=np.complex128))
        if basis is None:
            mats = []
            for _, _, C, L in self.parts:
                mats.append(self.rng.random((N, self.n_basis, C, L))[..., None] * np.eye(L) + 0j)
            basis = tuple(mats) if len(mats) > 1 else mats[0]
        self.basis = tuple(np.array(t) for t in basis) if isinstance(basis, tuple) else np.array(basis)
        if activation is None:
            activation = self.floor(self.rng.random((N, self.n_basis, T)))
        self.V = np.array(activation, dtype=np.float64)
        if self.source_normalization:
            self.normalize()
        self.loss = []

    def _set_basis(self, mats):
        self.basis = tuple(mats) if len(mats) > 1 else mats[0]

    def normalize(self):
        mats = as_parts(self.basis)
        trace = sum(np.real(np.trace(t, axis1=-2, axis2=-1)).sum(axis=-1) for t in mats)
        self._set_basis([t / trace[:, :, None, None, None] for t in mats])
        self.V = self.V * trace[:, :, None]

    def weight(self):
        if self.dof is None:
            return np.ones(self.V.shape[::2])
        quads, _ = quadratic_forms(self.X, self.W, self.basis, self.V, self.parts)
        return t_weight(quads, self.dof, self.X.shape[1])[0]

    # -- the three stages of an iteration, each on freshly rebuilt R
    def update_basis(self):
        pi, new = self.weight(), []
        for T, part in zip(as_parts(self.basis), self.parts):
            _, _, Rinv, u = frame_quantities(self.X, self.W, T, self.V, part)
            uu = np.einsum("ntca,ntcb->ntcab", u, np.conj(u))
            P = np.einsum("nkt,ntcab->nkcab", self.V, Rinv) / self.V.shape[-1]
            Q = np.einsum("nkt,nt,ntcab->nkcab", self.V, pi, uu) / self.V.shape[-1]
            if self.dof is None:
                G = gmean_inv_a(psd(P, self.floor), psd(T @ Q @ T, self.floor))
            else:
                Qh = herm_fn(psd(Q, self.floor), np.sqrt)
                mid = psd(Qh @ T @ P @ T @ Qh, self.floor)
                G = T @ Qh @ herm_fn(mid, lambda x: 1 / self.floor(np.sqrt(x))) @ Qh @ T
            new.append(psd(G, self.floor))
        self._set_basis(new)

    def update_activation(self):
        pi, num, den = self.weight(), 0, 0
        for T, part in zip(as_parts(self.basis), self.parts):
            _, _, Rinv, u = frame_quantities(self.X, self.W, T, self.V, part)
            num = num + np.real(np.einsum("ntca,nkcab,ntcb,nt->nkt", np.conj(u), T, u, pi))
            den = den + np.real(np.einsum("ntcab,nkcba->nkt", Rinv, T))
        self.V = self.V * np.sqrt(num / den)

    def weighted_covariances(self):
        pi, out = self.weight(), []
        for T, part in zip(as_parts(self.basis), self.parts):
            _, _, Rinv, _ = frame_quantities(self.X, self.W, T, self.V, part)
            x = blocks_of(self.X, part, 1)  # (M, C, L, t)
            out.append(np.einsum("nt,ntcba,pcat,qcbt->cabnpq", pi, Rinv, x, np.conj(x))
                       / self.V.shape[-1])
        return out

    def update_spatial(self):
        W = self.W.copy()
        for RXX, (f0, _, C, L) in zip(self.weighted_covariances(), self.parts):
            blk = W[f0:f0 + C * L].reshape((C, L) + W.shape[1:])
            W[f0:f0 + C * L] = vcd(blk, RXX, self.threshold).reshape((C * L,) + W.shape[1:])
        self.W = W

    def update_once(self):
        self.update_basis()
        self.update_activation()
        if self.source_normalization:
            self.normalize()
        self.update_spatial()

    def compute_loss(self):
        quads, logdets = quadratic_forms(self.X, self.W, self.basis, self.V, self.parts)
        logdet_r = sum(ld.sum(axis=(0, 2)) for ld in logdets)
        if self.dof is None:
            data = sum(np.maximum(q.sum(axis=(0, 2)), 0) for q in quads)
        else:
            _, s = t_weight(quads, self.dof, self.X.shape[1])
            data = np.sum((self.dof + 2 * self.X.shape[1]) / 2 * np.log(1 + 2 / self.dof * s), axis=0)
        return float(np.mean(data + logdet_r) - 2 * np.linalg.slogdet(self.W)[1].sum())

    def output(self):
        return np.einsum("fnm,mft->nft", self.W, self.X)

    def restore_scale(self):
        how = self.scale_restoration
        if how is True or how == "projection_back":
            scale = np.linalg.inv(self.W)[:, self.reference_id, :]
            self.W = self.W * scale[:, :, None]
        elif how == "minimal_distortion_principle":
            Y = self.output()
            ref = self.X[self.reference_id]
            z = np.sum(np.conj(Y) * ref, axis=-1) / np.sum(np.abs(Y) ** 2, axis=-1)
            Ys = (z[..., None] * Y).transpose(1, 0, 2)
            Xf = self.X.transpose(1, 0, 2)
            XH = np.conj(Xf.transpose(0, 2, 1))
            self.W = Ys @ XH @ np.linalg.inv(Xf @ XH)
        elif how:
            raise ValueError(how)

    def run(self, X, n_iter, record_loss=True, callback=None, **state):
        self.reset(X, **state)
        if record_loss:
            self.loss.append(self.compute_loss())
        for _ in range(n_iter):
            self.update_once()
            if record_loss:
                self.loss.append(self.compute_loss())
            if callback is not None:
                callback(self)
        self.restore_scale()
        return self.output()
