"""Extended-precision restatement of the GaussMNMF entry points (full-rank spatial model), with bars.

TEST INFRASTRUCTURE ONLY.  One function per ``steps`` bit of ssspy_gmnmf_update (BASIS, ACTIVATION,
SPATIAL, NORMALIZE, LATENT; with and without ``latent``), ssspy_gmnmf_loss and ssspy_gmnmf_separate,
written from the header comments of include/ssspy_amd.h and the reference lines they cite
(ssspy/bss/mnmf.py:729-1073, special/psd.py:11-71, linalg/mean.py:6-83) in ``np.longdouble``; with
``dtype=np.float64`` the SAME formula runs in plain NumPy on np.linalg.eigh / inv
(tests/test_gmnmf_reference_cpu.py: the bars are attainable, and seven mutants of that restatement
break them).  Nothing here calls into oracle/ or reads a kernel.  Conventions of
tests/mnmf_reference.py: every function returns ``(value, bar)``.

Shapes: X (B,M,F,T) c128, spatial H (B,N,F,M,M) c128, basis (B,N,F,K), activation (B,N,K,T); with
partitioning basis (B,F,K), activation (B,K,T), latent (B,N,K).

to_psd is applied literally everywhere -- Hermitise, eigendecompose (long-double Jacobi,
mnmf_reference.eigh_jacobi), floor the eigenvalues, rebuild, Hermitise -- to R_ij = sum_n lambda H_n,
to the instantaneous covariance x x^H (its closed form c1 x x^H + c0 I is the kernels' business, not
restated here), and to P, H Q H and the geometric mean of the spatial update.

Bars.  Sums over frames, bins, bases and sources get the ``m u companion`` budgets of
pass_reference.py (a sum of n terms: n + 1).  Everything that passes through R_ij^-1 is a solve and
is scaled by a condition number:

* point quantities -- kappa = kappa_2 of the FLOORED R_ij:
    Bt = tr(R^-1 H_n):          C["Bt"]   kappa u  sum_ac |R^-1|_ac |H_n|_ca
    A  = tr(R^-1 XX R^-1 H_n):  C["A"]    kappa u  sum_ac (|R^-1| |XX| |R^-1|)_ac |H_n|_ca
    P, Q sums (every entry):    C["PQ"]   kappa u  lambda ||R^-1||_F,  lambda ||R^-1||_F^2 ||XX||_F
    loss term:                  C["loss"] kappa u  (sum_ac |R^-1|_ac |XX|_ca + M)
    filter output:              || y - y_ref ||_(over n) <= C["separate"] kappa u ||x||  per point
* spatial update -- kappa_S = max(kappa_2(P), kappa_2(H Q H)) of the floored matrices, and kappa_pt
  the largest point kappa of the bin (the solve errors of P and Q pass through the mean about one to
  one, relative):  || H - H_ref ||_F <= C["gmean"] (kappa_S + kappa_pt) u || H_ref ||_F.

C[q] = 8 x the largest error, in units of kappa u companion (the solve's share alone: the bars of
P, Q and the loss add their summation budgets on top, the yardstick does not), that the float64
restatement makes against the long-double one over the shape families of the GPU test (yardsticks(); one constant per quantity, measured
on the CPU, never against a kernel), rounded up to two digits; the CPU test measures them again and
holds them to that rule, and the GPU test file prints them into profiles/gmnmf_pass_elementwise.txt.
"""

import numpy as np

import mnmf_reference as mr
import pass_reference as pr

LD, U = pr.LD, pr.U
BASIS, ACTIVATION, SPATIAL, NORMALIZE, LATENT = 1, 2, 4, 8, 16
NOF = (pr.FLOOR_NONE, 0.0)

# 8 x the float64 yardstick, see the module docstring (MEASURED: the yardsticks themselves)
MEASURED = {"A": 19.0, "Bt": 7.9, "PQ": 3.8, "loss": 7.3, "separate": 6.2, "gmean": 6.8}
C = {k: 8.0 * v for k, v in MEASURED.items()}


def _c(dtype):
    return np.clongdouble if dtype is LD else np.complex128


def _herm(A):
    return (A + np.swapaxes(A, -1, -2).conj()) / 2


def _eigh(A, dtype):
    if dtype is LD:
        w, V = mr.eigh_jacobi(A.reshape((-1,) + A.shape[-2:]))
        return w.reshape(A.shape[:-1]), V.reshape(A.shape)
    return np.linalg.eigh(A)


def _rebuild(V, w):
    return np.einsum("...am,...m,...cm->...ac", V, w.astype(V.dtype), V.conj())


def to_psd(A, flooring, dtype=LD, hermitize=True):
    """special/psd.py:11-71.  Returns (to_psd(A), raw eigenvalues, floored eigenvalues)."""
    if hermitize:
        A = _herm(A)
    w, V = _eigh(A, dtype)
    wf = pr.floor(w, flooring)
    return _herm(_rebuild(V, wf)), w, wf


def _inv(A, dtype):
    if dtype is not LD:
        return np.linalg.inv(A)
    M = A.shape[-1]
    flat = A.reshape(-1, M, M)
    eye = np.broadcast_to(np.eye(M, dtype=A.dtype), flat.shape).copy()
    return pr.lu_solve(flat, eye)[0].reshape(A.shape)


def _funm(A, fn, dtype):
    """fn on the eigenvalues of a Hermitian A."""
    w, V = _eigh(_herm(A), dtype)
    return _rebuild(V, fn(w))


def expand(basis, activation, latent, dtype=LD):
    """The per-source pair (Teff (B,N,F,K) = z t, Vrep (B,N,K,T) = v) of partitioning."""
    if latent is None:
        return basis.astype(dtype), activation.astype(dtype)
    N = latent.shape[1]
    Te = latent.astype(dtype)[:, :, None, :] * basis.astype(dtype)[:, None]
    Vr = np.broadcast_to(activation.astype(dtype)[:, None], (activation.shape[0], N) + activation.shape[1:])
    return Te, Vr


class Points:
    """Everything the passes share per (b, i, j): lambda (B,N,F,T), the floored R, R^-1, XX (B,F,T,M,M),
    raw and floored eigenvalues of R and kappa_2 of the floored R (B,F,T).  `mutant`: see
    tests/test_gmnmf_reference_cpu.py."""

    def __init__(self, X, basis, activation, H, flooring, latent=None, dtype=LD, mutant=None):
        c = _c(dtype)
        self.dtype, self.flooring = dtype, flooring
        Te, Vr = expand(basis, activation, latent, dtype)
        if mutant == "basis":
            Te, Vr = Te[..., :-1], Vr[:, :, :-1]
        self.lam = np.einsum("bnik,bnkj->bnij", Te, Vr)
        Hc = H.astype(c)
        lam_r, H_r = (self.lam[:, :-1], Hc[:, :-1]) if mutant == "source" else (self.lam, Hc)
        Rsum = np.einsum("bnij,bniac->bijac", lam_r.astype(c), H_r)
        self.R, self.ev_raw, self.ev = to_psd(Rsum, flooring, dtype, hermitize=mutant != "hermitize")
        self.G = _inv(self.R, dtype)
        Xc = np.moveaxis(X.astype(c), 1, -1)                       # (B,F,T,M)
        self.x = Xc
        self.XX = to_psd(np.einsum("bija,bijc->bijac", Xc, Xc.conj()), flooring, dtype)[0]
        if mutant == "c0":  # the rank-one part alone: c0 I of the floored x x^H dropped
            self.XX = self.XX - dtype(flooring[1]) * np.eye(X.shape[1], dtype=c)
        self.H = Hc
        self.kappa = (self.ev.max(axis=-1) / self.ev.min(axis=-1)).astype(np.float64)
        self.K = Te.shape[-1]
        self.N = Te.shape[1]

    def traces(self):
        """A, Bt (B,N,F,T) with bars and the companions the sums are budgeted on."""
        G, XX, H = self.G, self.XX, self.H
        GXG = G @ XX @ G
        A = np.einsum("bijac,bnica->bnij", GXG, H).real
        Bt = np.einsum("bijac,bnica->bnij", G, H).real
        aH = np.abs(H).real
        compA = np.einsum("bijac,bnica->bnij", np.abs(G) @ np.abs(XX) @ np.abs(G), aH)
        compB = np.einsum("bijac,bnica->bnij", np.abs(G), aH)
        k = self.kappa[:, None]
        return A, C["A"] * k * U * compA, compA, Bt, C["Bt"] * k * U * compB, compB


def _mm(pt, weight, spec, nterms, old, flooring, dtype, mutant=None):
    """old * sqrt(sum weight A / sum weight Bt), floored; `spec` contracts (weight, trace)."""
    A, barA, compA, Bt, barB, compB = pt.traces()
    num, den = np.einsum(spec, weight, A), np.einsum(spec, weight, Bt)
    num_eu = (nterms + 2) * np.einsum(spec, weight, compA) + np.einsum(spec, weight, barA) / U
    den_eu = (nterms + 2) * np.einsum(spec, weight, compB) + np.einsum(spec, weight, barB) / U
    if mutant == "floor_first":  # the floor applied to the ratio, before the square root
        return old.astype(dtype) * np.sqrt(pr.floor(num / den, flooring)), None
    return pr._finish(num, num_eu, den, den_eu, dtype(0.5), old, flooring, dtype)


def _drop_last(a, axis, on):
    if not on:
        return a
    a = a.copy()
    idx = [slice(None)] * a.ndim
    idx[axis] = -1
    a[tuple(idx)] = 0
    return a


def update_basis(X, basis, activation, H, flooring, latent=None, dtype=LD, mutant=None, pt=None):
    """t <- floor(t sqrt(sum_j v A / sum_j v Bt)); partitioning: the sums also run over n with z
    (mnmf.py:836-901)."""
    pt = pt or Points(X, basis, activation, H, flooring, latent, dtype, mutant)
    T = X.shape[-1]
    V = _drop_last(activation.astype(dtype), -1, mutant == "frame")
    if latent is None:
        return _mm(pt, V, "bnkj,bnij->bnik", T, basis, flooring, dtype, mutant)
    w = np.einsum("bnk,bkj->bnkj", latent.astype(dtype), V)
    return _mm(pt, w, "bnkj,bnij->bik", T + pt.N + 1, basis, flooring, dtype, mutant)


def update_activation(X, basis, activation, H, flooring, latent=None, dtype=LD, mutant=None, pt=None):
    """v <- floor(v sqrt(sum_i t A / sum_i t Bt)) (mnmf.py:903-968)."""
    pt = pt or Points(X, basis, activation, H, flooring, latent, dtype, mutant)
    F = X.shape[2]
    Tm = _drop_last(basis.astype(dtype), -2, mutant == "bin")
    if latent is None:
        return _mm(pt, Tm, "bnik,bnij->bnkj", F, activation, flooring, dtype, mutant)
    w = np.einsum("bnk,bik->bnik", latent.astype(dtype), Tm)
    return _mm(pt, w, "bnik,bnij->bkj", F + pt.N + 1, activation, flooring, dtype, mutant)


def update_latent(X, basis, activation, H, flooring, latent, dtype=LD, mutant=None, pt=None):
    """z <- z sqrt(sum_ij t v A / sum_ij t v Bt), columns renormalised; no floor (mnmf.py:1018-1073)."""
    pt = pt or Points(X, basis, activation, H, flooring, latent, dtype, mutant)
    F, T = X.shape[2], X.shape[3]
    w = np.einsum("bik,bkj->bikj", basis.astype(dtype), activation.astype(dtype))
    z, zbar = _mm(pt, w, "bikj,bnij->bnk", F + T + 2, latent, NOF, dtype)
    col = z.sum(axis=1, keepdims=True)
    out = z / col
    N = z.shape[1]
    bar = zbar / col + out * (zbar.sum(axis=1, keepdims=True) + (N + 1) * U * col) / col + 2 * U * out
    return out, bar


def spatial_sums(X, basis, activation, H, flooring, latent=None, dtype=LD, mutant=None, pt=None):
    """P_ni = sum_j lambda R^-1, Q_ni = sum_j lambda R^-1 XX R^-1 (B,N,F,M,M) with elementwise bars,
    and the points."""
    pt = pt or Points(X, basis, activation, H, flooring, latent, dtype, mutant)
    c = _c(dtype)
    T = X.shape[-1]
    lam = _drop_last(pt.lam, -1, mutant == "frame")
    GXG = pt.G @ pt.XX @ pt.G
    P = np.einsum("bnij,bijac->bniac", lam.astype(c), pt.G)
    Q = np.einsum("bnij,bijac->bniac", lam.astype(c), GXG)
    k = pt.kappa[..., None, None]
    # normwise per point: an entry of a computed inverse is off by kappa u ||R^-1||, however small it is
    nG = np.linalg.norm(pt.G.astype(np.complex128), axis=(-2, -1))[..., None, None]
    nX = np.linalg.norm(pt.XX.astype(np.complex128), axis=(-2, -1))[..., None, None]
    aG, aGXG = nG * np.ones(pt.G.shape[-2:]), nG * nG * nX * np.ones(pt.G.shape[-2:])
    n = T + pt.K + 3
    # the solve's share in units of C["PQ"] (what the yardstick is normalised by), then the sums'
    solveP = U * np.einsum("bnij,bijac->bniac", lam, k * aG)
    solveQ = U * np.einsum("bnij,bijac->bniac", lam, k * aGXG)
    pt.pq_solve = (solveP, solveQ)
    barP = C["PQ"] * solveP + U * n * np.einsum("bnij,bijac->bniac", lam, aG)
    barQ = C["PQ"] * solveQ + U * n * np.einsum("bnij,bijac->bniac", lam, aGXG)
    return P, barP, Q, barQ, pt


def update_spatial(X, basis, activation, H, flooring, latent=None, dtype=LD, mutant=None, pt=None):
    """H <- to_psd(to_psd(P)^-1 # to_psd(H Q H)) (mnmf.py:970-1016; the geometric mean of
    linalg/mean.py type 2, as P^-1/2 (P^1/2 B P^1/2)^1/2 P^-1/2).  Returns (H_new, relative
    Frobenius bar per matrix (B,N,F), floored eigenvalue count of the three to_psd (B,N,F))."""
    P, _, Q, _, pt = spatial_sums(X, basis, activation, H, flooring, latent, dtype, mutant, pt)
    Hc = pt.H
    Pf, wP, wPf = to_psd(P, flooring, dtype)
    Bf, wB, wBf = to_psd(Hc @ Q @ Hc, flooring, dtype)
    Ph = _funm(Pf, np.sqrt, dtype)
    Pih = _funm(Pf, lambda w: 1 / np.sqrt(w), dtype)
    mid = _funm(Ph @ Bf @ Ph, lambda w: np.sqrt(np.maximum(w, 0)), dtype)
    Gm, wG, _ = to_psd(Pih @ mid @ Pih, flooring, dtype)
    eps = flooring[1]
    moved = sum((w < eps).sum(axis=-1) for w in (wP, wB, wG)) if flooring[0] == pr.FLOOR_MAX else \
        np.zeros(wP.shape[:-1], int)
    kS = np.maximum(wPf.max(axis=-1) / wPf.min(axis=-1), wBf.max(axis=-1) / wBf.min(axis=-1))
    kpt = pt.kappa.max(axis=-1)[:, None]                           # (B,1,F)
    kap = (kS + kpt).astype(np.float64)
    return Gm, C["gmean"] * kap * U, moved, kap


def spatial_error(Ha, Href, kap):
    """max over matrices of ||H - H_ref||_F / ((kappa_S + kappa_pt) u ||H_ref||_F)."""
    d = np.linalg.norm((Ha.astype(np.clongdouble) - Href).astype(np.complex128), axis=(-2, -1))
    return float(np.max(d / (np.linalg.norm(Href.astype(np.complex128), axis=(-2, -1)) * kap * U)))


def normalize(basis, H, latent=None, dtype=LD):
    """H /= tr H, basis[n, i, :] *= tr H; with partitioning the basis stays (mnmf.py:391-414)."""
    c = _c(dtype)
    M = H.shape[-1]
    Hc = H.astype(c)
    tr = np.einsum("bniaa->bni", Hc).real
    atr = np.einsum("bniaa->bni", np.abs(Hc.real))
    rel = (M + 1) * atr / np.abs(tr)
    Hn = Hc / tr[..., None, None]
    barH = U * np.abs(Hn) * (rel + 3)[..., None, None]
    if latent is not None:
        return Hn, barH, basis.astype(dtype), np.zeros(basis.shape)
    Tn = basis.astype(dtype) * tr[..., None]
    return Hn, barH, Tn, U * np.abs(Tn) * (rel + 2)[..., None]


def loss(X, basis, activation, H, flooring, dtype=LD, mutant=None, pt=None):
    """out[b] = sum_i mean_j (tr(R^-1 XX) + log det R) (mnmf.py:765-804), absolute bar."""
    pt = pt or Points(X, basis, activation, H, flooring, None, dtype, mutant)
    B, M, F, T = X.shape
    tr = np.einsum("bijac,bijca->bij", pt.G, pt.XX).real
    comp = np.einsum("bijac,bijca->bij", np.abs(pt.G), np.abs(pt.XX)).real
    ld = np.log(pt.ev).sum(axis=-1)
    term = tr + ld
    val = term.sum(axis=(1, 2)) / dtype(T)
    # the solve's share in units of C["loss"] (what the yardstick is normalised by), then the sum's
    pt.loss_solve = U * (pt.kappa * (comp + M)).sum(axis=(1, 2)) / dtype(T)
    bar = C["loss"] * pt.loss_solve \
        + U * (F * T + 2) * (np.abs(tr) + np.abs(ld)).sum(axis=(1, 2)) / dtype(T)
    return val, bar, pt


def separate(X, basis, activation, H, reference_id, flooring, dtype=LD, mutant=None, pt=None):
    """y_nij = (lambda_n H_n R^-1 x)[ref] (mnmf.py:729-763).  Returns (Y (B,N,F,T), points)."""
    pt = pt or Points(X, basis, activation, H, flooring, None, dtype, mutant)
    u = np.einsum("bijac,bijc->bija", pt.G, pt.x)
    Y = np.einsum("bnij,bnic,bijc->bnij", pt.lam.astype(_c(dtype)), pt.H[:, :, :, reference_id, :], u)
    return Y, pt


# ---------------------------------------------------------------------------------- yardsticks
def _ratio(a, ref, bar):
    err = np.abs(np.asarray(a).astype(ref.dtype) - ref)
    return float(np.max(err / bar))


def yardsticks(X, basis, activation, H, flooring, latent=None):
    """The kappa-normalised errors of the float64 restatement against the long-double one on these
    inputs, per quantity, in units of kappa u companion -- the solve's share of the bar alone, so that
    the float64 summation error of P, Q and the loss counts against the constant too (the numbers C
    is 8 x the maximum of)."""
    pl = Points(X, basis, activation, H, flooring, latent, LD)
    pf = Points(X, basis, activation, H, flooring, latent, np.float64)
    A, barA, _, Bt, barB, _ = pl.traces()
    Af, _, _, Bf, _, _ = pf.traces()
    out = {"A": _ratio(Af, A, barA) * C["A"], "Bt": _ratio(Bf, Bt, barB) * C["Bt"]}
    P, _, Q, _, pq = spatial_sums(X, basis, activation, H, flooring, latent, LD)
    Pf, _, Qf, _, _ = spatial_sums(X, basis, activation, H, flooring, latent, np.float64)
    out["PQ"] = max(_ratio(Pf, P, pq.pq_solve[0]), _ratio(Qf, Q, pq.pq_solve[1]))
    Hn, _, _, kap = update_spatial(X, basis, activation, H, flooring, latent, LD)
    Hf = update_spatial(X, basis, activation, H, flooring, latent, np.float64)[0]
    out["gmean"] = spatial_error(Hf, Hn, kap)
    if latent is None:
        v, _, lp = loss(X, basis, activation, H, flooring, LD)
        vf = loss(X, basis, activation, H, flooring, np.float64)[0]
        out["loss"] = _ratio(vf, v, lp.loss_solve)
        Y, pt = separate(X, basis, activation, H, X.shape[1] - 1, flooring, LD)
        Yf = separate(X, basis, activation, H, X.shape[1] - 1, flooring, np.float64)[0]
        out["separate"] = mr.separate_error(Yf, Y, X, pt.kappa)
    return out


# ---------------------------------------------------------------------------------- generators
def gen_state(seed, B, N, M, F, T, K, part=False, skew=1e-3):
    """(X, basis, activation, H, latent or None) of moderate dynamic range: every positive factor
    over 2^-1..2^1, H_n = A A^H / M + I / 4 scaled over 2^-1..2^1 -- plus an anti-Hermitian part of
    relative size `skew`, which to_psd's Hermitisation of R must remove and the traces must keep."""
    rng = np.random.default_rng(seed + 23)
    X = (rng.standard_normal((B, M, F, T)) + 1j * rng.standard_normal((B, M, F, T))) \
        * pr._log_uniform(rng, -1, 1, (B, M, F, T))
    A = rng.standard_normal((B, N, F, M, M)) + 1j * rng.standard_normal((B, N, F, M, M))
    H = (A @ np.swapaxes(A, -1, -2).conj() / M + np.eye(M) / 4) * pr._log_uniform(rng, -1, 1, (B, N, F, 1, 1))
    S = rng.standard_normal((B, N, F, M, M)) + 1j * rng.standard_normal((B, N, F, M, M))
    H = H + skew * (S - np.swapaxes(S, -1, -2).conj()) / 2
    if part:
        basis = pr._log_uniform(rng, -1, 1, (B, F, K))
        act = pr._log_uniform(rng, -1, 1, (B, K, T))
        z = pr._log_uniform(rng, -1, 1, (B, N, K))
        return X, basis, act, H, z / z.sum(axis=1, keepdims=True)
    return X, pr._log_uniform(rng, -1, 1, (B, N, F, K)), pr._log_uniform(rng, -1, 1, (B, N, K, T)), H, None


def gen_repair_points(seed, B, N, M, F, T, K, eps, frames):
    """gen_state scaled so that every eigenvalue of R_ij lies well above sqrt(M) eps, except at
    `frames` (of every bin), where the activation is scaled so that the MAX floor moves the smallest
    eigenvalue of R_ij (both asserted by the caller on the reference)."""
    X, basis, act, H, _ = gen_state(seed, B, N, M, F, T, K)
    lam = np.einsum("bnik,bnkj->bnij", basis, act)
    R = _herm(np.einsum("bnij,bniac->bijac", lam, H))
    lo = np.linalg.eigvalsh(R)[..., 0]
    act = act * (4 * np.sqrt(M) * eps / lo.min())
    lam = np.einsum("bnik,bnkj->bnij", basis, act)
    R = _herm(np.einsum("bnij,bniac->bijac", lam, H))
    lo = np.linalg.eigvalsh(R)[..., 0]
    for j in frames:
        act[..., j] *= 0.5 * eps / lo[:, :, j].max()
    return X, basis, act, H, None


def gen_silent_bin(seed, B, N, M, F, T, K, eps, silent, scale=1e6):
    """gen_state with bin `silent` made silent against its model: X = 0 there and the bin's spatial
    matrices scaled by `scale`, so that P = sum_j lambda R^-1 (of the order of 1 / scale) and H Q H
    fall below eps and to_psd floors them (asserted by the caller on the reference)."""
    X, basis, act, H, _ = gen_state(seed, B, N, M, F, T, K)
    X, H = X.copy(), H.copy()
    X[:, :, silent, :] = 0
    H[:, :, silent] *= scale
    return X, basis, act, H, None
