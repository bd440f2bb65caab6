"""Extended-precision restatement of the batched linear-algebra entry points, with per-matrix bars.

TEST INFRASTRUCTURE ONLY, in the style of tests/spatial_reference.py.  One function per entry point of
the "batched small linear algebra" and "Hermitian matrix functions" sections of include/ssspy_amd.h
(ssspy_solve, ssspy_inv2, ssspy_eigh, ssspy_eigh2, ssspy_eigh_general, ssspy_to_psd, ssspy_sqrtmh with
its inverse mode, ssspy_gmeanmh, ssspy_herm_rebuild), written from its header comments in
``np.longdouble`` on the long-double Jacobi of mnmf_reference.eigh_jacobi and the elimination of
pass_reference.lu_solve; with ``dtype=np.float64`` the SAME formula runs on np.linalg.eigh / solve /
inv / cholesky, which is the yardstick.  Nothing here calls into oracle/ or reads a kernel.

Definitions, as the header states them.  The Hermitian functions act on the Hermitian part
(A + A^H) / 2 of the input (the imaginary part of the diagonal is dropped).  np.linalg.eigh reads the
lower triangle only, so the float64 run is handed the Hermitian part.  Eigenvalues ascend, ties by
index.  to_psd is floor, rebuild, Hermitise.  The inverse square root is
P diag(1 / floor(sqrt(lam))) P^H.  The generalised problem goes through the Cholesky factor B = L L^H
(the lower triangle of B): type 1, A z = lam B z, C = L^-1 A L^-H, z = L^-H y; type 2, A B z = lam z,
C = L^H A L, z = L^-H y; type 3, B A z = lam z, C = L^H A L, z = L y.  gmeanmh is
X # Y = X^1/2 (X^-1/2 Y X^-1/2)^1/2 X^1/2 with type 1: A # B, 2: A^-1 # B, 3: A # B^-1.

Bars.  All per matrix, in u = 2^-53, evaluated in long double on the output under test.  None holds
an eigenvalue gap; no case and no element is left out.  A quantity whose scale is exactly zero (the
zero matrix) has to be exactly zero.

* eigh.  A backward-stable eigensolver returns the exact decomposition of A + E, ||E|| = O(u ||A||):
    eigenvalues   max_k |lam_k - ref_k| <= C["eig"]  u ||A||_2     (Weyl: |dlam| <= ||E||_2)
    residual      ||A V - V diag(lam)||_F <= C["res"]  u ||A||_F
    orthonormality ||V^H V - I||_F <= C["orth"] u
  Eigenvectors are never compared (they move by ||E|| / gap), except at 2 x 2 with a relative gap of
  0.1 or more, where V is held against np.linalg.eigh of the Hermitian part WITH its phases: both
  sit within residual / gap of the eigenvectors, so ||V - V_np||_F <= 2 C["res"] u / relgap.
* eigh2 / eigh_general.  C is formed with L^-1 or L, which loses kappa_2(L)^2 = kappa_2(B):
    eigenvalues   max_k |lam_k - ref_k| <= C["geig"] kappa_2(B) u max_k |ref_k|
    residual      type 1: ||A Z - B Z diag(lam)||_F <= C["gres"] kappa_2(B) u ||A||_F ||Z||_F
                  type 2: ||A B Z - Z diag(lam)||_F, type 3: ||B A Z - Z diag(lam)||_F
                          <= C["gres"] kappa_2(B) u ||A||_F ||B||_F ||Z||_F
                  (each right side has the dimension of its left: the bar holds at any scale)
    B-orthonormality  types 1, 2: ||Z^H B Z - I||_F, type 3: ||Z^H B^-1 Z - I||_F <= C["gorth"] kappa_2(B) u
* matrix functions.  ||out - ref||_F <= C[q] g u ||ref||_F with g the conditioning of f on the
  spectrum: an eigenvalue carries u ||A||_2 absolutely, f moves by |f'| times that.
    to_psd     g = 1: max(., eps), + eps and the identity are 1-Lipschitz.
    sqrtmh     f' = 1 / (2 sqrt(lam)): u lam_max / sqrt(lam_min) against ||ref|| ~ sqrt(lam_max):
               g = sqrt(kappa_2) of the spectrum.
    invsqrtmh  f = 1 / floor(sqrt(lam)): |f'| <= 1 / (2 lam^(3/2)): u lam_max / lam_min^(3/2) against
               ||ref|| ~ 1 / sqrt(lam_min): g = kappa_2 of the floored spectrum (floor(sqrt(lam))^2).
    gmeanmh    X^-1/2 Y X^-1/2 loses kappa_2(X), its root and the outer products no more than
               kappa_2 of either: g = kappa_2(A) + kappa_2(B).
    herm_rebuild  a sum of M products: g = || |P| diag|w| |P|^H ||_F / ||ref||_F (cancellation).
  Hermitian to the last bit: out == out^H exactly where the kernel Hermitises last (to_psd), else
  |out - out^H| <= 2 u |out| elementwise.
* solve.  Per right-hand side ||x - ref|| <= C["solve"] kappa_2(A) u ||ref||; inv2 per matrix in the
  Frobenius norm, ||out - ref||_F <= C["inv2"] kappa_2(A) u ||ref||_F.

C[q] = 8 x the float64 yardstick: the largest value, in the same normalised units, that the float64
run reaches against the long-double one over the input families below at every size the GPU test
uses (``yardsticks``), rounded up to two digits -- the rule of tests/gmnmf_reference.py.  Measured on
the CPU, never against a kernel; tests/test_linalg_reference_cpu.py measures them again.  All bars
are relative, so they hold unchanged for the families times an exact power of two.

``mutant`` arguments switch on one deliberate mistake each (CPU only; see the CPU test).
"""

import numpy as np

import mnmf_reference as mr
import pass_reference as pr
import prox_reference as xr

LD, U = pr.LD, pr.U
NOF = (pr.FLOOR_NONE, 0.0)
SIZES = (1, 2, 3, 5, 6, 7, 8, 9, 13, 16)          # Hermitian sizes of the GPU test, one per route
SOLVE_SIZES = (1, 2, 4, 8, 9, 16)
N_BATCH = 72

# the float64 yardsticks (see the module docstring); C = 8 x
MEASURED = {"eig": 17.0, "res": 13.0, "orth": 53.0, "geig": 19.0, "gres": 5.4, "gorth": 63.0, "psd": 26.0,
            "sqrt": 11.0, "invsqrt": 150.0, "gmean": 27.0, "rebuild": 1.3, "solve": 3.2, "inv2": 0.71}
C = {k: 8.0 * v for k, v in MEASURED.items()}


def _c(dtype):
    return np.clongdouble if dtype is LD else np.complex128


def _H(A):
    return np.swapaxes(A, -1, -2).conj()


def herm(A):
    return (A + _H(A)) / 2


def lower(A):
    """The Hermitian matrix np.linalg.eigh sees: the lower triangle and the real diagonal."""
    L = np.tril(A, -1)
    d = np.einsum("nmm->nm", A).real
    return L + _H(L) + d[:, :, None] * np.eye(A.shape[-1])


def fro(A):
    return np.sqrt((np.abs(A) ** 2).sum(axis=(-2, -1)))


def ratio(num, den):
    """num / den per matrix; a zero scale admits a zero error only; non-finite counts as infinite."""
    num, den = np.asarray(num, dtype=LD), np.asarray(den, dtype=LD)
    with np.errstate(all="ignore"):
        r = np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num == 0, 0.0, np.inf))
    return np.where(np.isfinite(r), r, np.inf).astype(np.float64)


def kappa2(A):
    """kappa_2 of a stack of matrices (float64 singular values: exact enough up to 1e12)."""
    s = np.linalg.svd(np.asarray(A, dtype=np.complex128), compute_uv=False)
    with np.errstate(all="ignore"):
        return np.where(s[:, -1] > 0, s[:, 0] / np.where(s[:, -1] > 0, s[:, -1], 1), np.inf)


# ------------------------------------------------------------------------------- eigen core
def sweeps_needed(A):
    """Cyclic Jacobi sweeps in complex128 until off^2 <= 1e-34 diag^2 holds for every matrix of the
    stack (the criterion the kernels vote on)."""
    for s in range(1, 13):
        w, V = mr.eigh_jacobi(A, sweeps=s)
        D = _H(V) @ A @ V
        diag = (np.einsum("nmm->nm", D).real ** 2).sum(axis=-1)
        off = (np.abs(D) ** 2).sum(axis=(-2, -1)) - diag
        if np.all(off / 2 <= 1e-34 * diag):
            return s
    return 12


def sort_by_rank(w, V, mutant=None):
    """Ascending order through the rank of every eigenvalue, ties by index, into zeroed outputs (as a
    kernel without dynamic indexing stores them).  mutant "ties_by_value": the tie term dropped, so
    equal eigenvalues land on one slot and leave another unwritten."""
    n, M = w.shape
    j = np.arange(M)
    before = w[:, :, None] < w[:, None, :]                       # [n, j, k]: w_j < w_k
    if mutant != "ties_by_value":
        before = before | ((w[:, :, None] == w[:, None, :]) & (j[:, None] < j[None, :]))
    rank = before.sum(axis=1)
    lam, Vs = np.zeros_like(w), np.zeros_like(V)
    np.put_along_axis(lam, rank, w, axis=1)
    np.put_along_axis(Vs, np.broadcast_to(rank[:, None, :], V.shape), V, axis=2)
    return lam, Vs


def _eig_of(Hm, dtype, mutant=None):
    """(lam ascending, V) of an exactly Hermitian stack in `dtype`."""
    if mutant == "sweeps":
        H64 = Hm.astype(np.complex128)
        w, V = mr.eigh_jacobi(H64, sweeps=sweeps_needed(H64) - 1)
    elif dtype is LD:
        with np.errstate(over="ignore"):  # (tau^2 of a pair already annihilated: t = 0 either way)
            w, V = mr.eigh_jacobi(Hm.astype(np.clongdouble))
    else:
        w, V = np.linalg.eigh(Hm)
    return sort_by_rank(w, V, mutant)


def hermitian_part(A, dtype=LD, mutant=None):
    return lower(A.astype(_c(dtype))) if mutant == "lower" else herm(A.astype(_c(dtype)))


def eigh(A, dtype=LD, mutant=None):
    """ssspy_eigh: lam (n,M) ascending, V (n,M,M) unit eigenvectors in columns."""
    return _eig_of(hermitian_part(A, dtype, mutant), dtype, mutant)


def _rebuild(V, w):
    return (V * w.astype(V.dtype)[:, None, :]) @ _H(V)


def to_psd(A, flooring, dtype=LD, mutant=None):
    """ssspy_to_psd.  Returns (out, g = 1)."""
    w, V = eigh(A, dtype, mutant)
    return herm(_rebuild(V, pr.floor(w, flooring))), np.ones(A.shape[0])


def sqrtmh(A, dtype=LD, mutant=None):
    """ssspy_sqrtmh, inverse == 0.  Returns (out, g = sqrt(kappa_2))."""
    w, V = eigh(A, dtype, mutant)
    with np.errstate(all="ignore"):
        g = np.sqrt(np.abs(w).max(axis=-1) / np.abs(w).min(axis=-1)).astype(np.float64)
        return _rebuild(V, np.sqrt(w)), g


def invsqrtmh(A, flooring=NOF, dtype=LD, mutant=None):
    """ssspy_sqrtmh, inverse == 1.  Returns (out, g = kappa_2 of the floored spectrum)."""
    w, V = eigh(A, dtype, mutant)
    with np.errstate(all="ignore"):
        s = np.sqrt(pr.floor(w, flooring)) if mutant == "floor_lam" else pr.floor(np.sqrt(w), flooring)
        g = ((s.max(axis=-1) / s.min(axis=-1)) ** 2).astype(np.float64)
        return _rebuild(V, 1 / s), g


def herm_rebuild(P, w, hermitise, dtype=LD):
    """ssspy_herm_rebuild.  Returns (out, g)."""
    Pc = P.astype(_c(dtype))
    out = _rebuild(Pc, w.astype(dtype))
    comp = (np.abs(Pc) * np.abs(w.astype(dtype))[:, None, :]) @ np.swapaxes(np.abs(Pc), -1, -2)
    if hermitise:
        out = herm(out)
    return out, np.maximum(ratio(fro(comp), fro(out)), 1.0)


def _funm(Hm, fn, dtype):
    w, V = _eig_of(Hm, dtype)
    return _rebuild(V, fn(w))


def _swap23(type, mutant):
    return {2: 3, 3: 2}.get(type, type) if mutant == "swap_types" else type


def gmeanmh(A, Bm, type=1, dtype=LD, mutant=None):
    """ssspy_gmeanmh.  Returns (G, g = kappa_2(A) + kappa_2(B))."""
    type = _swap23(type, mutant)
    Ah, Bh = hermitian_part(A, dtype), hermitian_part(Bm, dtype)
    X, Y = (Bh, Ah) if type == 3 else (Ah, Bh)
    w, V = _eig_of(X, dtype)
    root, iroot = _rebuild(V, np.sqrt(w)), _rebuild(V, 1 / np.sqrt(w))
    outer, inner = (root, iroot) if type == 1 else (iroot, root)
    mid = _funm(herm(inner @ Y @ inner), lambda w: np.sqrt(np.maximum(w, 0)), dtype)
    G = herm(outer @ mid @ outer)
    return G, kappa2(herm(A.astype(np.complex128))) + kappa2(herm(Bm.astype(np.complex128)))


def cholesky(Bm, dtype=LD):
    """Lower Cholesky factor from the lower triangle of Bm."""
    if dtype is not LD:
        return np.linalg.cholesky(Bm.astype(np.complex128))
    Bc = Bm.astype(np.clongdouble)
    n, M, _ = Bc.shape
    L = np.zeros_like(Bc)
    for c in range(M):
        d = Bc[:, c, c].real - (np.abs(L[:, c, :c]) ** 2).sum(axis=-1)
        L[:, c, c] = np.sqrt(d)
        L[:, c + 1:, c] = (Bc[:, c + 1:, c] - (L[:, c + 1:, :c] * L[:, c, None, :c].conj()).sum(axis=-1)) \
            / L[:, c, c][:, None]
    return L


def inv(A, dtype=LD):
    if dtype is not LD:
        return np.linalg.inv(A)
    eye = np.broadcast_to(np.eye(A.shape[-1], dtype=A.dtype), A.shape).copy()
    return pr.lu_solve(A, eye)[0]


def eigh_general(A, Bm, type=1, dtype=LD, mutant=None):
    """ssspy_eigh_general (and ssspy_eigh2 at 2 x 2).  Returns (lam ascending, Z)."""
    type = _swap23(type, mutant)
    Ac = A.astype(_c(dtype))
    L = cholesky(Bm, dtype)
    Li = inv(L, dtype)
    Cm = Li @ Ac @ _H(Li) if type == 1 else _H(L) @ Ac @ L
    lam, Y = _eig_of(herm(Cm), dtype)
    return lam, (L @ Y if type == 3 else _H(Li) @ Y)


def solve(A, Bm, dtype=LD, mutant=None):
    """ssspy_solve: X = A^-1 B by elimination with partial pivoting."""
    c = _c(dtype)
    if mutant == "no_pivot":
        return _solve_no_pivot(A.astype(np.complex128), Bm.astype(np.complex128))
    if dtype is LD:
        return pr.lu_solve(A.astype(c), Bm.astype(c))[0]
    return np.linalg.solve(A.astype(c), Bm.astype(c))


def _solve_no_pivot(A, X):
    A, X = A.copy(), X.copy()
    N = A.shape[-1]
    with np.errstate(all="ignore"):
        for k in range(N):
            f = A[:, k + 1:, k] / A[:, k, k][:, None]
            A[:, k + 1:, :] -= f[:, :, None] * A[:, k, :][:, None, :]
            X[:, k + 1:, :] -= f[:, :, None] * X[:, k, :][:, None, :]
        for k in range(N - 1, -1, -1):
            X[:, k, :] = (X[:, k, :] - (A[:, k, k + 1:, None] * X[:, k + 1:, :]).sum(axis=1)) \
                / A[:, k, k][:, None]
    return X


def inv2(A, dtype=LD):
    """ssspy_inv2: the closed form [[d, -b], [-c, a]] / (a d - b c)."""
    if dtype is not LD:
        return np.linalg.inv(A.astype(np.complex128))
    Ac = A.astype(np.clongdouble)
    a, b, c, d = Ac[:, 0, 0], Ac[:, 0, 1], Ac[:, 1, 0], Ac[:, 1, 1]
    det = a * d - b * c
    return np.stack([np.stack([d, -b], axis=-1), np.stack([-c, a], axis=-1)], axis=-2) / det[:, None, None]


# ------------------------------------------------------------------------------- measures (no C)
def eig_error(lam, ref):
    """max_k |lam_k - ref_k| / (u ||A||_2), ||A||_2 = max |ref|."""
    d = np.abs(np.asarray(lam).astype(LD) - ref).max(axis=-1)
    return ratio(d, U * np.abs(ref).max(axis=-1))


def residual(A, lam, V):
    """||H V - V diag(lam)||_F / (u ||H||_F), H the Hermitian part of A."""
    Hm = herm(A.astype(np.clongdouble))
    Vc = np.asarray(V).astype(np.clongdouble)
    R = Hm @ Vc - Vc * np.asarray(lam).astype(LD)[:, None, :]
    return ratio(fro(R), U * fro(Hm))


def orthonormality(V, Bm=None):
    """||V^H V - I||_F / u (with Bm: ||V^H Bm V - I||_F / u)."""
    Vc = np.asarray(V).astype(np.clongdouble)
    G = _H(Vc) @ Vc if Bm is None else _H(Vc) @ Bm.astype(np.clongdouble) @ Vc
    return ratio(fro(G - np.eye(Vc.shape[-1])), U * np.ones(Vc.shape[0]))


def general_measures(A, Bm, type, lam, Z, ref_lam):
    """(eigenvalue error, residual, B-orthonormality) of a generalised decomposition, each divided
    by kappa_2(B) u and its scale."""
    Ac, Bc = A.astype(np.clongdouble), herm(lower(Bm.astype(np.clongdouble)))
    Zc, lc = np.asarray(Z).astype(np.clongdouble), np.asarray(lam).astype(LD)
    k = kappa2(Bc)
    if type == 1:
        R = Ac @ Zc - (Bc @ Zc) * lc[:, None, :]
    elif type == 2:
        R = Ac @ Bc @ Zc - Zc * lc[:, None, :]
    else:
        R = Bc @ Ac @ Zc - Zc * lc[:, None, :]
    metric = inv(Bc) if type == 3 else Bc
    e = ratio(np.abs(lc - ref_lam).max(axis=-1), k * U * np.abs(ref_lam).max(axis=-1))
    r = ratio(fro(R), k * U * fro(Ac) * (1.0 if type == 1 else fro(Bc)) * fro(Zc))
    o = orthonormality(Zc, metric) / k
    return e, r, o


def fn_error(out, ref, g):
    """||out - ref||_F / (g u ||ref||_F)."""
    return ratio(fro(np.asarray(out).astype(np.clongdouble) - ref), g * U * fro(ref))


def hermitian_defect(out):
    """max over elements of |out - out^H| / (u |out|) per matrix (0: Hermitian to the last bit)."""
    out = np.asarray(out)
    d = np.abs(out - _H(out))
    return np.array([float(ratio(d[i], U * np.abs(out[i])).max()) for i in range(out.shape[0])])


def solve_error(X, ref, kappa):
    """||x - ref|| / (kappa u ||ref||) per right-hand side -> (n, nrhs)."""
    d = np.sqrt((np.abs(np.asarray(X).astype(np.clongdouble) - ref) ** 2).sum(axis=-2))
    return ratio(d, kappa[:, None] * U * np.sqrt((np.abs(ref) ** 2).sum(axis=-2)))


def relgap2(A):
    """(lam1 - lam0) / max |lam| of 2 x 2 Hermitian parts, in float64."""
    w = np.linalg.eigvalsh(herm(np.asarray(A, dtype=np.complex128)))
    with np.errstate(all="ignore"):
        return np.where(np.abs(w).max(axis=-1) > 0, (w[:, 1] - w[:, 0]) / np.abs(w).max(axis=-1), 0.0)


# ------------------------------------------------------------------------------- generators
HERMITIAN_KINDS = ["indefinite", "graded", "clustered", "rank_one", "repeated_pairs", "real_symmetric",
                   "non_hermitian", "diagonal_descending", "identity", "zero"]
KINDS_2X2 = ["zero_offdiagonal", "equal_diagonals", "scaled_identity", "weak_coupling"]
PD_KINDS = ["gram", "graded", "clustered", "repeated_pairs", "real_symmetric", "non_hermitian",
            "diagonal_descending", "identity"]
SYSTEM_KINDS = ["complex", "real", "zero_00", "scaled_permutation", "pivot_tie", "kappa_1e4", "kappa_1e8",
                "kappa_1e12"]


def _gauss(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _unitary(rng, M):
    return np.linalg.qr(_gauss(rng, (M, M)))[0]


def _with_spectrum(rng, d):
    Q = _unitary(rng, len(d))
    return herm(((Q * np.asarray(d, dtype=np.float64)) @ Q.conj().T)[None])[0]


def _repeated(rng, M, positive):
    h = (M + 1) // 2
    d = rng.uniform(0.5, 2.0, h) if positive else rng.uniform(-2.0, 2.0, h)
    K = np.kron(_with_spectrum(rng, d), np.eye(2))      # every eigenvalue exactly twice
    p = rng.permutation(2 * h)
    return K[np.ix_(p, p)][:M, :M]


def _skew(rng, M):
    S = _gauss(rng, (M, M))
    return 1e-3 * ((S - S.conj().T) / 2 + 1j * np.diag(rng.standard_normal(M)))


def _hermitian_one(rng, kind, M):
    if kind == "indefinite":
        G = _gauss(rng, (M, M))
        return G + G.conj().T
    if kind == "graded":
        return _with_spectrum(rng, np.logspace(0, -12, M))
    if kind == "clustered":
        q = _unitary(rng, M)[:, 0]
        return herm((np.eye(M) + 1e-9 * np.outer(q, q.conj()))[None])[0]
    if kind == "rank_one":
        v = _gauss(rng, (M,))
        return np.outer(v, v.conj())
    if kind == "repeated_pairs":
        return _repeated(rng, M, False)
    if kind == "real_symmetric":
        G = rng.standard_normal((M, M))
        return (G + G.T).astype(np.complex128)
    if kind == "non_hermitian":
        G = _gauss(rng, (M, M))
        return G + G.conj().T + _skew(rng, M)
    if kind == "diagonal_descending":
        return np.diag(np.linspace(2.0, -1.0, M) if M > 1 else np.ones(1)).astype(np.complex128)
    if kind == "identity":
        return np.eye(M, dtype=np.complex128)
    if kind == "zero":
        return np.zeros((M, M), np.complex128)
    a, d = rng.uniform(0.5, 2.0), rng.uniform(-2.0, -0.5)
    ph = np.exp(1j * rng.uniform(0, 2 * np.pi))
    if kind == "zero_offdiagonal":
        return np.array([[a, 0], [0, d]], np.complex128)
    if kind == "equal_diagonals":
        return np.array([[a, ph], [np.conj(ph), a]])
    if kind == "scaled_identity":
        return a * np.eye(2, dtype=np.complex128)
    b = 1e-9 * abs(a - d) * ph                                 # weak_coupling
    return np.array([[a, b], [np.conj(b), d]])


def hermitian_kinds(M):
    return HERMITIAN_KINDS + (KINDS_2X2 if M == 2 else [])


def gen_hermitian(seed, n, M, scale=1.0):
    """n matrices (n,M,M) c128, the families interleaved one by one (matrix i is of kind i mod 10; at
    2 x 2 four more kinds follow), so that every wave and every group of 8 holds several kinds.
    Returns (A, kind names per matrix).  `scale`: an exact power of two."""
    rng = np.random.default_rng(1000 * M + seed)
    kinds = hermitian_kinds(M)
    names = [kinds[i % len(kinds)] for i in range(n)]
    return np.ascontiguousarray(np.stack([_hermitian_one(rng, k, M) for k in names]) * scale), names


def _pd_one(rng, kind, M, skew, decades=2):
    if kind == "gram":
        G = _gauss(rng, (M, 2 * M))
        return G @ G.conj().T / (2 * M) + 0.1 * np.eye(M)
    if kind == "graded":
        return _with_spectrum(rng, np.logspace(0, -decades, M))
    if kind == "clustered":
        return _hermitian_one(rng, "clustered", M)
    if kind == "repeated_pairs":
        return _repeated(rng, M, True)
    if kind == "real_symmetric":
        G = rng.standard_normal((M, 2 * M))
        return (G @ G.T / (2 * M) + 0.1 * np.eye(M)).astype(np.complex128)
    if kind == "non_hermitian":
        return _pd_one(rng, "gram", M, False) + (_skew(rng, M) if skew else 0)
    if kind == "diagonal_descending":
        return np.diag(np.linspace(2.0, 0.25, M) if M > 1 else np.ones(1)).astype(np.complex128)
    return np.eye(M, dtype=np.complex128)


def gen_pd_pairs(seed, n, M, scale=1.0, skew=False, decades=2):
    """Positive definite pairs (A, B): A of kind i mod 8, kappa_2(B) = 1e0, 1e4, 1e8 for i mod 3 = 0,
    1, 2 (B = 1.5 I, then a graded spectrum under a random unitary); exactly Hermitian unless `skew`
    (A's non_hermitian kind then carries its 1e-3 anti-Hermitian part).  A's graded kind spans
    `decades`: 2 in the pairs, because the mean and the generalised problem lose the PRODUCT of the
    two condition numbers where both are large, which the factors of their bars (a sum, kappa_2(B)
    alone) do not hold; 6 where A is used alone (sqrtmh, invsqrtmh).  Returns (A, B, names)."""
    rng = np.random.default_rng(2000 * M + seed)
    names = ["{} kB1e{}".format(PD_KINDS[i % len(PD_KINDS)], 4 * (i % 3)) for i in range(n)]
    A = np.stack([_pd_one(rng, PD_KINDS[i % len(PD_KINDS)], M, skew, decades) for i in range(n)])
    Bs = []
    for i in range(n):
        e = 4 * (i % 3)
        Bs.append(1.5 * np.eye(M, dtype=np.complex128) if e == 0 or M == 1
                  else _with_spectrum(rng, np.logspace(0, -e, M)))
    return (np.ascontiguousarray(A * scale), np.ascontiguousarray(np.stack(Bs) * scale), names)


def gen_pd(seed, n, M, scale=1.0):
    """The positive definite A alone, for sqrtmh / invsqrtmh: graded over 6 decades, with the
    non-Hermitian kind."""
    return gen_pd_pairs(seed, n, M, scale, skew=True, decades=6)[0]


def _system_one(rng, kind, N):
    if kind == "real":
        return rng.standard_normal((N, N)).astype(np.complex128)
    if kind.startswith("kappa"):
        return xr.with_singular_values(rng, N, xr.graded(float(kind[6:]), N))
    A = _gauss(rng, (N, N))
    if N == 1:
        return A
    if kind == "zero_00":
        A[0, 0] = 0
    elif kind == "scaled_permutation":       # a cyclic shift: every step needs a row exchange
        A = np.roll(np.diag(np.exp2(rng.integers(-2, 3, N)) * np.exp(1j * rng.uniform(0, 6, N))), 1, axis=0)
    elif kind == "pivot_tie":
        A[0, 0] *= 4
        A[1, 0] = np.conj(A[0, 0])
    return A


def gen_systems(seed, n, N, nrhs, scale=1.0):
    """(A (n,N,N), B (n,N,nrhs), names): kinds interleaved as in gen_hermitian."""
    rng = np.random.default_rng(3000 * N + 10 * nrhs + seed)
    names = [SYSTEM_KINDS[i % len(SYSTEM_KINDS)] for i in range(n)]
    A = np.stack([_system_one(rng, k, N) for k in names])
    Bm = _gauss(rng, (n, N, nrhs))
    Bm[1::8] = Bm[1::8].real
    return np.ascontiguousarray(A * scale), np.ascontiguousarray(Bm), names


# ------------------------------------------------------------------------------- yardsticks
FLOORS = (NOF, (pr.FLOOR_MAX, 1e-10), (pr.FLOOR_ADD, 1e-10), (pr.FLOOR_MAX, 0.5), (pr.FLOOR_ADD, 0.5))


def gen_rebuild(seed, n, M):
    """(P, w) for herm_rebuild: the eigenvectors of the Hermitian families, signed weights."""
    A, _ = gen_hermitian(seed, n, M)
    _, V = np.linalg.eigh(herm(A))
    w = np.random.default_rng(4000 + M + seed).standard_normal((n, M))
    return np.ascontiguousarray(V), w


def _worst(d, key, values):
    d[key] = max(d.get(key, 0.0), float(np.max(values)))


def yardsticks(M, seed=0, mutant=None, keys=None):
    """The largest normalised error of the (mutated) float64 restatement against the long-double one
    at size M over the families, per quantity (the numbers MEASURED is the maximum of)."""
    out = {}
    want = lambda k: keys is None or k in keys  # noqa: E731
    f64 = np.float64
    if want("eig") or want("res") or want("orth") or want("psd"):
        A, _ = gen_hermitian(seed, N_BATCH, M)
        ref_lam, _ = eigh(A)
        lam, V = eigh(A, f64, mutant)
        _worst(out, "eig", eig_error(lam, ref_lam))
        _worst(out, "res", residual(A, lam, V))
        _worst(out, "orth", orthonormality(V))
        if want("psd"):
            for fl in FLOORS:
                ref, g = to_psd(A, fl)
                _worst(out, "psd", fn_error(to_psd(A, fl, f64, mutant)[0], ref, g))
    if M >= 2 and (want("sqrt") or want("invsqrt")):
        A = gen_pd(seed, N_BATCH, M)
        ref, g = sqrtmh(A)
        _worst(out, "sqrt", fn_error(sqrtmh(A, f64, mutant)[0], ref, g))
        for fl in FLOORS:
            ref, g = invsqrtmh(A, fl)
            _worst(out, "invsqrt", fn_error(invsqrtmh(A, fl, f64, mutant)[0], ref, g))
    if M >= 2 and (want("gmean") or want("geig")):
        A, Bm, _ = gen_pd_pairs(seed, N_BATCH, M)
        for t in (1, 2, 3):
            if want("gmean"):
                ref, g = gmeanmh(A, Bm, t)
                _worst(out, "gmean", fn_error(gmeanmh(A, Bm, t, f64, mutant)[0], ref, g))
            if want("geig"):
                ref_lam, _ = eigh_general(A, Bm, t)
                lam, Z = eigh_general(A, Bm, t, f64, mutant)
                e, r, o = general_measures(A, Bm, t, lam, Z, ref_lam)
                _worst(out, "geig", e)
                _worst(out, "gres", r)
                _worst(out, "gorth", o)
    if want("rebuild"):
        P, w = gen_rebuild(seed, N_BATCH, M)
        for h in (0, 1):
            ref, g = herm_rebuild(P, w, h)
            _worst(out, "rebuild", fn_error(herm_rebuild(P, w, h, f64)[0], ref, g))
    return out


def solve_yardsticks(N, seed=0, mutant=None):
    out = {}
    for nrhs in sorted({1, 3, N}):
        A, Bm, _ = gen_systems(seed, N_BATCH, N, nrhs)
        _worst(out, "solve", solve_error(solve(A, Bm, np.float64, mutant), solve(A, Bm), kappa2(A)))
    if N == 2:
        A, _, _ = gen_systems(seed, N_BATCH, 2, 1)
        ref = inv2(A)
        _worst(out, "inv2", fn_error(inv2(A, np.float64), ref, kappa2(A)))
    return out


def measure_all():
    worst = {}
    for M in SIZES:
        for k, v in yardsticks(M).items():
            worst[k] = max(worst.get(k, 0.0), v)
    for N in SOLVE_SIZES:
        for k, v in solve_yardsticks(N).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


if __name__ == "__main__":
    for k, v in sorted(measure_all().items()):
        print(k, v)
