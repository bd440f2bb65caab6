"""Every batched linear-algebra entry point alone, matrix by matrix, against the extended-precision
restatement of tests/linalg_reference.py (the bars, their conditioning factors and the input families
are in its module docstring: per matrix, c g u scale with c = 8 x the float64 restatement's own
normalised error, measured on the CPU; nothing fitted to a kernel, no matrix and no element left out).

The C entry points are called through _lib.load(); inputs carry a NaN band behind the data, outputs
lie between sentinel bands (a store past n, or into a padded row or column, fails the case).

Routes (every case names the one it reaches): ssspy_eigh / ssspy_to_psd -- k_eigh at 1, 3, 5,
k_eigh2_plain at 2, k_eigh_p on packed storage at 6 (to_psd through its LDS rebuild), a matrix on 8
lanes at 7 (padded) and 8, the size at run time at 9, 13, 16; the other Hermitian functions -- a lane
per matrix up to 6, 8 lanes at 7 and 8, run time from 9; ssspy_eigh2 (k_eigh2); ssspy_solve -- per-N
kernels at 1, 2, 4, 8, solve_rt at 9 and 16.  Batches: 72 matrices (a full 64-lane block plus 8; two
full blocks of 32 plus one group of 8), 33 (ragged last group and block) and 1; solve also at 65.
The families are interleaved, so the zero and identity matrices share every wave with the clustered
and graded ones, whose sweeps the wave vote makes them run, and meet the same bars.

What the file found (all fixed in the kernels, every case passes): ssspy_eigh at 2 x 2 read the lower
triangle only; to_psd and sqrtmh on 8 lanes did not Hermitise their rebuilt rows; and the run-time-size
Jacobi (rt_jacobi) kept turning the pairs of a resolved eigenvalue cluster, where diagonal difference
and coupling are both rounding noise and the normwise criterion sits at that noise from 13 x 13 on --
all 12 sweeps, the eigenvectors losing orthonormality turn by turn (clustered family, 16 x 16: 670 u
against the bar 424; sqrtmh 182 against 88; gmeanmh 243 against 216).  A pair below
1e-16 sqrt(|a_pp a_qq|) is now left alone.

Run as a script on the GPU to rewrite profiles/linalg_elementwise.txt.
"""

import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linalg_reference as lr  # noqa: E402
import pass_reference as pr  # noqa: E402
from test_gpu_pass_elementwise import Out, _mods, up  # noqa: E402

pytestmark = pytest.mark.gpu

LD = pr.LD
NOF = lr.NOF
FLOORS = lr.FLOORS
MAX_HALF = (pr.FLOOR_MAX, 0.5)
N = lr.N_BATCH
BATCHES = (N, 33, 1)
ONE_SCALES = (-240, 240)   # one-matrix entries and solve: squares stay inside [1e-300, 1e300]
TWO_SCALES = (-120, 120)   # two-matrix entries (both matrices): pairwise products stay inside it
HERM_SIZES = [m for m in lr.SIZES if m >= 2]


def eigh_route(M):
    return {1: "k_eigh<Fixed<1>>", 2: "k_eigh2_plain", 3: "k_eigh<Fixed<3>>", 5: "k_eigh<Fixed<5>>", 6: "k_eigh_p<6>",
            7: "8 lanes padded M7", 8: "8 lanes M8"}.get(M, "run-time M{}".format(M))


def fn_route(M):
    return "lane per matrix M{}".format(M) if M <= 6 else eigh_route(M)


def record(entry, route, err, c, names, extra=""):
    """Per-matrix normalised errors against the bar c: one line per family (its worst matrix)."""
    err = np.asarray(err, dtype=np.float64)
    err = err.reshape(err.shape[0], -1).max(axis=1)
    worst = {}
    for k, e in zip(names, err):
        worst[k] = max(worst.get(k, 0.0), float(e))
    path = os.environ.get("SSSPY_PASS_PROFILE_RAW")
    lines = []
    for k in sorted(worst):
        line = "{}\t{} | {}\t{:.3f}\t{:.3f}\t{:.4f}\t{}".format(entry, route, k, worst[k], c,
                                                             worst[k] / c, extra)
        print(line)
        lines.append(line)
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    bad = [ln for ln, k in zip(lines, sorted(worst)) if not worst[k] <= c]
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------- device calls
def _lib_call(name, *args):
    torch, _, _lib, _ = _mods()
    _lib.check(getattr(_lib.load(), name)(*args), name)
    torch.cuda.synchronize()
    del _KEEP[:]


_KEEP = []


def keep(a):
    """up(a), held until the outputs of the launch are read back (a view dropped right after its
    pointer is taken would hand its memory to the next upload)."""
    _KEEP.append(up(a))
    return _KEEP[-1]


def _ptr(t):
    from ssspy_amd._device import ptr

    return ptr(t) if t is not None else None


def _st():
    _, dv, _, _ = _mods()
    return dv.stream_handle()


def _info():
    _, dv, _, _ = _mods()
    return dv.zeros((1,), dv.i32)


def run_eigh(A):
    n, M, _ = A.shape
    ol, oV = Out((n, M)), Out((n, M, M), True)
    _lib_call("ssspy_eigh", _ptr(keep(A)), _ptr(ol.t), _ptr(oV.t), n, M, _st())
    return ol.get(), oV.get()


def run_to_psd(A, flooring):
    n, M, _ = A.shape
    o = Out((n, M, M), True)
    _lib_call("ssspy_to_psd", _ptr(keep(A)), _ptr(o.t), n, M, flooring[0], float(flooring[1]), _st())
    return o.get()


def run_sqrtmh(A, inverse, flooring=NOF):
    n, M, _ = A.shape
    o = Out((n, M, M), True)
    _lib_call("ssspy_sqrtmh", _ptr(keep(A)), _ptr(o.t), n, M, int(inverse), flooring[0], float(flooring[1]),
              _st())
    return o.get()


def run_gmeanmh(A, Bm, type):
    n, M, _ = A.shape
    o = Out((n, M, M), True)
    _lib_call("ssspy_gmeanmh", _ptr(keep(A)), _ptr(keep(Bm)), _ptr(o.t), n, M, type, _st())
    return o.get()


def run_general(A, Bm, type, entry):
    n, M, _ = A.shape
    ol, oZ, info = Out((n, M)), Out((n, M, M), True), _info()
    if entry == "eigh2":
        _lib_call("ssspy_eigh2", _ptr(keep(A)), _ptr(keep(Bm)), _ptr(ol.t), _ptr(oZ.t), n, type, _ptr(info), _st())
    else:
        _lib_call("ssspy_eigh_general", _ptr(keep(A)), _ptr(keep(Bm)), _ptr(ol.t), _ptr(oZ.t), n, M, type,
                  _ptr(info), _st())
    return ol.get(), oZ.get(), int(info.item())


def run_rebuild(P, w, hermitise):
    n, M, _ = P.shape
    o = Out((n, M, M), True)
    _lib_call("ssspy_herm_rebuild", _ptr(keep(P)), _ptr(keep(w)), _ptr(o.t), n, M, int(hermitise), _st())
    return o.get()


def run_solve(A, Bm):
    n, Nn, nrhs = Bm.shape
    o, info = Out((n, Nn, nrhs), True), _info()
    _lib_call("ssspy_solve", _ptr(keep(A)), _ptr(keep(Bm)), _ptr(o.t), n, Nn, nrhs, _ptr(info), _st())
    return o.get(), int(info.item())


def run_inv2(A):
    o = Out(A.shape, True)
    _lib_call("ssspy_inv2", _ptr(keep(A)), _ptr(o.t), A.shape[0], _st())
    return o.get()


# ------------------------------------------------------------------------------- references, once
# (a scaled case: the long-double run of the inputs times 2^e is the unscaled run times a power of two,
#  exactly -- long double neither overflows nor underflows here -- so the reference is scaled, not redone)
def _x2(a, p):
    return a * LD(2.0) ** p


@functools.lru_cache(maxsize=None)
def herm_case(M, e=0):
    A, names = lr.gen_hermitian(0, N, M, 2.0 ** e)
    lam = _x2(herm_case(M)[2], e) if e else lr.eigh(A)[0]
    return A, names, lam


@functools.lru_cache(maxsize=None)
def psd_ref(M, flooring, e=0):
    if e:
        assert flooring == NOF
        ref, g = psd_ref(M, NOF)
        return _x2(ref, e), g
    return lr.to_psd(herm_case(M)[0], flooring)


@functools.lru_cache(maxsize=None)
def pd_case(M, e=0):
    names = lr.gen_pd_pairs(0, N, M, skew=True, decades=6)[2]
    return lr.gen_pd(0, N, M, 2.0 ** e), [k.split(" ")[0] for k in names]


@functools.lru_cache(maxsize=None)
def sqrt_ref(M, inverse, flooring, e=0):
    if e:
        assert flooring == NOF and e % 2 == 0
        ref, g = sqrt_ref(M, inverse, NOF)
        return _x2(ref, -e // 2 if inverse else e // 2), g
    A = pd_case(M)[0]
    return lr.invsqrtmh(A, flooring) if inverse else lr.sqrtmh(A)


@functools.lru_cache(maxsize=None)
def pair_case(M, e=0):
    return lr.gen_pd_pairs(0, N, M, 2.0 ** e)


@functools.lru_cache(maxsize=None)
def gmean_ref(M, type, e=0):
    if e:  # A # B scales with the pair; the means with an inverse do not
        ref, g = gmean_ref(M, type)
        return _x2(ref, e if type == 1 else 0), g
    A, Bm, _ = pair_case(M)
    return lr.gmeanmh(A, Bm, type)


@functools.lru_cache(maxsize=None)
def general_ref(M, type, e=0):
    if e:  # A z = lam B z keeps its eigenvalues; A B and B A square the scale
        return _x2(general_ref(M, type), 0 if type == 1 else 2 * e)
    A, Bm, _ = pair_case(M)
    return lr.eigh_general(A, Bm, type)[0]


@functools.lru_cache(maxsize=None)
def solve_case(Nn, nrhs, e=0):
    A, Bm, names = lr.gen_systems(0, N, Nn, nrhs, 2.0 ** e)
    if e:
        _, _, _, ref, kap = solve_case(Nn, nrhs)
        return A, Bm, names, _x2(ref, -e), kap
    return A, Bm, names, lr.solve(A, Bm), lr.kappa2(A)


# ------------------------------------------------------------------------------- checks
def check_eigh(M, A, names, ref_lam, route, with_vectors=True):
    lam, V = run_eigh(A)
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(V))
    assert np.all(np.diff(lam, axis=-1) >= 0)
    record("eigh_eigenvalues", route, lr.eig_error(lam, ref_lam), lr.C["eig"], names)
    record("eigh_residual", route, lr.residual(A, lam, V), lr.C["res"], names)
    record("eigh_orthonormality", route, lr.orthonormality(V), lr.C["orth"], names)
    if M == 2 and with_vectors:
        # eigenvectors WITH np.linalg.eigh's phases where the relative gap is 0.1 or more (the
        # scaled identity and every other close pair: eigenvalues, residual, orthonormality only)
        gap = lr.relgap2(A)
        keep = gap >= 0.1
        Vn = np.linalg.eigh(lr.herm(A))[1]
        err = lr.ratio(lr.fro(V.astype(np.clongdouble) - Vn), 2 * pr.U / np.where(keep, gap, 1.0))
        record("eigh_vectors_with_phases", route, np.where(keep, err, 0.0), lr.C["res"], names)
    return lam, V


@pytest.mark.parametrize("M", lr.SIZES)
def test_eigh(M):
    A, names, ref = herm_case(M)
    first = None
    for n in BATCHES:
        out = check_eigh(M, A[:n], names[:n], ref[:n], "{} n{}".format(eigh_route(M), n))
        first = first or out
    again = run_eigh(A)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), "two runs differ"


@pytest.mark.parametrize("e", ONE_SCALES)
@pytest.mark.parametrize("M", lr.SIZES)
def test_eigh_scaled(M, e):
    A, names, ref = herm_case(M, e)
    check_eigh(M, A, names, ref, "{} n{} x2^{}".format(eigh_route(M), N, e))


def check_psd(M, A, names, flooring, ref, route):
    out = run_to_psd(A, flooring)
    assert np.all(np.isfinite(out))
    record("to_psd", route, lr.fn_error(out, ref[0], ref[1]), lr.C["psd"], names)
    assert np.array_equal(out, np.swapaxes(out, -1, -2).conj()), "to_psd: not Hermitian to the last bit"
    return out


@pytest.mark.parametrize("M", lr.SIZES)
def test_to_psd(M):
    A, names, _ = herm_case(M)
    tag = eigh_route(M) + (" LDS rebuild" if M == 6 else "")
    for fl in FLOORS:
        ref = psd_ref(M, fl)
        for n in (BATCHES if fl == MAX_HALF else (N,)):
            out = check_psd(M, A[:n], names[:n], fl, (ref[0][:n], ref[1][:n]),
                            "{} n{} floor{} eps{:g}".format(tag, n, fl[0], fl[1]))
            if n == N and fl == MAX_HALF:
                assert np.array_equal(out, run_to_psd(A, fl)), "two runs differ"


@pytest.mark.parametrize("e", ONE_SCALES)
@pytest.mark.parametrize("M", lr.SIZES)
def test_to_psd_scaled(M, e):
    A, names, _ = herm_case(M, e)
    check_psd(M, A, names, NOF, psd_ref(M, NOF, e), "{} n{} x2^{}".format(eigh_route(M), N, e))


def check_sqrt(M, A, names, inverse, flooring, ref, route):
    out = run_sqrtmh(A, inverse, flooring)
    assert np.all(np.isfinite(out))
    key = "invsqrt" if inverse else "sqrt"
    record(key + "mh", route, lr.fn_error(out, ref[0], ref[1]), lr.C[key], names,
           "(g max {:.3g})".format(float(np.max(ref[1]))))
    assert lr.hermitian_defect(out).max() <= 2.0, key + "mh: not Hermitian within 2 u"
    return out


@pytest.mark.parametrize("M", HERM_SIZES)
def test_sqrtmh_invsqrtmh(M):
    A, names = pd_case(M)
    for n in BATCHES:
        ref = sqrt_ref(M, 0, NOF)
        check_sqrt(M, A[:n], names[:n], 0, NOF, (ref[0][:n], ref[1][:n]), "{} n{}".format(fn_route(M), n))
    for fl in FLOORS:
        ref = sqrt_ref(M, 1, fl)
        for n in (BATCHES if fl == MAX_HALF else (N,)):
            out = check_sqrt(M, A[:n], names[:n], 1, fl, (ref[0][:n], ref[1][:n]),
                             "{} n{} floor{} eps{:g}".format(fn_route(M), n, fl[0], fl[1]))
            if n == N and fl == MAX_HALF:
                assert np.array_equal(out, run_sqrtmh(A, 1, fl)), "two runs differ"


@pytest.mark.parametrize("e", ONE_SCALES)
@pytest.mark.parametrize("M", HERM_SIZES)
def test_sqrtmh_invsqrtmh_scaled(M, e):
    A, names = pd_case(M, e)
    for inverse in (0, 1):
        check_sqrt(M, A, names, inverse, NOF, sqrt_ref(M, inverse, NOF, e),
                   "{} n{} x2^{}".format(fn_route(M), N, e))


def check_gmean(M, type, A, Bm, names, ref, route):
    out = run_gmeanmh(A, Bm, type)
    assert np.all(np.isfinite(out))
    record("gmeanmh_type{}".format(type), route, lr.fn_error(out, ref[0], ref[1]), lr.C["gmean"], names)
    assert lr.hermitian_defect(out).max() <= 2.0, "gmeanmh: not Hermitian within 2 u"
    return out


@pytest.mark.parametrize("type", [1, 2, 3])
@pytest.mark.parametrize("M", HERM_SIZES)
def test_gmeanmh(M, type):
    A, Bm, names = pair_case(M)
    ref = gmean_ref(M, type)
    first = None
    for n in BATCHES:
        out = check_gmean(M, type, A[:n], Bm[:n], names[:n], (ref[0][:n], ref[1][:n]),
                          "{} n{}".format(fn_route(M), n))
        first = out if first is None else first
    assert np.array_equal(first, run_gmeanmh(A, Bm, type)), "two runs differ"


@pytest.mark.parametrize("e", TWO_SCALES)
@pytest.mark.parametrize("type", [1, 2, 3])
@pytest.mark.parametrize("M", HERM_SIZES)
def test_gmeanmh_scaled(M, type, e):
    A, Bm, names = pair_case(M, e)
    check_gmean(M, type, A, Bm, names, gmean_ref(M, type, e), "{} n{} x2^{}".format(fn_route(M), N, e))


def check_general(entry, M, type, A, Bm, names, ref_lam, route, skip=()):
    """`skip`: matrices whose B was made indefinite (nothing asserted about them)."""
    lam, Z, info = run_general(A, Bm, type, entry)
    keep = np.array([i not in skip for i in range(A.shape[0])])
    lam, Z, A, Bm, ref_lam = lam[keep], Z[keep], A[keep], Bm[keep], ref_lam[keep]
    names = [k for k, ok in zip(names, keep) if ok]
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(Z))
    assert np.all(np.diff(lam, axis=-1) >= 0)
    e, r, o = lr.general_measures(A, Bm, type, lam, Z, ref_lam)
    name = "{}_type{}".format(entry, type)
    record(name + "_eigenvalues", route, e, lr.C["geig"], names)
    record(name + "_residual", route, r, lr.C["gres"], names)
    record(name + "_B_orthonormality", route, o, lr.C["gorth"], names)
    return info


def general_entries(M):
    return ("eigh2", "eigh_general") if M == 2 else ("eigh_general",)


def general_route(entry, M):
    return "k_eigh2" if entry == "eigh2" else fn_route(M)


@pytest.mark.parametrize("type", [1, 2, 3])
@pytest.mark.parametrize("M", HERM_SIZES)
def test_eigh_general(M, type):
    A, Bm, names = pair_case(M)
    ref = general_ref(M, type)
    for entry in general_entries(M):
        for n in BATCHES:
            info = check_general(entry, M, type, A[:n], Bm[:n], names[:n], ref[:n],
                                 "{} n{}".format(general_route(entry, M), n))
            assert info == 0
        a, b = run_general(A, Bm, type, entry), run_general(A, Bm, type, entry)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "two runs differ"


@pytest.mark.parametrize("e", TWO_SCALES)
@pytest.mark.parametrize("type", [1, 2, 3])
@pytest.mark.parametrize("M", HERM_SIZES)
def test_eigh_general_scaled(M, type, e):
    A, Bm, names = pair_case(M, e)
    for entry in general_entries(M):
        info = check_general(entry, M, type, A, Bm, names, general_ref(M, type, e),
                             "{} n{} x2^{}".format(general_route(entry, M), N, e))
        assert info == 0


@pytest.mark.parametrize("M", [2, 5, 8, 16])
def test_eigh_general_counts_indefinite_b(M):
    """Two indefinite B among 72: info is nonzero, every other matrix within its bars."""
    A, Bm, names = pair_case(M)
    bad = (9, 44)
    Bb = Bm.copy()
    for i in bad:
        Bb[i] = -Bb[i]
    for entry in general_entries(M):
        info = check_general(entry, M, 1, A, Bb, names, general_ref(M, 1),
                             "{} n{} 2 indefinite B".format(general_route(entry, M), N), skip=bad)
        assert info != 0


@pytest.mark.parametrize("M", lr.SIZES)
def test_herm_rebuild(M):
    P, w = lr.gen_rebuild(0, N, M)
    names = lr.gen_hermitian(0, N, M)[1]
    for hermitise in (0, 1):
        ref, g = lr.herm_rebuild(P, w, hermitise)
        for n in BATCHES:
            out = run_rebuild(P[:n], w[:n], hermitise)
            record("herm_rebuild", "M{} n{} hermitise{}".format(M, n, hermitise),
                   lr.fn_error(out, ref[:n], g[:n]), lr.C["rebuild"], names[:n])
            if hermitise:
                assert lr.hermitian_defect(out).max() <= 2.0


# ------------------------------------------------------------------------------- solves
def solve_route(Nn):
    return "k_solve<{}>".format(Nn) if Nn <= 8 else "solve_rt N{}".format(Nn)


def check_solve(Nn, A, Bm, names, ref, kap, route, skip=()):
    X, info = run_solve(A, Bm)
    keep = np.array([i not in skip for i in range(A.shape[0])])
    assert np.all(np.isfinite(X[keep]))
    record("solve", route, lr.solve_error(X[keep], ref[keep], kap[keep]), lr.C["solve"],
           [k for k, ok in zip(names, keep) if ok], "(kappa max {:.3g})".format(float(kap[keep].max())))
    return X, info


@pytest.mark.parametrize("Nn", lr.SOLVE_SIZES)
def test_solve(Nn):
    for nrhs in sorted({1, 3, Nn}):
        A, Bm, names, ref, kap = solve_case(Nn, nrhs)
        for n in (N, 65):
            X, info = check_solve(Nn, A[:n], Bm[:n], names[:n], ref[:n], kap[:n],
                                  "{} nrhs{} n{}".format(solve_route(Nn), nrhs, n))
            assert info == 0
        assert np.array_equal(X, run_solve(A[:65], Bm[:65])[0]), "two runs differ"


@pytest.mark.parametrize("e", ONE_SCALES)
@pytest.mark.parametrize("Nn", lr.SOLVE_SIZES)
def test_solve_scaled(Nn, e):
    A, Bm, names, ref, kap = solve_case(Nn, 3, e)
    _, info = check_solve(Nn, A, Bm, names, ref, kap, "{} nrhs3 n{} x2^{}".format(solve_route(Nn), N, e))
    assert info == 0


@pytest.mark.parametrize("Nn", [4, 16])
def test_solve_counts_singular_systems(Nn):
    """Three exactly singular systems (a zero row) among 72: info reads 3, the other 69 meet the bar."""
    A, Bm, names, ref, kap = solve_case(Nn, 3)
    bad = (5, 40, 71)
    As = A.copy()
    for i in bad:
        As[i, Nn // 2, :] = 0
    _, info = check_solve(Nn, As, Bm, names, ref, kap, "{} n{} 3 singular".format(solve_route(Nn), N),
                          skip=bad)
    assert info == 3


def test_inv2():
    A, _, names = lr.gen_systems(0, N, 2, 1)
    ref, kap = lr.inv2(A), lr.kappa2(A)
    for n in (N, 257, 1):   # k_inv2: 256 lanes per block
        reps = -(-n // N)
        An = np.concatenate([A] * reps)[:n]
        out = run_inv2(An)
        record("inv2", "k_inv2 n{}".format(n),
               lr.fn_error(out, np.concatenate([ref] * reps)[:n], np.concatenate([kap] * reps)[:n]),
               lr.C["inv2"], (names * reps)[:n])


# ------------------------------------------------------------------------------- NaN isolation
@pytest.mark.parametrize("M", [3, 8])
def test_eigh_nan_matrix_leaves_its_wave_alone(M):
    """One NaN matrix in the middle of a wave: the vote then runs all 12 sweeps for every lane, and
    every other matrix still meets its bars.  Nothing is asserted about the NaN matrix."""
    A, names, ref = herm_case(M)
    An = A.copy()
    bad = 27
    An[bad] = np.nan
    lam, V = run_eigh(An)
    keep = np.arange(N) != bad
    route = "{} n{} NaN at {}".format(eigh_route(M), N, bad)
    kept = [k for k, ok in zip(names, keep) if ok]
    assert np.all(np.isfinite(lam[keep])) and np.all(np.isfinite(V[keep]))
    record("eigh_eigenvalues", route, lr.eig_error(lam[keep], ref[keep]), lr.C["eig"], kept)
    record("eigh_residual", route, lr.residual(A[keep], lam[keep], V[keep]), lr.C["res"], kept)
    record("eigh_orthonormality", route, lr.orthonormality(V[keep]), lr.C["orth"], kept)


# ------------------------------------------------------------------------------- profile
def _write_profile(raw, path):
    worst = {}
    for line in open(raw):
        f = line.rstrip("\n").split("\t")
        key = (f[0], f[1].split(" | ")[0])   # the worst family of every (entry, route)
        if key not in worst or float(f[4]) > float(worst[key][4]):
            worst[key] = f
    with open(path, "w") as out:
        out.write("# largest measured error of every entry point and route (| the input family that reaches "
                  "it), tests/test_gpu_linalg_elementwise.py on an MI355X\n# per matrix, in the normalised units of tests/"
                  "linalg_reference.py (g u scale); bar = 8 x the float64 restatement's own error\n"
                  "# (MEASURED: {}); ratio = error / bar\n".format(
                      ", ".join("{} {:g}".format(k, v) for k, v in sorted(lr.MEASURED.items()))))
        for key in sorted(worst):
            f = worst[key]
            out.write("{:34s} {:72s} err {:>10s}  bar {:>9s}  ratio {}{}\n".format(
                f[0], f[1], f[2], f[3], f[4], "  " + f[5] if len(f) > 5 and f[5] else ""))


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles")
    raw = os.path.join(out_dir, "linalg_elementwise.raw")
    if os.path.exists(raw):
        os.remove(raw)
    os.environ["SSSPY_PASS_PROFILE_RAW"] = raw
    rc = pytest.main([os.path.abspath(__file__), "-m", "gpu", "-q", "--maxfail=40", "--durations=8"]
                     + sys.argv[2:])
    if os.path.exists(raw):
        _write_profile(raw, os.path.join(out_dir, "linalg_elementwise.txt"))
        os.remove(raw)
    sys.exit(int(rc))
