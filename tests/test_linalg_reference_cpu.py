"""tests/linalg_reference.py on the CPU: the long-double restatement satisfies the defining identities
to a few long-double ulps on every family, the float64 restatement stays under every bar (the bars
are attainable), MEASURED holds the freshly measured yardsticks by the "8 times, rounded up to two
digits" rule, and six mutants of the restatement each break their own bar (the bars notice).  No
kernel is built or run here."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linalg_reference as lr  # noqa: E402
import pass_reference as pr  # noqa: E402

LD, U = pr.LD, pr.U
LD_FEW_ULPS = 0.125  # in u = 2^-53: 256 long-double ulps (2^-64) -- sums of up to 16 terms, three
#                      products deep; or a twentieth of the float64 yardstick the reference measures
#                      (the kappa-normalised residual of the generalised problem: 5.4 u)
MAX_HALF = (pr.FLOOR_MAX, 0.5)


@pytest.fixture(scope="module")
def measured():
    return lr.measure_all()


def test_float64_restatement_meets_every_bar(measured):
    for k, v in sorted(measured.items()):
        print("float64", k, round(v, 4), "bar", lr.C[k])
        assert v <= lr.C[k], (k, v)
    assert set(measured) == set(lr.C)


def test_constants_are_eight_times_the_yardsticks(measured):
    """MEASURED is the largest normalised float64 error over the families and sizes, rounded up to
    two digits (at most 10 % above), and C = 8 x MEASURED."""
    for k, v in sorted(measured.items()):
        print("yardstick", k, round(v, 4), "MEASURED", lr.MEASURED[k])
        assert v <= lr.MEASURED[k] <= 1.10 * v + 0.01, (k, v, lr.MEASURED[k])
        assert lr.C[k] == 8.0 * lr.MEASURED[k]


@pytest.mark.parametrize("M", [1, 2, 3, 8, 16])
def test_long_double_identities(M):
    A, _ = lr.gen_hermitian(0, lr.N_BATCH, M)
    lam, V = lr.eigh(A)
    assert np.all(np.diff(lam, axis=-1) >= 0)
    worst = {"res": lr.residual(A, lam, V).max(), "orth": lr.orthonormality(V).max()}
    Hm = lr.herm(A.astype(np.clongdouble))
    worst["psd"] = lr.fn_error(lr.to_psd(A, lr.NOF)[0], Hm, 1.0).max()
    if M >= 2:
        P = lr.gen_pd(0, lr.N_BATCH, M)
        Ph = lr.herm(P.astype(np.clongdouble))
        S, g = lr.sqrtmh(P)
        worst["sqrt"] = lr.fn_error(S @ S, Ph, g).max()
        R, g = lr.invsqrtmh(P)
        eye = np.broadcast_to(np.eye(M, dtype=np.clongdouble), Ph.shape)
        worst["invsqrt"] = lr.fn_error(R @ Ph @ R, eye, g).max()
        A2, B2, _ = lr.gen_pd_pairs(0, lr.N_BATCH, M)
        Ac, Bc = A2.astype(np.clongdouble), B2.astype(np.clongdouble)
        for t in (1, 2, 3):
            lam, Z = lr.eigh_general(A2, B2, t)
            _, r, o = lr.general_measures(A2, B2, t, lam, Z, lam)
            worst["gres%d" % t], worst["gorth%d" % t] = r.max(), o.max()
            G, g = lr.gmeanmh(A2, B2, t)   # the Riccati identity of each type
            left = G @ (Ac if t == 2 else lr.inv(Ac)) @ G
            worst["gmean%d" % t] = lr.fn_error(left, lr.inv(Bc) if t == 3 else Bc, g * g).max()
    for N in (M,):
        As, Bs, _ = lr.gen_systems(0, lr.N_BATCH, N, 3)
        X = lr.solve(As, Bs)
        back = lr.solve_error(As.astype(np.clongdouble) @ X, Bs.astype(np.clongdouble), lr.kappa2(As))
        worst["solve"] = back.max()
    for k, v in worst.items():
        print("long double", M, k, float(v))
        assert v <= max(LD_FEW_ULPS, 0.05 * lr.MEASURED[k.rstrip("123")]), (M, k, v)


def _of_kind(A, names, kind):
    keep = [i for i, k in enumerate(names) if k == kind]
    return np.ascontiguousarray(A[keep])


def _mutant_sweeps(M):
    A = _of_kind(*lr.gen_hermitian(0, lr.N_BATCH, M), "clustered")
    lam, V = lr.eigh(A, np.float64, "sweeps")
    return {"res": lr.residual(A, lam, V).max()}


def _mutant_lower(M):
    A = _of_kind(*lr.gen_hermitian(0, lr.N_BATCH, M), "non_hermitian")
    return {"eig": lr.eig_error(lr.eigh(A, np.float64, "lower")[0], lr.eigh(A)[0]).max()}


def _mutant_floor_lam(M):
    A = lr.gen_pd(0, lr.N_BATCH, M)
    ref, g = lr.invsqrtmh(A, MAX_HALF)
    return {"invsqrt": lr.fn_error(lr.invsqrtmh(A, MAX_HALF, np.float64, "floor_lam")[0], ref, g).max()}


def _mutant_ties(M):
    A = _of_kind(*lr.gen_hermitian(0, lr.N_BATCH, M), "identity")
    return {"orth": lr.orthonormality(lr.eigh(A, np.float64, "ties_by_value")[1]).max()}


def _mutant_no_pivot(N):
    return {"solve": lr.solve_yardsticks(N, mutant="no_pivot")["solve"]}


def _mutant_swap(M):
    r = lr.yardsticks(M, mutant="swap_types", keys=("gmean", "geig"))
    # (A B and B A share their eigenvalues: the swap shows in the vectors, residual and metric)
    return {"gmean": r["gmean"], "gres": r["gres"], "gorth": r["gorth"]}


# mutant -> (what it does, sizes it is tried at): every quantity it returns must pass its bar there
MUTANTS = {
    "sweeps": (_mutant_sweeps, (3, 8)),          # one Jacobi sweep too few on the clustered family
    "lower": (_mutant_lower, (2, 8)),            # the lower triangle instead of the Hermitian part
    "floor_lam": (_mutant_floor_lam, (3, 8)),    # floor on lam instead of sqrt(lam)
    "ties_by_value": (_mutant_ties, (2, 8)),     # ties ordered by value only
    "no_pivot": (_mutant_no_pivot, (2, 8)),      # a solve without row exchanges
    "swap_types": (_mutant_swap, (2, 7)),        # type 2 and type 3 swapped
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_breaks_its_bar(mutant):
    fn, sizes = MUTANTS[mutant]
    for M in sizes:
        for k, v in fn(M).items():
            print(mutant, M, k, float(v), "bar", lr.C[k])
            assert not v <= lr.C[k], "mutant {} survives at {} on {}: {}".format(mutant, M, k, v)


def test_generators_interleave_the_families():
    """Every group of 8 consecutive matrices holds 8 different kinds; B takes each kappa_2 in turn."""
    for M in (2, 7):
        _, names = lr.gen_hermitian(0, lr.N_BATCH, M)
        assert all(len(set(names[i:i + 8])) == 8 for i in range(0, lr.N_BATCH, 8))
        assert set(names) == set(lr.hermitian_kinds(M))
        _, Bm, _ = lr.gen_pd_pairs(0, lr.N_BATCH, M)
        k = lr.kappa2(Bm)
        for i, e in enumerate((1e0, 1e4, 1e8)):
            assert np.all(np.abs(k[i::3] / e - 1) < 1e-3), (M, e, k[i::3])
