"""The bars of tests/mnmf_reference.py are attainable, and its formulas are the reference's: on the
inputs of the GPU cases the float64 evaluation of every restated FastGaussMNMF entry point stays
within its own bar of the extended-precision one, and one whole update_once agrees with oracle/mnmf.py
to the oracle's precision.  No GPU."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mnmf_reference as mr  # noqa: E402
import pass_reference as pr  # noqa: E402

LD = pr.LD
MAXF, ADDF, NOF = (pr.FLOOR_MAX, pr.EPS), (pr.FLOOR_ADD, pr.EPS), (pr.FLOOR_NONE, 0.0)
# (B, N, M, F, T, K): the families of the GPU cases at their smallest members
SHAPES = [(2, 2, 2, 17, 32, 3), (1, 2, 3, 17, 34, 8), (2, 3, 4, 17, 33, 9), (1, 4, 4, 65, 32, 16),
          (1, 3, 3, 17, 32, 17), (1, 2, 2, 17, 32, 40), (1, 5, 5, 9, 65, 5), (1, 2, 6, 9, 65, 20),
          (1, 1, 3, 9, 65, 8), (1, 6, 2, 9, 65, 9), (1, 9, 9, 9, 40, 4), (1, 3, 16, 9, 40, 9)]


def _within(name, f64, ref, bar):
    err = np.abs(np.asarray(f64).astype(ref.dtype) - ref)
    ratio = float(np.max(err / bar))
    print("{}: float64 / bar = {:.3f}".format(name, ratio))
    assert np.all(np.isfinite(np.asarray(f64, dtype=np.complex128)))
    assert ratio <= 1.0, "{}: the float64 evaluation leaves its own bar ({:.3f})".format(name, ratio)


@pytest.mark.parametrize("flooring", [MAXF, ADDF])
@pytest.mark.parametrize("B,N,M,F,T,K", SHAPES)
def test_float64_within_bars(B, N, M, F, T, K, flooring):
    X, C, Q, D, basis, act = mr.gen_state(B + N + M + F + T + K, B, N, M, F, T, K)
    f = np.float64
    for name, fn, args in (
            ("weights", mr.fastmnmf_weights, (D, basis, act)),
            ("diagonalizer_covariance", mr.fastmnmf_diagonalizer_covariance, (X, D, basis, act)),
            ("basis", mr.update_basis, (X, Q, D, basis, act, flooring)),
            ("activation", mr.update_activation, (X, Q, D, basis, act, flooring)),
            ("spatial", mr.update_spatial, (X, Q, D, basis, act)),
            ("loss_data", mr.loss_data, (X, Q, D, basis, act)),
            ("handover", mr.handover_buffer, (X, Q))):
        ref, bar = fn(*args)
        _within(name, fn(*args, dtype=f)[0], ref, bar)
    Qn, barQ, Dn, barD, psi = mr.normalize(Q, C, D, flooring)
    Qf, _, Df, _, _ = mr.normalize(Q, C, D, flooring, dtype=f)
    _within("normalize_Q", Qf, Qn, barQ)
    _within("normalize_D", Df, Dn, barD)


@pytest.mark.parametrize("flooring", [MAXF, ADDF])
def test_float64_within_bars_floored(flooring):
    """The floor active on a share of the updated values, and on a known set of psi."""
    B, N, M, F, T, K = 2, 3, 3, 17, 32, 8
    X, C, Q, D, basis, act = mr.gen_floor_state(5, B, N, M, F, T, K)
    for name, fn in (("basis", mr.update_basis), ("activation", mr.update_activation)):
        ref, bar = fn(X, Q, D, basis, act, flooring)
        if flooring[0] == pr.FLOOR_MAX:
            share = float(np.mean(ref == LD(pr.EPS)))
            assert 0.05 < share < 0.95, share
        _within(name + "_floored", fn(X, Q, D, basis, act, flooring, dtype=np.float64)[0], ref, bar)
    X, C, Q, D, basis, act = mr.gen_state(6, B, N, M, F, T, K)
    Qs, floored = mr.gen_floor_rows(Q, C)
    Qn, barQ, Dn, barD, psi = mr.normalize(Qs, C, D, flooring)
    if flooring[0] == pr.FLOOR_MAX:
        assert np.array_equal(psi == LD(pr.EPS), floored)
    Qf, _, Df, _, _ = mr.normalize(Qs, C, D, flooring, dtype=np.float64)
    _within("normalize_Q_floored", Qf, Qn, barQ)
    _within("normalize_D_floored", Df, Dn, barD)


@pytest.mark.parametrize("B,N,M,F,T,K", [(2, 3, 3, 17, 32, 8), (1, 2, 4, 9, 40, 4), (1, 5, 6, 9, 33, 5)])
def test_update_once_agrees_with_the_oracle(B, N, M, F, T, K):
    """One update_once of the extended restatement against oracle/mnmf.py (float64, written from the
    reference independently): 1e-11 relative, what float64 leaves of a chain of five steps whose
    solves have kappa <= 1e3.  The same for the loss and the unfloored Wiener filter."""
    from oracle.mnmf import FastGaussMNMFOracle

    X, C, Q, D, basis, act = mr.gen_state(40 + M, B, N, M, F, T, K)
    Q1, D1, b1, a1 = mr.update_once(X, C, Q, D, basis, act, MAXF)
    loss, _ = mr.loss_data(X, Q, D, basis, act)
    Y, kappa, lam_min = mr.separate(X, Q1, D1, b1, a1, 0, MAXF)
    assert float(lam_min.min()) > 1e3 * pr.EPS  # the eigenvalue floor of to_psd is inactive
    for b in range(B):
        o = FastGaussMNMFOracle(n_basis=K, n_sources=N, record_loss=False)
        o.reset(X[b], basis=basis[b], activation=act[b], diagonalizer=Q[b], spatial=D[b])
        ld = float(np.sum(np.log(np.abs(np.linalg.det(Q[b])))))
        assert abs(o.compute_loss() + 2 * ld - float(loss[b])) <= 1e-11 * abs(float(loss[b]))
        o.update_once()
        for got, ref in ((o.diagonalizer, Q1[b]), (o.spatial, D1[b]), (o.basis, b1[b]),
                         (o.activation, a1[b])):
            err = np.max(np.abs(got - ref.astype(got.dtype))) / np.max(np.abs(got))
            assert err <= 1e-11, err
        Yo = o.separate(X[b])
        err = np.max(np.abs(Yo - Y[b].astype(np.complex128))) / np.max(np.abs(Yo))
        assert err <= 1e-10 * max(1.0, float(kappa[b].max()) / 16), err


@pytest.mark.parametrize("B,N,M,F,T,K", [(2, 3, 3, 17, 32, 8), (1, 2, 4, 9, 40, 4), (1, 9, 9, 9, 40, 4)])
def test_ip1_and_wiener_yardsticks(B, N, M, F, T, K):
    """The c inputs of the normwise bars: the kappa-normalised error of the float64 composition is a
    small multiple of u (a backward-stable solve of M unknowns: a few M at most), so c = 8 x it is
    a bar and not a blank cheque."""
    X, C, Q, D, basis, act = mr.gen_state(60 + M, B, N, M, F, T, K)
    ref, kappa = mr.update_diagonalizer(X, Q, D, basis, act, MAXF)
    f64 = mr.ip1_yardstick(X, Q, D, basis, act, MAXF)  # np.linalg.solve on the reference's own U
    c_np = pr.ip1_row_error(f64, ref, kappa)
    print("IP1 c_np {:.3f} kappa max {:.1f}".format(c_np, float(kappa.max())))
    assert kappa.max() <= 1e3 and 0 < c_np <= 4 * M
    for flooring in (MAXF, ADDF, (pr.FLOOR_ADD, 0.3)):
        Y, kap, lam_min = mr.separate(X, Q, D, basis, act, 0, flooring)
        Yf = mr.separate_float64(X, Q, D, basis, act, 0, flooring)
        c_w = mr.separate_error(Yf, Y, X, kap)
        print("Wiener c_np {:.3f} kappa max {:.1f}".format(c_w, float(kap.max())))
        assert 0 < c_w <= 4 * M


def test_eigh_jacobi():
    """The long-double eigendecomposition of the active-floor Wiener reference: A = V diag(w) V^H and
    V unitary to extended precision, eigenvalues those of np.linalg.eigvalsh to float64's."""
    rng = np.random.default_rng(3)
    for M in (2, 3, 4, 9, 16):
        A = rng.standard_normal((20, M, M)) + 1j * rng.standard_normal((20, M, M))
        A = (A + np.swapaxes(A, -1, -2).conj()).astype(np.clongdouble)
        w, V = mr.eigh_jacobi(A)
        rec = np.einsum("nam,nm,ncm->nac", V, w.astype(np.clongdouble), V.conj())
        assert float(np.abs(rec - A).max()) <= 64 * M * float(np.finfo(LD).eps) * float(np.abs(A).max())
        assert float(np.abs(np.einsum("nma,nmc->nac", V.conj(), V) - np.eye(M)).max()) <= 1e-17
        ev = np.linalg.eigvalsh(A.astype(np.complex128))
        assert np.allclose(np.sort(w.astype(np.float64), axis=1), ev, rtol=0, atol=1e-12)


@pytest.mark.parametrize("B,N,M,F,T,K", [(2, 3, 3, 17, 33, 8), (1, 5, 5, 9, 65, 8), (1, 3, 9, 9, 40, 4)])
def test_wiener_active_floor_yardstick(B, N, M, F, T, K):
    """MAX, eps = 0.3, about half of the eigenvalues floored: the float64 composition stays a small
    multiple of kappa u from the extended reference, and with an inactive floor the eigendecomposition
    route of the reference agrees with the direct one."""
    fl = (pr.FLOOR_MAX, 0.3)
    X, C, Q, D, basis, act = mr.gen_wiener_floor_state(9 + M + K, B, N, M, F, T, K, 0.3)
    Y, kap, lam = mr.separate(X, Q, D, basis, act, M - 1, fl, eig=True)
    assert 0.3 < float(np.mean(lam < 0.3)) < 0.7
    c_w = mr.separate_error(mr.separate_float64(X, Q, D, basis, act, M - 1, fl), Y, X, kap)
    print("Wiener (active floor) c_np {:.3f} kappa max {:.1f}".format(c_w, float(kap.max())))
    assert 0 < c_w <= 4 * M
    X, C, Q, D, basis, act = mr.gen_state(9, B, N, M, F, T, K)
    Y1 = mr.separate(X, Q, D, basis, act, 0, MAXF, eig=True)[0]
    Y0 = mr.separate(X, Q, D, basis, act, 0, MAXF)[0]
    assert float(np.abs(Y1 - Y0).max()) <= 1e-15 * float(np.abs(Y0).max())
