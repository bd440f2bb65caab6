"""The forms of the three ILRMA pass kernels on the tuned (n_sources <= 4) path.

Two forms are chosen at run time: the full-tile instances (n_basis == 16 and T a multiple of 16, the
plain Gauss model with a filter: no k or frame masks in the walks) and the masked ones for every other
shape.  At 4 sources the covariance pass splits x x^H between the two waves of a bin tile by
component (Gauss-family models) or by source (t, GGD).  Every form must give the oracle's numbers, the
step methods must equal the fused update, a batch must equal its single-mixture runs (small path, split
tail items and unsplit items), and a run must repeat bit for bit.
"""

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-8
LOSS_RTOL = 1e-9


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _inputs(seed, N, F, T, K):
    from ssspy_amd.utils.dataset import nmf_mixture

    X = nmf_mixture(seed, N, F, T)
    rng = np.random.default_rng(seed + 1)
    return X, rng.random((N, F, K)), rng.random((N, K, T))


@pytest.mark.parametrize("T", [512, 500])
@pytest.mark.parametrize("K", [4, 12, 16, 32])
def test_fused_update_against_oracle(K, T):
    """update_once() (IP1, N = 4, F = 65: a ragged bin edge) against the oracle, loss included;
    K = 16 at T = 512 runs the full-tile instances, the others the masked ones."""
    from oracle.ilrma import GaussILRMAOracle
    from ssspy_amd.bss.ilrma import GaussILRMA

    N, F = 4, 65
    X, basis, act = _inputs(500 + K + T, N, F, T, K)
    ref = GaussILRMAOracle(n_basis=K)
    Yr = ref.run(X, n_iter=3, basis=basis, activation=act)
    m = GaussILRMA(n_basis=K)
    Y = m(X, n_iter=3, basis=basis, activation=act)
    assert rel_err(Y, Yr) < TOL
    assert rel_err(m.demix_filter, ref.demix_filter) < TOL
    assert rel_err(m.basis, ref.basis) < TOL and rel_err(m.activation, ref.activation) < TOL
    np.testing.assert_allclose(m.loss, ref.loss, rtol=LOSS_RTOL)


@pytest.mark.parametrize("K,T", [(16, 512), (12, 500)])
def test_step_methods_match_fused_update(K, T):
    """The public per-step methods == the fused update_once(), full-tile and masked shapes."""
    from ssspy_amd.bss.ilrma import GaussILRMA

    class Stepwise(GaussILRMA):
        def normalize(self, flooring_fn="self"):  # overriding forces the step-by-step path
            super().normalize(flooring_fn=flooring_fn)

    X, basis, act = _inputs(700 + K, 4, 65, T, K)
    outs = []
    for cls in (GaussILRMA, Stepwise):
        m = cls(n_basis=K)
        outs.append((m(X, n_iter=3, basis=basis, activation=act), m.basis, m.activation))
    for a, b in zip(*outs):
        assert rel_err(b, a) < 1e-12


@pytest.mark.parametrize("B", [1, 8, 40])
def test_batches_equal_single_mixtures(B):
    """The headline shape (N = 4, F = 1025, T = 512, n_basis = 16) in batches of 1 (small path), 8
    (split items only) and 40 (unsplit items and a split tail); the first and last mixture against
    their single-mixture runs, the first also against the oracle at B = 1."""
    import torch

    from oracle.ilrma import GaussILRMAOracle
    from ssspy_amd.bss.ilrma import GaussILRMA
    from ssspy_amd.utils.dataset import nmf_mixture_batch

    N, F, T, K = 4, 1025, 512, 16
    Xh = nmf_mixture_batch(900, B, N, F, T)
    rng = np.random.default_rng(901)
    basis, act = rng.random((B, N, F, K)), rng.random((B, N, K, T))
    mb = GaussILRMA(n_basis=K, scale_restoration=False)
    Yb = mb(torch.from_numpy(Xh).to("cuda") if B > 1 else Xh[0], n_iter=2,
            basis=basis if B > 1 else basis[0], activation=act if B > 1 else act[0])
    if B == 1:
        ref = GaussILRMAOracle(n_basis=K, scale_restoration=False)
        Yr = ref.run(Xh[0], n_iter=2, basis=basis[0], activation=act[0])
        assert rel_err(_np(Yb), Yr) < TOL
        assert rel_err(mb.basis, ref.basis) < TOL and rel_err(mb.activation, ref.activation) < TOL
        np.testing.assert_allclose(mb.loss, ref.loss, rtol=LOSS_RTOL)
        return
    Yb = _np(Yb)
    for b in (0, B - 1):
        m1 = GaussILRMA(n_basis=K, scale_restoration=False)
        Y1 = m1(Xh[b], n_iter=2, basis=basis[b], activation=act[b])
        assert rel_err(Yb[b], Y1) < 1e-10
        assert rel_err(_np(mb.basis)[b], m1.basis) < 1e-10
        assert rel_err(_np(mb.activation)[b], m1.activation) < 1e-10
        np.testing.assert_allclose(np.asarray(mb.loss)[:, b], m1.loss, rtol=1e-10)


@pytest.mark.parametrize("model", [("t", 3.0), ("ggd", 1.2)])
@pytest.mark.parametrize("T", [512, 500])
def test_heavy_tailed_covariance_pass_against_oracle(model, T):
    """t and GGD weights need |w_n^H x|^2: the covariance pass keeps the source split for them."""
    from oracle.ilrma import GaussILRMAOracle
    from ssspy_amd.bss.ilrma import GGDILRMA, TILRMA

    N, F, K = 4, 65, 16
    X, basis, act = _inputs(800 + T, N, F, T, K)
    ref = GaussILRMAOracle(n_basis=K, model=model, scale_restoration=False)
    Yr = ref.run(X, n_iter=3, basis=basis, activation=act)
    if model[0] == "t":
        m = TILRMA(n_basis=K, dof=model[1], scale_restoration=False)
    else:
        m = GGDILRMA(n_basis=K, beta=model[1], scale_restoration=False)
    Y = m(X, n_iter=3, basis=basis, activation=act)
    assert rel_err(Y, Yr) < TOL
    assert rel_err(m.basis, ref.basis) < TOL and rel_err(m.activation, ref.activation) < TOL
    np.testing.assert_allclose(m.loss, ref.loss, rtol=LOSS_RTOL)


@pytest.mark.parametrize("K,T", [(16, 512), (12, 500)])
def test_runs_repeat_bitwise(K, T):
    """Two runs of the same batch give the same bits (no atomics, fixed fold orders)."""
    import torch

    from ssspy_amd.bss.ilrma import GaussILRMA
    from ssspy_amd.utils.dataset import nmf_mixture_batch

    B, N, F = 6, 4, 257
    Xh = nmf_mixture_batch(950, B, N, F, T)
    rng = np.random.default_rng(951)
    basis, act = rng.random((B, N, F, K)), rng.random((B, N, K, T))
    outs = []
    for _ in range(2):
        m = GaussILRMA(n_basis=K)
        Y = m(torch.from_numpy(Xh).to("cuda"), n_iter=3, basis=basis, activation=act)
        outs.append((_np(Y), _np(m.demix_filter), _np(m.basis), _np(m.activation),
                     np.asarray(m.loss)))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
