"""GaussMNMF at 9-16 sources on 2-8 channels (the NX = 16 forms of csrc/gmnmf_kernels.hip): golden
replays of the reference, the NumPy oracle at shapes the fixtures do not reach, batches, determinism,
the step methods, record_loss, separate() and the bounds."""

import numpy as np
import pytest

from conftest import rel_err
from test_gpu_parity import test_gauss_mnmf_against_golden as _replay_gauss_mnmf_golden

pytestmark = pytest.mark.gpu

GOLDEN_CASES = ["gmnmf_m2_n9", "gmnmf_m4_n12", "gmnmf_m8_n16", "gmnmf_part_m3_n10",
                "gmnmf_m6_n16_nonorm_add", "gmnmf_floor_m5_n9"]


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_gauss_mnmf_sources_against_golden(case):
    """Snapshots, spatial, basis and output at 1e-7, loss at rtol 1e-8, latent where partitioned:
    the bar of the 8-source replays."""
    _replay_gauss_mnmf_golden(case)


def _init(seed, N, F, T, K, partitioning=False):
    rng = np.random.default_rng(seed)
    if partitioning:
        latent = rng.random((N, K))
        return dict(basis=rng.random((F, K)), activation=rng.random((K, T)),
                    latent=latent / latent.sum(axis=0))
    return dict(basis=rng.random((N, F, K)), activation=rng.random((N, K, T)))


# (M, N, K, partitioning): K = 40 walks more than 32 bases; the partitioned shape has K > N
ORACLE_SHAPES = [(2, 16, 2, False), (4, 9, 40, False), (8, 16, 8, False), (4, 16, 24, True)]


@pytest.mark.parametrize("shape", ORACLE_SHAPES,
                         ids=lambda s: "m{}_n{}_k{}{}".format(s[0], s[1], s[2], "_part" * s[3]))
def test_gauss_mnmf_sources_against_oracle(shape):
    from oracle.gmnmf import GaussMNMFOracle
    from ssspy_amd.bss.mnmf import GaussMNMF
    from ssspy_amd.utils.dataset import nmf_mixture

    M, N, K, part = shape
    F, T, n_iter = 17, 50, 6
    X = nmf_mixture(1100 + M + N, M, F, T)
    init = _init(1101 + K, N, F, T, K, part)
    ref = GaussMNMFOracle(n_basis=K, n_sources=N, partitioning=part)
    Yr = ref.run(X, n_iter=n_iter, **{k: v.copy() for k, v in init.items()})
    m = GaussMNMF(n_basis=K, n_sources=N, partitioning=part)
    Y = m(X, n_iter=n_iter, **{k: v.copy() for k, v in init.items()})
    np.testing.assert_allclose(m.loss, ref.loss, rtol=1e-8)
    for name in ("basis", "activation", "spatial") + (("latent",) if part else ()):
        assert rel_err(getattr(m, name), getattr(ref, name)) < 1e-7, name
    assert rel_err(Y, Yr) < 1e-7


def _run(x, state, **kwargs):
    from ssspy_amd.bss.mnmf import GaussMNMF

    m = GaussMNMF(**kwargs)
    y = m(x, n_iter=5, **{k: v.copy() for k, v in state.items()})
    return m, y


@pytest.mark.parametrize("part", [False, True], ids=["plain", "part"])
def test_gauss_mnmf_sources_batch_equals_single_runs_and_is_deterministic(part):
    from ssspy_amd.utils.dataset import nmf_mixture

    M, N, K, F, T = 4, 12, 14 if part else 4, 9, 40
    X = np.stack([nmf_mixture(1200 + b, M, F, T) for b in range(3)])
    init = [_init(1210 + b, N, F, T, K, part) for b in range(3)]
    batched = {k: np.stack([i[k] for i in init]) for k in init[0]}
    kw = dict(n_basis=K, n_sources=N, partitioning=part)
    names = ("basis", "activation", "spatial") + (("latent",) if part else ())
    mb, Yb = _run(X, batched, **kw)
    for b in range(3):
        ms, Ys = _run(X[b], init[b], **kw)
        assert rel_err(Yb[b], Ys) < 1e-10
        for name in names:
            assert rel_err(getattr(mb, name)[b], getattr(ms, name)) < 1e-10, name
        np.testing.assert_allclose(np.asarray(mb.loss)[:, b], ms.loss, rtol=1e-10)
    mb2, Yb2 = _run(X, batched, **kw)
    assert np.array_equal(Yb, Yb2)
    for name in names:
        assert np.array_equal(getattr(mb, name), getattr(mb2, name)), name
    assert np.array_equal(np.asarray(mb.loss), np.asarray(mb2.loss))


@pytest.mark.parametrize("part", [False, True], ids=["plain", "part"])
def test_gauss_mnmf_sources_step_methods_match_fused_update(part):
    from ssspy_amd.bss.mnmf import GaussMNMF
    from ssspy_amd.utils.dataset import nmf_mixture

    class Stepwise(GaussMNMF):
        def normalize(self, axis1=-2, axis2=-1):
            super().normalize(axis1=axis1, axis2=axis2)

    M, N, K, F, T = 5, 11, 13 if part else 3, 9, 70
    X = nmf_mixture(1300, M, F, T)
    init = _init(1301, N, F, T, K, part)
    kw = dict(n_basis=K, n_sources=N, partitioning=part)
    fused, Yf = _run(X, init, **kw)
    m = Stepwise(**kw)
    Ys = m(X, n_iter=5, **{k: v.copy() for k, v in init.items()})
    assert rel_err(Ys, Yf) < 1e-11
    for name in ("basis", "activation", "spatial") + (("latent",) if part else ()):
        assert rel_err(getattr(m, name), getattr(fused, name)) < 1e-11, name
    np.testing.assert_allclose(m.loss, fused.loss, rtol=1e-11)


def test_gauss_mnmf_sources_record_loss_with_and_without_callback():
    from ssspy_amd.utils.dataset import nmf_mixture

    M, N, K, F, T = 6, 16, 4, 9, 40
    X = nmf_mixture(1400, M, F, T)
    init = _init(1401, N, F, T, K)
    seen = []
    plain, Yp = _run(X, init, n_basis=K, n_sources=N)
    observed, Yo = _run(X, init, n_basis=K, n_sources=N,
                        callbacks=lambda m: seen.append(len(m.loss)))
    assert seen == [1, 2, 3, 4, 5, 6] and len(plain.loss) == 6
    np.testing.assert_allclose(plain.loss, observed.loss, rtol=1e-12)
    assert rel_err(Yp, Yo) < 1e-12


def test_gauss_mnmf_sources_separate_reference_channel_and_no_iterations():
    from oracle.gmnmf import GaussMNMFOracle
    from ssspy_amd.bss.mnmf import GaussMNMF
    from ssspy_amd.utils.dataset import nmf_mixture

    M, N, K, F, T = 7, 13, 4, 9, 40
    X = nmf_mixture(1500, M, F, T)
    init = _init(1501, N, F, T, K)
    # n_iter = 0: the Wiener filter of the initial state
    ref0 = GaussMNMFOracle(n_basis=K, n_sources=N, reference_id=M - 1)
    Y0r = ref0.run(X, n_iter=0, **{k: v.copy() for k, v in init.items()})
    m0 = GaussMNMF(n_basis=K, n_sources=N, reference_id=M - 1)
    Y0 = m0(X, n_iter=0, **{k: v.copy() for k, v in init.items()})
    assert rel_err(Y0, Y0r) < 1e-7
    # separate() on a fresh input with the fitted parameters
    ref = GaussMNMFOracle(n_basis=K, n_sources=N, reference_id=M - 1)
    ref.run(X, n_iter=3, **{k: v.copy() for k, v in init.items()})
    m = GaussMNMF(n_basis=K, n_sources=N, reference_id=M - 1)
    m(X, n_iter=3, **{k: v.copy() for k, v in init.items()})
    X2 = nmf_mixture(1502, M, F, T)
    assert rel_err(m.separate(X2), ref.separate(X2)) < 1e-7


def test_gauss_mnmf_sources_bounds():
    from ssspy_amd.bss.mnmf import GaussMNMF
    from ssspy_amd.utils.dataset import nmf_mixture

    X4 = nmf_mixture(1600, 4, 9, 32)
    with pytest.raises(NotImplementedError, match="16"):
        GaussMNMF(n_basis=2, n_sources=17)(X4, n_iter=1)
    X9 = nmf_mixture(1601, 9, 9, 32)
    with pytest.raises(NotImplementedError, match="8"):
        GaussMNMF(n_basis=2)(X9, n_iter=1)
