"""Host-side behaviour of CACGMM and of the permutation solvers that needs no device: constructor
keywords, ``__repr__``, the draw order of the initialisation, the solvers' argument checks."""

import functools

import numpy as np
import pytest

import cacgmm_numpy as cn
from ssspy_amd.algorithm.permutation_alignment import (
    correlation_based_permutation_solver,
    score_based_permutation_solver,
)
from ssspy_amd.bss import CACGMM, CACGMMBase
from ssspy_amd.bss.cacgmm import CACGMM as CACGMMFromModule


def test_exports():
    assert CACGMM is CACGMMFromModule and issubclass(CACGMM, CACGMMBase)


@pytest.mark.parametrize("alignment", [True, "posterior_score", "amplitude_score"])
def test_score_keywords_accepted(alignment):
    m = CACGMM(permutation_alignment=alignment, global_iter=2, local_iter=3)
    assert (m.global_iter, m.local_iter) == (2, 3)


@pytest.mark.parametrize("alignment", [False, "posterior_correlation", "amplitude_correlation"])
def test_score_keywords_refused(alignment):
    with pytest.raises(AssertionError, match="Invalid keywords"):
        CACGMM(permutation_alignment=alignment, global_iter=2)
    with pytest.raises(AssertionError, match="Invalid keywords"):
        CACGMM(permutation_alignment=True, n_iter=3)


def test_repr_and_defaults():
    m = CACGMM(n_sources=3, record_loss=False, reference_id=1)
    assert repr(m) == ("CACGMM(n_sources=3, record_loss=False, normalization=True, "
                       "permutation_alignment=True, reference_id=1)")
    assert repr(CACGMM()) == ("CACGMM(record_loss=True, normalization=True, "
                              "permutation_alignment=True, reference_id=0)")
    assert repr(CACGMMBase(n_sources=2)) == "CACGMM(n_sources=2, record_loss=True)"
    assert m.loss is None and CACGMM().loss == []
    assert CACGMM(flooring_fn=None).flooring_fn(-1.0) == -1.0
    assert CACGMM(callbacks=print).callbacks == [print]


@pytest.mark.parametrize("batch", [1, 3])
def test_initialisation_draw_order(batch):
    """alpha (N, F) first, then the diagonals (N, F, M), mixture after mixture, from one generator."""
    N, F, M = 3, 5, 4
    m = CACGMM(n_sources=N, rng=np.random.default_rng(5))
    m._X = np.empty((batch, M, F, 7))  # only the number of mixtures is read
    m._batched = batch > 1
    m.n_sources, m.n_channels, m.n_bins = N, M, F
    m._init_parameters(rng=m.rng)
    rng = np.random.default_rng(5)
    expect = [cn.init_parameters(rng, N, F, M) for _ in range(batch)]
    mixing, covariance = np.asarray(m.mixing), np.asarray(m.covariance)
    if batch == 1:
        mixing, covariance = mixing[None], covariance[None]
    for b in range(batch):
        assert np.array_equal(mixing[b], expect[b][0])
        assert np.array_equal(covariance[b], expect[b][1])
    assert m.posterior is None
    assert covariance.shape == (batch, N, F, M, M) and covariance.dtype == np.complex128


def test_solver_argument_checks():
    seq = np.random.default_rng(0).random((4, 3, 10))
    for solver in (score_based_permutation_solver, correlation_based_permutation_solver):
        with pytest.raises(AssertionError, match="Dimension"):
            solver(seq[0])
        with pytest.raises(ValueError, match="1th argument"):
            solver(seq, np.zeros((4, 2)))
        with pytest.raises(ValueError, match="2th argument"):
            solver(seq, np.zeros((4, 3)), np.zeros((3, 3, 1)))
    with pytest.raises(AssertionError, match="multi_centroids"):
        score_based_permutation_solver(seq, multi_centroids=True)


def test_solver_return_forms_and_overwrite():
    rng = np.random.default_rng(3)
    seq = rng.random((6, 3, 20))
    extra = rng.random((6, 3, 2))
    for solver in (score_based_permutation_solver, correlation_based_permutation_solver):
        kept, kept_extra = seq.copy(), extra.copy()
        out = solver(kept, overwrite=False)
        assert isinstance(out, np.ndarray) and np.array_equal(kept, seq)
        out, one = solver(kept, kept_extra, overwrite=False)
        assert np.array_equal(kept_extra, extra) and one.shape == extra.shape
        out, many = solver(kept, kept_extra, kept_extra, overwrite=False)
        assert isinstance(many, tuple) and len(many) == 2
        # in place: the further arguments follow the sequence
        index = np.tile(np.arange(3), (6, 1))
        work = extra.copy()
        out, (index, work2) = solver(seq.copy(), index, work, overwrite=True)
        assert work2 is work
        assert np.array_equal(work, np.take_along_axis(extra, index[:, :, None], axis=1))


@pytest.mark.parametrize("N", [2, 3, 4])
def test_solvers_agree_with_the_restatement(N):
    rng = np.random.default_rng(10 + N)
    F, T = 14, 48
    env = rng.gamma(1.0, 1.0, (N, T))
    seq = np.stack([env[rng.permutation(N)] * rng.gamma(2.0, 1.0, (N, T)) for _ in range(F)])
    index = np.tile(np.arange(N), (F, 1))
    fn = functools.partial(cn.max_flooring, eps=1e-10)
    _, (want,) = cn.score_solver(seq, index, global_iter=2, local_iter=2, flooring_fn=fn)
    _, got = score_based_permutation_solver(seq, index, global_iter=2, local_iter=2, flooring_fn=fn,
                                            overwrite=False)
    assert np.array_equal(got, want)
    Y = seq * np.exp(1j * rng.standard_normal(seq.shape))
    _, (want,) = cn.correlation_solver(Y, index, flooring_fn=fn)
    _, got = correlation_based_permutation_solver(Y, index, flooring_fn=fn, overwrite=False)
    assert np.array_equal(got, want)
