"""WPE without a device: the NumPy restatement against itself in extended precision, the descent of
its loss, a known-answer autoregression, and the constructor / limit paths of the class."""

import functools

import numpy as np
import pytest

import wpe_cases
import wpe_numpy
from ssspy_amd.dereverb import WPE
from ssspy_amd.special.flooring import add_flooring, identity, max_flooring

N_ITER = 3


@functools.lru_cache(maxsize=None)
def _pair(case):
    X = wpe_cases.make_mixture(case)
    runs = tuple(wpe_numpy.run(X, case[1], case[2], n_iter=N_ITER, dtype=dtype, statistics=True)
                 for dtype in (np.float64, np.longdouble))
    cond = max(np.linalg.cond(r) for r in runs[0]["R"].reshape(-1, *runs[0]["R"].shape[-2:]))
    return runs + (cond,)


@pytest.mark.parametrize("case", wpe_cases.CASES, ids=wpe_cases.case_id)
def test_restatement_double_agrees_with_longdouble(case):
    """The double run is the longdouble run up to rounding amplified by cond(R): three solves, each
    off by at most ~L eps cond(R) relative (Higham, Accuracy and Stability, th. 10.4), on filters and
    spectrograms of order one: 100 L eps cond(R) leaves room for the sums in front of the solves."""
    double, extended, cond = _pair(case)
    L = case[0] * case[1]
    bar = 100 * L * np.finfo(np.float64).eps * cond
    for key in ("output", "prediction_filter"):
        scale = max(1.0, float(np.abs(extended[key]).max()))
        assert np.abs(double[key] - extended[key]).max() <= bar * scale, key
    rel = np.abs(np.asarray(double["loss"]) / np.asarray(extended["loss"], dtype=np.float64) - 1)
    assert rel.max() <= bar


@pytest.mark.parametrize("case", wpe_cases.CASES, ids=wpe_cases.case_id)
def test_restatement_loss_is_non_increasing(case):
    """With flooring_fn=None each half-step minimises the objective in one block of variables, so
    from the first iteration on the loss cannot rise (entry 0 is not of that form: its lambda comes
    from y = x)."""
    X = wpe_cases.make_mixture(case)
    loss = np.asarray(wpe_numpy.run(X, case[1], case[2], n_iter=4, flooring=None)["loss"])
    loss = loss.reshape(loss.shape[0], -1)
    assert np.all(loss[2:] - loss[1:-1] <= 1e-12 * np.abs(loss[1:-1])), loss


def test_known_answer_autoregression():
    """A mixture that IS an autoregression with the taps and the delay of the model and white
    innovations: after 3 iterations at T = 4000 the output is closer to the innovations than the
    input is, and the residual energy in double is the one the longdouble run reaches."""
    M, K, D, F, T = 2, 3, 2, 2, 4000
    X, E = wpe_cases.make_autoregression(M, K, D, F, T)

    def residual(Y):
        return float(np.sum(np.abs(np.asarray(Y, dtype=np.complex128) - E) ** 2)
                     / np.sum(np.abs(E) ** 2))

    before = residual(X)
    double = residual(wpe_numpy.run(X, K, D, n_iter=3)["output"])
    extended = residual(wpe_numpy.run(X, K, D, n_iter=3, dtype=np.longdouble)["output"])
    assert double < 0.2 * before, (double, before)
    assert abs(double - extended) <= 1e-9 * extended


def test_stacked_history_has_zero_prefix():
    Xf = np.arange(1, 11, dtype=np.complex128).reshape(2, 5)
    xs = wpe_numpy.stack_history(Xf, taps=2, delay=2)
    assert xs.shape == (4, 5)
    assert np.all(xs[:2, :2] == 0) and np.all(xs[2:, :3] == 0)
    assert np.array_equal(xs[:2, 2:], Xf[:, :3]) and np.array_equal(xs[2:, 3:], Xf[:, :2])


# ---- the class, as far as it goes without a device
def test_constructor_and_repr():
    m = WPE()
    assert (m.taps, m.delay, m.record_loss, m.loss) == (10, 3, True, [])
    assert repr(m) == "WPE(taps=10, delay=3, record_loss=True)"
    m = WPE(taps=4, delay=1, flooring_fn=None, record_loss=False)
    assert m.flooring_fn is identity and m.loss is None
    assert repr(m) == "WPE(taps=4, delay=1, record_loss=False)"
    hook = lambda method: None  # noqa: E731
    assert WPE(callbacks=hook).callbacks == [hook]
    for fn in (identity, max_flooring, add_flooring, functools.partial(add_flooring, eps=1e-3)):
        WPE(flooring_fn=fn)


@pytest.mark.parametrize("kwargs", [{"delay": 0}, {"delay": -2}, {"taps": 0}, {"taps": 2.5}])
def test_bad_taps_or_delay_is_a_value_error(kwargs):
    with pytest.raises(ValueError):
        WPE(**kwargs)


def test_custom_floor_is_not_implemented():
    with pytest.raises(NotImplementedError, match="max_flooring"):
        WPE(flooring_fn=lambda x: np.maximum(x, 1e-3))


@pytest.mark.parametrize("taps, shape, match", [
    (10, (9, 3, 20), "channels"),
    (13, (5, 3, 20), "taps"),
    (65, (2, 1, 3, 20), "taps"),
])
def test_limits_raise_before_anything_is_uploaded(taps, shape, match):
    with pytest.raises(NotImplementedError, match=match):
        WPE(taps=taps)(np.zeros(shape, dtype=np.complex128))


def test_bad_rank_is_a_value_error():
    with pytest.raises(ValueError):
        WPE()(np.zeros((3, 20), dtype=np.complex128))
