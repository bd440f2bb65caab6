"""CPU-side checks of the time-domain ICA classes: constructors, repr strings, exports, the route
decision, the size limits, the "no CPU fallback" error and the named nonlinearities.  No device."""

import functools

import numpy as np
import pytest
import torch

import ica_cases
from ssspy_amd import _routes, bss
from ssspy_amd.bss import ica


def test_constructor_defaults_and_errors():
    m = ica.GradICA(contrast_fn=np.abs, score_fn=np.sign)
    assert (m.step_size, m.is_holonomic, m.record_loss) == (1e-1, False, True)
    assert m.loss == [] and m.input is None and not hasattr(m, "demix_filter")
    assert ica.NaturalGradLaplaceICA().is_holonomic is False
    assert ica.GradLaplaceICA(record_loss=False).loss is None
    for cls in (ica.GradICABase, ica.GradICA, ica.NaturalGradICA):
        with pytest.raises(ValueError, match=r"^Specify contrast function\.$"):
            cls(score_fn=np.sign)
        with pytest.raises(ValueError, match=r"^Specify score function\.$"):
            cls(contrast_fn=np.abs)
    for cls in (ica.FastICABase, ica.FastICA):
        with pytest.raises(ValueError, match=r"^Specify contrast function\.$"):
            cls(score_fn=np.tanh, d_score_fn=np.cos)
        with pytest.raises(ValueError, match=r"^Specify score function\.$"):
            cls(contrast_fn=np.abs, d_score_fn=np.cos)
        with pytest.raises(ValueError, match=r"^Specify derivative of score function\.$"):
            cls(contrast_fn=np.abs, score_fn=np.tanh)
    hook = lambda method: None  # noqa: E731
    assert ica.GradLaplaceICA(callbacks=hook).callbacks == [hook]
    with pytest.raises(NotImplementedError):
        ica.GradICABase(contrast_fn=np.abs, score_fn=np.sign).update_once()
    with pytest.raises(NotImplementedError):
        ica.FastICABase(contrast_fn=np.abs, score_fn=np.tanh, d_score_fn=np.cos).update_once()


def test_repr_strings():
    fns = dict(contrast_fn=np.abs, score_fn=np.sign)
    assert repr(ica.GradICABase(**fns)) == "GradICA(step_size=0.1, record_loss=True)"
    assert repr(ica.GradICA(step_size=0.5, is_holonomic=True, **fns)) == \
        "GradICA(step_size=0.5, is_holonomic=True, record_loss=True)"
    assert repr(ica.NaturalGradICA(record_loss=False, **fns)) == \
        "NaturalGradICA(step_size=0.1, is_holonomic=False, record_loss=False)"
    assert repr(ica.GradLaplaceICA()) == \
        "GradLaplaceICA(step_size=0.1, is_holonomic=False, record_loss=True)"
    assert repr(ica.NaturalGradLaplaceICA(step_size=0.2)) == \
        "NaturalGradLaplaceICA(step_size=0.2, is_holonomic=False, record_loss=True)"
    fast = dict(contrast_fn=np.abs, score_fn=np.tanh, d_score_fn=np.cos)
    assert repr(ica.FastICABase(**fast)) == "FastICA(record_loss=True)"
    assert repr(ica.FastICA(record_loss=False, **fast)) == "FastICA(record_loss=False)"


def test_exports():
    assert bss.ica is ica and "ica" in bss.__all__
    names = ["GradICA", "NaturalGradICA", "FastICA", "GradLaplaceICA", "NaturalGradLaplaceICA"]
    assert ica.__all__ == names
    for name in names:
        assert name in bss.__all__ and getattr(bss, name) is getattr(ica, name)
    assert issubclass(ica.GradLaplaceICA, ica.GradICA)
    assert issubclass(ica.NaturalGradLaplaceICA, ica.NaturalGradICA)
    assert issubclass(ica.FastICA, ica.FastICABase) and issubclass(ica.GradICA, ica.GradICABase)
    assert issubclass(ica.GradICABase, bss.IterativeMethodBase)


def test_route_decision():
    assert ica.route(ica.GradLaplaceICA()) == (ica.DEVICE, "laplace")
    assert ica.route(ica.NaturalGradLaplaceICA()) == (ica.DEVICE, "laplace")
    for name, (g, s, d) in ica.NAMED.items():
        assert ica.route(ica.GradICA(contrast_fn=g, score_fn=s)) == (ica.DEVICE, name)
        assert ica.route(ica.NaturalGradICA(contrast_fn=g, score_fn=s)) == (ica.DEVICE, name)
        if d is not None:
            assert ica.route(ica.FastICA(contrast_fn=g, score_fn=s, d_score_fn=d)) == \
                (ica.DEVICE, name)
    compat = (ica.COMPATIBILITY, None)
    g, s, d = ica.NAMED["logistic"]
    # a closure around a named function, a partial of one, a mixed pair, a same-named stranger
    assert ica.route(ica.GradICA(contrast_fn=lambda y: g(y), score_fn=s)) == compat
    assert ica.route(ica.GradICA(contrast_fn=g, score_fn=functools.partial(s))) == compat
    assert ica.route(ica.GradICA(contrast_fn=g, score_fn=ica.logcosh_score)) == compat
    assert ica.route(ica.GradICA(contrast_fn=ica_cases.logistic_contrast,
                                 score_fn=ica_cases.logistic_score)) == compat
    assert ica.route(ica.FastICA(contrast_fn=g, score_fn=s, d_score_fn=lambda y: d(y))) == compat
    # laplace has no derivative of the score: never the device route of FastICA
    lg, ls, _ = ica.NAMED["laplace"]
    assert ica.route(ica.FastICA(contrast_fn=lg, score_fn=ls, d_score_fn=np.zeros_like)) == compat
    # the route entry forces the compatibility route (what the tests compare the two with)
    assert _routes.get("ica_named") is True
    with _routes.override(ica_named=False):
        assert ica.route(ica.GradLaplaceICA()) == compat
    assert ica.route(ica.GradLaplaceICA()) == (ica.DEVICE, "laplace")


@pytest.mark.parametrize("n_sources", [1, 17])
def test_size_limits_name_the_limit(n_sources):
    x = np.zeros((n_sources, 8))
    fast = ica.FastICA(*ica.NAMED["logcosh"])
    for m in (ica.GradLaplaceICA(), ica.NaturalGradLaplaceICA(), fast):
        with pytest.raises(NotImplementedError, match="2 to 16 sources, got {}".format(n_sources)):
            m(x, n_iter=1)
    with pytest.raises(NotImplementedError, match="2 to 16 sources"):
        ica.GradLaplaceICA()(np.zeros((3, n_sources, 8)), n_iter=1)


def test_bad_inputs():
    with pytest.raises(ValueError, match="n_samples must be at least 1"):
        ica.GradLaplaceICA()(np.zeros((2, 0)), n_iter=1)
    with pytest.raises(ValueError, match="n_channels, n_samples"):
        ica.GradLaplaceICA()(np.zeros((2, 2, 2, 2)), n_iter=1)


def test_product_path_fails_loudly_without_device():
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    for m in (ica.GradLaplaceICA(), ica.FastICA(*ica.NAMED["logistic"])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(np.zeros((2, 16)), n_iter=1)


GRID = np.array([0.0, 1e-300, -1e-300, 1e-8, -1e-8, 0.5, -0.5, 1.0, -1.0, 3.0, -3.0, 20.0, -20.0,
                 40.0, -40.0, 700.0, -700.0] + list(np.linspace(-6, 6, 97)))


def test_named_functions_agree_with_their_formulas():
    """On the grid NumPy's exp and cosh neither overflow nor underflow, so the overflow-safe forms
    equal the textbook ones: to 1e-13 relative, or 1e-15 absolute where the textbook form cancels
    (s (1 - s) for large x, log(cosh(x)) for small x)."""
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        for name in ("logistic", "logcosh"):
            for fn, formula in zip(ica.NAMED[name], ica_cases.FORMULAS[name]):
                np.testing.assert_allclose(fn(GRID), formula(GRID), rtol=1e-13, atol=1e-15,
                                           err_msg=fn.__name__)
    g, s, d = ica.NAMED["laplace"]
    assert d is None
    assert np.array_equal(g(GRID), np.abs(GRID)) and np.array_equal(s(GRID), np.sign(GRID))
    assert s(np.zeros(3)).tolist() == [0.0, 0.0, 0.0]


def test_named_functions_stay_finite_where_the_formulas_overflow():
    x = np.array([-1e4, -800.0, 800.0, 1e4, 1e300, -1e300])
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        for name in ("logistic", "logcosh"):
            for fn in ica.NAMED[name]:
                assert np.isfinite(fn(x)).all(), fn.__name__
    np.testing.assert_allclose(ica.logistic_contrast(x), np.maximum(x, 0), rtol=1e-15)
    np.testing.assert_allclose(ica.logcosh_contrast(x), np.abs(x) - np.log(2), rtol=1e-15)
    # shapes: (n_sources, n_samples) arrays and single rows alike
    y = np.linspace(-2, 2, 12).reshape(3, 4)
    for fns in ica.NAMED.values():
        for fn in fns:
            if fn is not None:
                assert fn(y).shape == (3, 4) and fn(y[0]).shape == (4,)
