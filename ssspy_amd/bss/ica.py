"""Time-domain independent component analysis (ICA) on MI355X.

Drop-in separator classes for the reference's ``ssspy.bss.ica`` (ssspy/bss/ica.py): ``GradICABase``,
``FastICABase``, ``GradICA``, ``NaturalGradICA``, ``FastICA``, ``GradLaplaceICA`` and
``NaturalGradLaplaceICA``, on real fp64 waveforms ``(n_channels, n_samples)`` or batches
``(n_mixtures, n_channels, n_samples)`` of independent mixtures (then ``loss`` holds one array of
``n_mixtures`` values per state).  2 to 16 sources, any ``n_samples >= 1``.

An iteration is two launches (csrc/ica.hip): the statistics pass reads the mixture once, forms
``y = W x`` and the nonlinearity in registers and leaves one partial record per 2048 samples; the
step kernel adds the records in order, divides by ``n_samples`` and updates ``W``.  The loss of a
state is a by-product of the statistics pass that starts from it, so without callbacks ``__call__``
enqueues all iterations with no host synchronisation and reads the loss terms once at the end.

Two routes, decided once per call (``route``):

* the device route for a named nonlinearity -- the two Laplace classes always, the generic classes
  when ``contrast_fn``, ``score_fn`` (and ``d_score_fn`` for FastICA) are passed AS THEMSELVES from
  the module-level functions below (``NAMED``: laplace, logistic, logcosh);
* the compatibility route for any other callable (a closure, a ``functools.partial``, a function of
  the same name from elsewhere): once per iteration ``Y`` comes to the host, the closure's ``Phi``
  (FastICA: ``d_score`` too) goes back up; the reductions and the filter step stay on the device.
  ``contrast_fn`` runs on the host only when the loss is recorded.

The named functions are ordinary NumPy callables in overflow-safe forms: equal to
``log(1 + exp(x))``, ``1 / (1 + exp(-x))``, ``log(cosh(x))`` wherever NumPy's ``exp`` and ``cosh``
neither overflow nor underflow, finite where they do.  The kernels use the same forms.
"""

from typing import Callable, List, Optional, Union

import numpy as np
import torch

from .. import _device as dv
from .. import _lib, _ops, _routes
from .base import IterativeMethodBase

__all__ = ["GradICA", "NaturalGradICA", "FastICA", "GradLaplaceICA", "NaturalGradLaplaceICA"]

MIN_SOURCES, MAX_SOURCES = _lib.ICA_MIN_SOURCES, _lib.RT_MAX_SOURCES
DEVICE, COMPATIBILITY = "device", "compatibility"


# ---- the named nonlinearities -------------------------------------------------------------------
def laplace_contrast(x):
    """G(x) = |x|."""
    return np.abs(x)


def laplace_score(x):
    """phi(x) = sign(x), sign(0) = 0."""
    return np.sign(x)


def logistic_contrast(x):
    """G(x) = log(1 + exp(x)) as max(x, 0) + log1p(exp(-|x|))."""
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def logistic_score(x):
    """phi(x) = 1 / (1 + exp(-x)), without the overflow of exp(-x)."""
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    d = 1.0 / (1.0 + e)
    return np.where(x >= 0, d, e * d)


def logistic_d_score(x):
    """phi'(x) = s (1 - s), s = phi(x), as e / (1 + e)^2 with e = exp(-|x|)."""
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    d = 1.0 / (1.0 + e)
    return e * d * d


def logcosh_contrast(x):
    """G(x) = log(cosh(x)) as |x| + log1p(exp(-2 |x|)) - log 2."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    return a + np.log1p(np.exp(-2.0 * a)) - np.log(2.0)


def logcosh_score(x):
    """phi(x) = tanh(x)."""
    return np.tanh(x)


def logcosh_d_score(x):
    """phi'(x) = 1 - tanh(x)^2."""
    th = np.tanh(x)
    return 1.0 - th * th


# name -> (contrast, score, derivative of the score or None)
NAMED = {
    "laplace": (laplace_contrast, laplace_score, None),
    "logistic": (logistic_contrast, logistic_score, logistic_d_score),
    "logcosh": (logcosh_contrast, logcosh_score, logcosh_d_score),
}
_KIND = {"laplace": _lib.ICA_LAPLACE, "logistic": _lib.ICA_LOGISTIC, "logcosh": _lib.ICA_LOGCOSH}


def named_nonlinearity(contrast_fn, score_fn, d_score_fn=None, fast=False):
    """The name in ``NAMED`` whose functions were passed as themselves, or None.  The gradient classes
    need the contrast and the score, FastICA (``fast``) the derivative of the score as well."""
    for name, (contrast, score, d_score) in NAMED.items():
        if contrast_fn is contrast and score_fn is score:
            if not fast:
                return name
            if d_score is not None and d_score_fn is d_score:
                return name
    return None


def route(method):
    """``(DEVICE, name)`` when the kernels apply the nonlinearity of ``method``, else
    ``(COMPATIBILITY, None)``."""
    fast = isinstance(method, FastICABase)
    name = named_nonlinearity(getattr(method, "contrast_fn", None), getattr(method, "score_fn", None),
                              getattr(method, "d_score_fn", None), fast=fast)
    if name is None or not _routes.get("ica_named"):
        return COMPATIBILITY, None
    return DEVICE, name


def _check_sources(cls_name, n_sources):
    if not MIN_SOURCES <= n_sources <= MAX_SOURCES:
        raise NotImplementedError("{} takes {} to {} sources, got {}.".format(
            cls_name, MIN_SOURCES, MAX_SOURCES, n_sources))


def _to_batch(input, what):
    """(device tensor (B, N, T) f64, batched) of a NumPy array or a device tensor."""
    if input.ndim not in (2, 3):
        raise ValueError(
            "{} must be (n_channels, n_samples) or (n_mixtures, n_channels, n_samples), "
            "got shape {}".format(what, tuple(input.shape)))
    batched = input.ndim == 3
    if isinstance(input, torch.Tensor):
        if not input.is_cuda or input.dtype != torch.float64:
            raise ValueError("a tensor {} must be float64 on the HIP device".format(what))
        X3 = input if batched else input[None]
        return X3.contiguous(), batched
    arr = np.asarray(input)
    if np.iscomplexobj(arr):
        raise ValueError("Real tensor is expected, but given complex tensor.")
    return dv.to_device(arr if batched else arr[None], dtype=np.float64), batched


class _ICABase(IterativeMethodBase):
    """State and drivers shared by the gradient classes and FastICA: the mixture, the filters and
    the estimate live in HBM as (B, N, T) / (B, N, N); the attributes are host views made on read."""

    _stock_methods = ("update_once", "compute_loss", "separate")
    _algorithm = _lib.ICA_FOLD_ONLY
    _right = _lib.ICA_RIGHT_Y
    _has_logdet = True
    _batched = False

    # -- input --------------------------------------------------------------------------------
    def _bind_input(self, input) -> None:
        shape = tuple(input.shape)
        if len(shape) in (2, 3):
            _check_sources(type(self).__name__, shape[-2])
            if shape[-1] < 1:
                raise ValueError("n_samples must be at least 1.")
        self._X, self._batched = _to_batch(input, "input")
        d = self.__dict__
        if isinstance(input, torch.Tensor):
            d["_input_value"], d["_input_dtype"] = input, None
        else:  # the private copy of the reference IS the HBM buffer; a host view is made on read
            d["_input_value"], d["_input_dtype"] = None, np.asarray(input).dtype
        d["_Z"] = d["_Z_host"] = None
        d["_ws"] = None

    @property
    def input(self):
        """The mixture(s) as given (ref: ssspy/bss/ica.py:79, a private copy)."""
        d = self.__dict__
        value = d.get("_input_value")
        if value is None and d.get("_input_dtype") is not None:
            host = dv.to_host(self._X)
            host = host if self._batched else host[0]
            value = d["_input_value"] = host.astype(d["_input_dtype"], copy=False)
        return value

    @input.setter
    def input(self, value):
        self.__dict__["_input_value"] = value
        self.__dict__["_input_dtype"] = None

    def _lead(self):
        return (self._X.shape[0],) if self._batched else ()

    def _source(self):
        """What the iterations read: the mixture (FastICA: the whitened mixture)."""
        return self._X

    # -- filters and estimate --------------------------------------------------------------------
    @property
    def demix_filter(self):
        d = self.__dict__
        if not d.get("_W_set"):
            raise AttributeError("'{}' object has no attribute 'demix_filter'".format(
                type(self).__name__))
        if d.get("_W_host") is None and d.get("_W_dev") is not None:
            self._check_device_errors()
            host = dv.to_host(d["_W_dev"])
            d["_W_host"] = np.array(host if self._batched else host[0])
        return d.get("_W_host")

    @demix_filter.setter
    def demix_filter(self, value):
        d = self.__dict__
        if isinstance(value, torch.Tensor):
            value = value.detach().cpu().numpy()
        d["_W_set"], d["_W_host"], d["_W_dev"] = True, value, None
        d["_Y_dev"] = d["_Y_host"] = None

    @property
    def output(self):
        d = self.__dict__
        if d.get("_Y_host") is None:
            if d.get("_Y_dev") is None:
                if d.get("_W_dev") is None:
                    raise AttributeError("'{}' object has no attribute 'output'".format(
                        type(self).__name__))
                d["_Y_dev"] = _ops.ica_separate(self._source(), d["_W_dev"])
            self._check_device_errors()
            host = dv.to_host(d["_Y_dev"])
            d["_Y_host"] = host if self._batched else host[0]
        return d["_Y_host"]

    @output.setter
    def output(self, value):
        self.__dict__["_Y_host"] = value

    def _filters_stepped(self) -> None:
        d = self.__dict__
        d["_W_host"] = d["_Y_dev"] = d["_Y_host"] = None

    def _reset_filters(self) -> None:
        """ref: ssspy/bss/ica.py:117-127: the identity, or a copy of what is there."""
        N = self.n_sources
        lead = self._lead()
        if not self.__dict__.get("_W_set"):
            W = np.tile(np.eye(N, dtype=np.float64), lead + (1, 1))
        else:
            W = self.demix_filter
            if W is None:
                raise ValueError("demix_filter=None cannot be given at reset.")
            # (a copy: the filters given by keyword are not overwritten)
            W = np.array(W, dtype=np.float64, copy=True)
        if W.shape != lead + (N, N):
            raise ValueError("demix_filter must have shape {}, got {}.".format(lead + (N, N), W.shape))
        d = self.__dict__
        d["_W_set"], d["_W_host"] = True, W
        d["_W_dev"] = dv.to_device(W if self._batched else W[None], dtype=np.float64,
                                   dev=self._X.device)
        d["_Y_dev"] = d["_Y_host"] = None

    def _set_shape(self) -> None:
        B, N, T = self._X.shape
        self.n_sources, self.n_channels = N, N
        self.n_samples = T
        self._route, name = route(self)
        self._kind = _KIND[name] if name else _lib.ICA_GIVEN

    # -- device plumbing -------------------------------------------------------------------------
    def _workspace(self):
        if self.__dict__.get("_ws") is None:
            B, N, T = self._X.shape
            self._ws = _ops.ica_workspace(B, N, T, self._X.device)
        return self._ws

    def _info_tensor(self):
        if self.__dict__.get("_info") is None:
            self._info = dv.zeros((1,), dv.i32, self._X.device)
        return self._info

    def _check_device_errors(self) -> None:
        """A zero pivot met by the GradICA step: ``numpy.linalg.inv`` raises there."""
        _ops.check_workspace_canaries()
        info = self.__dict__.get("_info")
        if info is not None:
            singular = int(info.item())  # synchronises
            if singular:
                info.zero_()
                raise np.linalg.LinAlgError("Singular matrix")

    # -- the passes ------------------------------------------------------------------------------
    def _host_nonlinearity(self, W):
        """The compatibility route: Y comes down, (Phi, d_score or None) go up."""
        raise NotImplementedError

    def _stats(self, W) -> None:
        """Records of the state W in the workspace."""
        if self._route == DEVICE:
            _ops.ica_stats(self._source(), W, self._workspace(), self._kind, self._right)
        else:
            phi, dphi = self._host_nonlinearity(W)
            _ops.ica_stats(self._source(), W, self._workspace(), _lib.ICA_GIVEN, self._right,
                           phi=phi, dphi=dphi)

    def _step(self, W, loss_data=None, logdet=None, algorithm=None) -> None:
        _ops.ica_step(self._workspace(), W, self.n_samples,
                      self._algorithm if algorithm is None else algorithm,
                      getattr(self, "is_holonomic", False), getattr(self, "step_size", 0.0),
                      loss_data=loss_data, logdet=logdet if self._has_logdet else None,
                      info=self._info_tensor())

    def _update_once(self) -> None:
        W = self.__dict__["_W_dev"]
        self._stats(W)
        self._step(W)
        self._filters_stepped()

    def _loss_entry(self, values):
        return values.copy() if self._batched else values[0].item()

    def _compute_loss(self):
        W = self.__dict__["_W_dev"]
        B = self._X.shape[0]
        if self._route == DEVICE:
            terms = dv.zeros((2, B), dv.f64, self._X.device)
            self._stats(W)
            self._step(W, terms[0], terms[1], algorithm=_lib.ICA_FOLD_ONLY)
            self._check_device_errors()
            host = dv.to_host(terms)
            return self._loss_entry(host[0] - host[1] if self._has_logdet else host[0].copy())
        self._check_device_errors()
        Y = dv.to_host(_ops.ica_separate(self._source(), W))
        values = np.array([np.sum(np.mean(self.contrast_fn(Yb), axis=-1)) for Yb in Y])
        if self._has_logdet:
            values = values - self.compute_logdet(dv.to_host(W))
        return self._loss_entry(values)

    def _iterate_resident(self, n_iter: int, initial_call: bool) -> bool:
        """All ``n_iter`` iterations enqueued with no host synchronisation when nothing can look in
        between: the device route, no callbacks, the methods this module defines.  The loss terms of
        state k are left by the step of iteration k + 1 (one closing pass for the last state) and
        stay in HBM until the end.  False: the reference's loop."""
        cls = type(self)
        stock = all(getattr(getattr(cls, name, None), "__module__", __name__) == __name__
                    for name in self._stock_methods)
        if self.callbacks or n_iter <= 0 or not stock or self._route != DEVICE:
            return False
        W = self.__dict__["_W_dev"]
        if not self.record_loss:
            for _ in range(n_iter):
                self._stats(W)
                self._step(W)
            self._filters_stepped()
            return True
        B, dev = self._X.shape[0], self._X.device
        terms = dv.zeros((2, n_iter + 1, B), dv.f64, dev)
        for k in range(n_iter):
            self._stats(W)
            self._step(W, terms[0, k], terms[1, k])
        self._stats(W)
        self._step(W, terms[0, n_iter], terms[1, n_iter], algorithm=_lib.ICA_FOLD_ONLY)
        self._filters_stepped()
        self._check_device_errors()
        host = dv.to_host(terms)
        values = host[0] - host[1] if self._has_logdet else host[0]
        self.loss.extend(self._loss_entry(v) for v in (values if initial_call else values[1:]))
        return True

    def _run(self, input, n_iter, initial_call, kwargs):
        self._bind_input(input)
        self._reset(**kwargs)
        if not self._iterate_resident(int(n_iter), initial_call):
            IterativeMethodBase.__call__(self, n_iter=n_iter, initial_call=initial_call)
        self._check_device_errors()
        return self.output

    def compute_logdet(self, demix_filter: np.ndarray) -> np.ndarray:
        """log|det W| (ref: ssspy/bss/ica.py:180-193)."""
        _, logdet = np.linalg.slogdet(demix_filter)
        return logdet


class GradICABase(_ICABase):
    """ICA by gradient descent (ref: ssspy/bss/ica.py:11-193)."""

    def __init__(
        self,
        step_size: float = 1e-1,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        score_fn: Callable[[np.ndarray], np.ndarray] = None,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        record_loss: bool = True,
    ) -> None:
        super().__init__(callbacks=callbacks, record_loss=record_loss)
        self.step_size = step_size
        if contrast_fn is None:
            raise ValueError("Specify contrast function.")
        self.contrast_fn = contrast_fn
        if score_fn is None:
            raise ValueError("Specify score function.")
        self.score_fn = score_fn
        self.input = None

    def __call__(
        self, input: np.ndarray, n_iter: int = 100, initial_call: bool = True, **kwargs
    ) -> np.ndarray:
        """Separate a time-domain multichannel signal (ref: ssspy/bss/ica.py:59-87)."""
        return self._run(input, n_iter, initial_call, kwargs)

    def __repr__(self) -> str:
        s = "GradICA("
        s += "step_size={step_size}"
        s += ", record_loss={record_loss}"
        s += ")"
        return s.format(**self.__dict__)

    def _repr_with_holonomic(self, name) -> str:
        s = name + "("
        s += "step_size={step_size}"
        s += ", is_holonomic={is_holonomic}"
        s += ", record_loss={record_loss}"
        s += ")"
        return s.format(**self.__dict__)

    def _reset(self, **kwargs) -> None:
        """ref: ssspy/bss/ica.py:97-127."""
        assert self.__dict__.get("_X") is not None, "Specify data!"
        for key, value in kwargs.items():
            setattr(self, key, value)
        self._set_shape()
        self._reset_filters()

    def update_once(self) -> None:
        raise NotImplementedError("Implement 'update_once' method.")

    def separate(self, input: np.ndarray, demix_filter: np.ndarray) -> np.ndarray:
        """y_t = W x_t (ref: ssspy/bss/ica.py:133-154); NumPy in, NumPy out."""
        X, batched = _to_batch(input, "input")
        W, _ = _to_batch(np.asarray(demix_filter, dtype=np.float64), "demix_filter")
        Y = dv.to_host(_ops.ica_separate(X, W))
        return Y if batched else Y[0]

    def compute_loss(self) -> float:
        """mean_t sum_n G(y_tn) - log|det W| (ref: ssspy/bss/ica.py:156-178)."""
        return self._compute_loss()

    def _host_nonlinearity(self, W):
        self._check_device_errors()
        Y = dv.to_host(_ops.ica_separate(self._X, W))
        Phi = np.stack([np.asarray(self.score_fn(Yb), dtype=np.float64) for Yb in Y])
        if Phi.shape != Y.shape:
            raise ValueError("score_fn must map (n_sources, n_samples) to the same shape.")
        return dv.to_device(Phi, dtype=np.float64, dev=W.device), None


class FastICABase(_ICABase):
    """FastICA (ref: ssspy/bss/ica.py:196-403)."""

    _right = _lib.ICA_RIGHT_X
    _has_logdet = False

    def __init__(
        self,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        score_fn: Callable[[np.ndarray], np.ndarray] = None,
        d_score_fn: Callable[[np.ndarray], np.ndarray] = None,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        record_loss: bool = True,
    ) -> None:
        super().__init__(callbacks=callbacks, record_loss=record_loss)
        if contrast_fn is None:
            raise ValueError("Specify contrast function.")
        self.contrast_fn = contrast_fn
        if score_fn is None:
            raise ValueError("Specify score function.")
        self.score_fn = score_fn
        if d_score_fn is None:
            raise ValueError("Specify derivative of score function.")
        self.d_score_fn = d_score_fn
        self.input = None

    def __call__(
        self, input: np.ndarray, n_iter: int = 100, initial_call: bool = True, **kwargs
    ) -> np.ndarray:
        """Separate a time-domain multichannel signal (ref: ssspy/bss/ica.py:248-278)."""
        return self._run(input, n_iter, initial_call, kwargs)

    def __repr__(self) -> str:
        s = "FastICA("
        s += "record_loss={record_loss}"
        s += ")"
        return s.format(**self.__dict__)

    def _reset(self, **kwargs) -> None:
        """ref: ssspy/bss/ica.py:287-321."""
        assert self.__dict__.get("_X") is not None, "Specify data!"
        for key, value in kwargs.items():
            setattr(self, key, value)
        self._set_shape()
        self.__dict__["_Z"] = _whiten_device(self._X, self._workspace())
        self.__dict__["_Z_host"] = None
        self._reset_filters()

    def _source(self):
        return self.__dict__["_Z"]

    @property
    def whitened_input(self):
        d = self.__dict__
        if d.get("_Z_host") is None:
            if d.get("_Z") is None:
                raise AttributeError("'{}' object has no attribute 'whitened_input'".format(
                    type(self).__name__))
            host = dv.to_host(d["_Z"])
            d["_Z_host"] = host if self._batched else host[0]
        return d["_Z_host"]

    def update_once(self) -> None:
        raise NotImplementedError("Implement 'update_once' method.")

    def separate(
        self, input: np.ndarray, demix_filter: np.ndarray, use_whitening: bool = True
    ) -> np.ndarray:
        """y_t = W z_t with z the whitened input when ``use_whitening``, else y_t = W x_t
        (ref: ssspy/bss/ica.py:327-381); NumPy in, NumPy out."""
        X, batched = _to_batch(input, "input")
        W, _ = _to_batch(np.asarray(demix_filter, dtype=np.float64), "demix_filter")
        if use_whitening:
            _check_sources(type(self).__name__, X.shape[1])
            B, N, T = X.shape
            X = _whiten_device(X, _ops.ica_workspace(B, N, T, X.device))
        Y = dv.to_host(_ops.ica_separate(X, W))
        return Y if batched else Y[0]

    def compute_loss(self) -> float:
        """mean_t sum_n G(y_tn) (ref: ssspy/bss/ica.py:383-403)."""
        return self._compute_loss()

    def _host_nonlinearity(self, W):
        # the closures see one row at a time, as in the reference (ssspy/bss/ica.py:825-827)
        Y = dv.to_host(_ops.ica_separate(self._source(), W))
        Phi, dPhi = np.empty_like(Y), np.empty_like(Y)
        for b in range(Y.shape[0]):
            for n in range(Y.shape[1]):
                Phi[b, n] = self.score_fn(Y[b, n])
                dPhi[b, n] = self.d_score_fn(Y[b, n])
        return (dv.to_device(Phi, dtype=np.float64, dev=W.device),
                dv.to_device(dPhi, dtype=np.float64, dev=W.device))


def _whiten_device(X, ws):
    """z = Lambda^-1/2 Gamma^T x with mean_t x x^T = Gamma Lambda Gamma^T, per mixture
    (ref: ssspy/transform/whiten.py).  The Gram matrix comes from the statistics pass with the
    identity nonlinearity; its N x N eigen-decomposition is numpy.linalg.eigh on the host, so the
    signs of the eigenvectors follow LAPACK as the reference's do; P x runs on the device."""
    B, N, T = X.shape
    eye = dv.zeros((B, N, N), dv.f64, X.device)
    eye.diagonal(dim1=-2, dim2=-1).fill_(1.0)
    means = dv.empty((B, N * N + 2 * N), dv.f64, X.device)
    _ops.ica_stats(X, eye, ws, _lib.ICA_IDENTITY, _lib.ICA_RIGHT_X)
    _ops.ica_step(ws, eye, T, _lib.ICA_FOLD_ONLY, means=means)
    covariance = dv.to_host(means)[:, :N * N].reshape(B, N, N)
    # (the record holds both triangles from the same products in the same order: symmetric to the bit)
    lam, V = np.linalg.eigh(covariance)
    P = (1 / np.sqrt(lam))[:, :, np.newaxis] * V.transpose(0, 2, 1)
    return _ops.ica_separate(X, dv.to_device(P, dtype=np.float64, dev=X.device))


class GradICA(GradICABase):
    """ICA by gradient descent, W <- W - eta D W^-T (ref: ssspy/bss/ica.py:406-554).  A singular W
    raises ``numpy.linalg.LinAlgError``, as ``numpy.linalg.inv`` does."""

    _algorithm = _lib.ICA_GRAD

    def __init__(
        self,
        step_size: float = 1e-1,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        score_fn: Callable[[np.ndarray], np.ndarray] = None,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        is_holonomic: bool = False,
        record_loss: bool = True,
    ) -> None:
        super().__init__(
            step_size=step_size,
            contrast_fn=contrast_fn,
            score_fn=score_fn,
            callbacks=callbacks,
            record_loss=record_loss,
        )
        self.is_holonomic = is_holonomic

    def __repr__(self) -> str:
        return self._repr_with_holonomic("GradICA")

    def update_once(self) -> None:
        """ref: ssspy/bss/ica.py:506-554."""
        self._update_once()


class NaturalGradICA(GradICABase):
    """ICA by natural gradient descent, W <- W - eta D W (ref: ssspy/bss/ica.py:557-707)."""

    _algorithm = _lib.ICA_NATURAL_GRAD

    def __init__(
        self,
        step_size: float = 1e-1,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        score_fn: Callable[[np.ndarray], np.ndarray] = None,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        is_holonomic: bool = False,
        record_loss: bool = True,
    ) -> None:
        super().__init__(
            step_size=step_size,
            contrast_fn=contrast_fn,
            score_fn=score_fn,
            callbacks=callbacks,
            record_loss=record_loss,
        )
        self.is_holonomic = is_holonomic

    def __repr__(self) -> str:
        return self._repr_with_holonomic("NaturalGradICA")

    def update_once(self) -> None:
        """ref: ssspy/bss/ica.py:661-707."""
        self._update_once()


class FastICA(FastICABase):
    """FastICA: w_n <- E[phi'] w_n - E[phi z], Gram-Schmidt against the rows already updated, unit
    norm (ref: ssspy/bss/ica.py:710-841).  A row of zero norm gives nan, as in the reference."""

    _algorithm = _lib.ICA_FAST

    def __init__(
        self,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        score_fn: Callable[[np.ndarray], np.ndarray] = None,
        d_score_fn: Callable[[np.ndarray], np.ndarray] = None,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        record_loss: bool = True,
    ) -> None:
        super().__init__(
            contrast_fn=contrast_fn,
            score_fn=score_fn,
            d_score_fn=d_score_fn,
            callbacks=callbacks,
            record_loss=record_loss,
        )

    def update_once(self) -> None:
        """ref: ssspy/bss/ica.py:801-841."""
        self._update_once()


class GradLaplaceICA(GradICA):
    """Gradient ICA with the Laplace model, G = |y|, phi = sign (ref: ssspy/bss/ica.py:844-966)."""

    def __init__(
        self,
        step_size: float = 1e-1,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        is_holonomic: bool = False,
        record_loss: bool = True,
    ) -> None:
        super().__init__(
            step_size=step_size,
            contrast_fn=laplace_contrast,
            score_fn=laplace_score,
            callbacks=callbacks,
            is_holonomic=is_holonomic,
            record_loss=record_loss,
        )

    def __repr__(self) -> str:
        return self._repr_with_holonomic("GradLaplaceICA")


class NaturalGradLaplaceICA(NaturalGradICA):
    """Natural-gradient ICA with the Laplace model (ref: ssspy/bss/ica.py:969-1095)."""

    def __init__(
        self,
        step_size: float = 1e-1,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        is_holonomic: bool = False,
        record_loss: bool = True,
    ) -> None:
        super().__init__(
            step_size=step_size,
            contrast_fn=laplace_contrast,
            score_fn=laplace_score,
            callbacks=callbacks,
            is_holonomic=is_holonomic,
            record_loss=record_loss,
        )

    def __repr__(self) -> str:
        return self._repr_with_holonomic("NaturalGradLaplaceICA")
