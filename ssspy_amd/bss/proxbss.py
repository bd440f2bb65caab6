"""Base class of the proximal BSS family on MI355X (ref: ssspy/bss/proxbss.py).

The source model of a proximal separator is a list of proximal operators, one per penalty term.  The
operators of ``ssspy_amd.linalg.prox`` are recognised by identity (``device_prox``) and applied by the
separator's own kernels; any other callable runs on the host, once per mixture, on the reference's
``(n_sources, n_bins, n_frames)`` arrays.  Scale restoration and the filter state are those of the
other demixing-filter separators (``DemixingFilterBase``).
"""

import functools
import warnings
from typing import Callable, List, Optional, Union

import numpy as np

from .. import _device as dv
from .. import _lib, _ops
from ..linalg import prox
from ._filter_base import DemixingFilterBase
from .base import IterativeMethodBase

__all__ = ["ProxBSSBase", "device_prox"]

_L21_AXES = {1: _lib.PROX_L21_BINS, -2: _lib.PROX_L21_BINS, 2: _lib.PROX_L21_FRAMES,
             -1: _lib.PROX_L21_FRAMES, 0: _lib.PROX_L21_SOURCES, -3: _lib.PROX_L21_SOURCES}


def device_prox(fn):
    """The _lib.PROX_* kind the kernels apply for ``fn``, or None for a callable only the host can
    run.  Recognised: ``prox.l1`` and ``prox.l21`` themselves, or a ``functools.partial`` of them
    with keywords only that leaves ``step_size`` open (the separator passes ``1 / mu2``); for ``l21``
    the group axis ``axis2`` on an ``(n_sources, n_bins, n_frames)`` array (``axis1`` is unused, as in
    the reference).  A lambda around them, or a function of the same name from elsewhere, is not."""
    keywords = {}
    if isinstance(fn, functools.partial):
        if fn.args:
            return None
        fn, keywords = fn.func, fn.keywords
    if "step_size" in keywords:
        return None
    if fn is prox.l1:
        return None if keywords else _lib.PROX_L1
    if fn is prox.l21:
        if set(keywords) - {"axis1", "axis2"}:
            return None
        axis2 = keywords.get("axis2", -1)
        if isinstance(axis2, (int, np.integer)) and not isinstance(axis2, bool):
            return _L21_AXES.get(int(axis2))
    return None


class ProxBSSBase(DemixingFilterBase):
    """Base class of blind source separation via proximal gradient method
    (ref: ssspy/bss/proxbss.py:16-266).

    One quirk of the reference is kept on purpose: the default of ``record_loss=None`` is worked out
    in a local variable and never stored (proxbss.py:58-70), so with the default the attribute stays
    ``None`` and NO loss is recorded even when ``penalty_fn`` is given; the loss list is filled only
    for an explicit ``record_loss=True``.
    """

    def __init__(
        self,
        penalty_fn: Optional[Callable[[np.ndarray], float]] = None,
        prox_penalty: Callable[[np.ndarray, float], np.ndarray] = None,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: Optional[bool] = None,
        reference_id: int = 0,
    ) -> None:
        self._init_iterative(callbacks, record_loss)
        if penalty_fn is None:
            # (penalty_fn is not necessarily written in closed form: None is acceptable)
            assert not record_loss, "To record loss, set penalty_fn."
        elif callable(penalty_fn):
            penalty_fn = [penalty_fn]
        if prox_penalty is None:
            raise ValueError("Specify proximal operator of penalty function.")
        if callable(prox_penalty):
            prox_penalty = [prox_penalty]
        self.penalty_fn = penalty_fn
        self.prox_penalty = prox_penalty
        if self.penalty_fn is not None:
            assert len(self.penalty_fn) == len(
                self.prox_penalty
            ), "Length of penalty_fn and prox_penalty are different."
        self._init_scale(scale_restoration, reference_id)

    _masking = False  # (the masking classes: one penalty, its state without the penalty axis)

    def _init_masking(self, penalty_fn, mask_fn, callbacks, scale_restoration, record_loss,
                      reference_id) -> None:
        """The constructor of a masking class: ``mask_fn`` in the place of ``prox_penalty``."""
        self._init_iterative(callbacks, record_loss)
        if penalty_fn is None:
            assert not record_loss, "To record loss, set penalty_fn."
        else:
            assert callable(penalty_fn), "penalty_fn should be callable."
        if mask_fn is None:
            raise ValueError("Specify masking function.")
        assert callable(mask_fn), "mask_fn should be callable."
        self.penalty_fn = penalty_fn
        self.mask_fn = mask_fn
        self._init_scale(scale_restoration, reference_id)

    def _init_relaxation(self, alpha, relaxation) -> None:
        """``relaxation``, or ``alpha``, its deprecated name."""
        if alpha is None:
            self.relaxation = relaxation
        else:
            assert relaxation == 1, "You cannot specify relaxation and alpha simultaneously."
            warnings.warn("alpha is deprecated. Set relaxation instead.", DeprecationWarning)
            self.relaxation = alpha

    def _init_iterative(self, callbacks, record_loss) -> None:
        IterativeMethodBase.__init__(self, callbacks=callbacks, record_loss=record_loss)
        self.record_loss = record_loss  # (as given: None stays None, see the class docstring)

    def _init_scale(self, scale_restoration, reference_id) -> None:
        self.input = None
        self.scale_restoration = scale_restoration
        if reference_id is None and scale_restoration:
            raise ValueError("Specify 'reference_id' if scale_restoration=True.")
        self.reference_id = reference_id

    def __repr__(self) -> str:
        s = "ProxBSSBase("
        s += "n_penalties={n_penalties}".format(n_penalties=self.n_penalties)
        s += ", scale_restoration={scale_restoration}"
        s += ", record_loss={record_loss}"
        if self.scale_restoration:
            s += ", reference_id={reference_id}"
        s += ")"
        return s.format(**self.__dict__)

    def _run(self, input, n_iter, initial_call, kwargs):
        """``__call__`` of the splitting separators (ref: ssspy/bss/pdsbss.py:126-156, :320-350;
        ssspy/bss/admmbss.py:121-151, :342-355)."""
        self._bind_input(input)
        self._reset(**kwargs)
        IterativeMethodBase.__call__(self, n_iter=n_iter, initial_call=initial_call)
        return self._finish_call()

    def _reset(self, **kwargs) -> None:
        """ref: ssspy/bss/proxbss.py:107-139."""
        assert self._has_input(), "Specify data!"
        if self._X.shape[1] > _lib.RT_MAX_SOURCES:
            raise NotImplementedError(
                "{} takes up to {} sources, got {}.".format(
                    type(self).__name__, _lib.RT_MAX_SOURCES, self._X.shape[1]))
        for key, value in kwargs.items():
            setattr(self, key, value)
        B, N, F, T = self._X.shape
        self.n_sources, self.n_channels = N, N
        self.n_bins, self.n_frames = F, T
        if not self._state_has("demix_filter"):
            self.demix_filter = np.tile(np.eye(N, dtype=np.complex128), self._lead() + (F, 1, 1))
        elif not self._state_is_none("demix_filter"):
            # (a copy: the filters given by keyword are not overwritten)
            self.demix_filter = np.array(self.demix_filter, dtype=np.complex128, copy=True)
        if self._state_is_none("demix_filter"):
            raise ValueError("demix_filter=None cannot be given at reset.")
        self._state_set_dev("output", _ops.separate(self._X, self._state_dev("demix_filter")))

    def _penalty_state_shape(self):
        """The shape of a spectrogram-sized state: an axis of penalties unless masking."""
        B, N, F, T = self._X.shape
        return (B, N, F, T) if self._masking else (B, self.n_penalties, N, F, T)

    def _reset_states(self, shapes) -> None:
        """The states ``{name: shape}`` beside the filters: zeros unless given by keyword, then copied
        (ref: ssspy/bss/pdsbss.py:173-195, :366-389; ssspy/bss/admmbss.py:168-218, :357-408)."""
        for name, shape in shapes.items():
            if not self._state_has(name):
                self._state_set_dev(name, dv.zeros(shape, dv.c128, self._X.device))
            elif not self._state_is_none(name):
                # (a copy: a state given by keyword is not overwritten)
                setattr(self, name, np.array(getattr(self, name), dtype=np.complex128, copy=True))
            if self._state_is_none(name):
                raise ValueError("{}=None cannot be given at reset.".format(name))
            got = tuple(self._state_dev(name).shape)
            if got != shape:
                skip = 0 if self._batched else 1
                raise ValueError("{} must have shape {}, got {}.".format(name, shape[skip:],
                                                                         got[skip:]))

    def _state5(self, name):
        """A spectrogram-sized state as (B, Q, N, F, T) (a view for the masking classes)."""
        state = self._state_dev(name)
        return state if state.dim() == 5 else state.unsqueeze(1)

    def _host_prox(self, Z, prox_penalty, step_size, residual=False):
        """The compatibility path: ``prox_penalty(Z)`` on the host, once per mixture of Z
        (B, N, F, T); ``residual``: ``Z - prox_penalty(Z)``.  The shape is checked on what is
        returned, so under ``residual`` the operator's value may broadcast against Z, as in the
        reference (ssspy/bss/pdsbss.py:213)."""
        V = [np.asarray(prox_penalty(Zb, step_size=step_size)) for Zb in Z]
        V = np.stack([Zb - Vb for Zb, Vb in zip(Z, V)] if residual else V)
        if V.shape != Z.shape:
            raise ValueError("prox_penalty must map (n_sources, n_bins, n_frames) to the "
                             "same shape.")
        return V

    def _host_mask_fn(self, Z):
        """``mask_fn(Z)`` on the host, once per mixture, broadcast to Z (B, N, F, T)."""
        return np.stack([np.broadcast_to(np.asarray(self.mask_fn(Zb)), Zb.shape) for Zb in Z])

    @property
    def n_penalties(self):
        """Number of penalty terms."""
        return 1 if self._masking else len(self.prox_penalty)

    def separate(self, input: np.ndarray, demix_filter: np.ndarray) -> np.ndarray:
        """y_ij = W_i x_ij (ref: ssspy/bss/proxbss.py:147-170); NumPy in, NumPy out."""
        batched = input.ndim == 4
        X = dv.to_device(input if batched else input[None], dtype=np.complex128)
        W = dv.to_device(demix_filter if batched else demix_filter[None], dtype=np.complex128)
        Y = dv.to_host(_ops.separate(X, W))
        return Y if batched else Y[0]

    def _penalty_fns(self):
        return [self.penalty_fn] if self._masking else self.penalty_fn

    def _host_penalties(self, Y):
        """sum_q penalty_q(Y) of every mixture of the device estimate Y, on the host."""
        values = []
        for Yb in dv.to_host(Y):
            penalty = 0
            for penalty_fn in self._penalty_fns():
                penalty = penalty + penalty_fn(Yb)
            values.append(penalty)
        return values

    def compute_loss(self) -> float:
        """sum_q penalty_q(Y) - sum_i log|det W_i| (ref: ssspy/bss/proxbss.py:172-189): the penalties
        on the host on the separated estimate of each mixture, the log-determinant on the device."""
        W = self._state_dev("demix_filter")
        logdet = _ops.sum_logdet(W)
        Y = _ops.separate(self._X, W)
        self._check_device_errors()
        values = np.asarray(self._host_penalties(Y), dtype=np.float64).reshape(-1)
        return self._loss_entry(values - dv.to_host(logdet))

    def compute_logdet(self, demix_filter: np.ndarray) -> np.ndarray:
        """log|det W_i| per bin (ref: ssspy/bss/proxbss.py:191-203)."""
        _, logdet = np.linalg.slogdet(demix_filter)
        return logdet

    def normalize_by_spectral_norm(self, input: np.ndarray, n_penalties: int = None) -> np.ndarray:
        """``input / (sqrt(n_penalties) max_i ||X_i||_2)`` (ref: ssspy/bss/proxbss.py:205-223): the
        spectral norm of a bin is the square root of the largest eigenvalue of X_i X_i^H, from the
        covariance and ``eigh`` operators; a batch is normalised per mixture."""
        from ..linalg import eigh

        if n_penalties is None:
            n_penalties = self.n_penalties
        input = np.asarray(input)
        batched = input.ndim == 4
        X = dv.to_device(input if batched else input[None], dtype=np.complex128)
        B, N, F, T = X.shape
        C = dv.to_host(_ops.weighted_covariance(X).reshape(B, F, N, N))  # mean_j x x^H
        lamb, _ = eigh(C)
        norm = np.sqrt(T * np.max(lamb[..., -1], axis=-1))  # (B,)
        scale = np.sqrt(n_penalties) * norm
        return input / (scale[:, None, None, None] if batched else scale[0])
