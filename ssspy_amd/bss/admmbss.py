"""Blind source separation by the alternating direction method of multipliers (ADMMBSS,
MaskingADMMBSS) on MI355X.

Drop-in classes for the reference's ``ssspy.bss.admmbss`` (ssspy/bss/admmbss.py).  The state is the
demixing filters W, ``auxiliary1`` / ``dual1`` of the filters' shape and ``auxiliary2`` / ``dual2``
of the spectrogram's shape per penalty.  Once per call the inverse of ``n_penalties conj(X) X^T + I``
is formed per bin (constant over the iterations; the reference solves it anew every time); an
iteration is three passes (csrc/admmbss.hip):

* the contraction ``R_i = (sum_q (auxiliary2_q - dual2_q))_i X_i^H`` per bin,
* the filter step ``W = Ainv (auxiliary1 - dual1 + R)``, ``U = relaxation W + (1 - relaxation)
  auxiliary1``, ``auxiliary1 <- prox.neg_logdet(U + dual1, 1 / rho)``, ``dual1 <- dual1 + U -
  auxiliary1``, a lane per bin,
* per penalty the auxiliary step ``Z = relaxation W x + (1 - relaxation) auxiliary2_q + dual2_q``,
  ``auxiliary2_q <- prox_q(Z, 1 / rho)``, ``dual2_q <- Z - auxiliary2_q``.

From the default zero state the first iteration gives ``W = 0`` and ``auxiliary1 = sqrt(1 / rho) I``
(what the reference's LAPACK returns for a zero matrix), and the loss recorded there is ``+inf``.

``prox.l1`` and ``prox.l21`` are applied by the kernels when ``proxbss.device_prox`` recognises them;
any other callable, and the mask of ``MaskingADMMBSS``, takes the compatibility path: Z comes to the
host, the callable runs once per mixture on an ``(n_sources, n_bins, n_frames)`` array, the value (or
the mask) goes back up; the contraction and the filter step stay on the device.

Extension over the reference: ``(n_mixtures, n_channels, n_bins, n_frames)`` input separates a batch,
every state then carries the same leading axis.  2..16 sources.
"""

import warnings
from typing import Callable, List, Optional, Union

import numpy as np

from .. import _device as dv
from .. import _lib, _ops
from ._device_state import Synced
from .proxbss import ProxBSSBase, device_prox

__all__ = ["ADMMBSS", "MaskingADMMBSS"]


class ADMMBSSBase(ProxBSSBase):
    """Base class of blind source separation via alternative direction method of multiplier
    (ref: ssspy/bss/admmbss.py:15-52)."""

    auxiliary1 = Synced(dv.c128)
    dual1 = Synced(dv.c128)
    auxiliary2 = Synced(dv.c128)
    dual2 = Synced(dv.c128)  # (these two (B, Q, N, F, T); (B, N, F, T) for the masking class)

    def __repr__(self) -> str:
        s = "ADMMBSS("
        s += "n_penalties={n_penalties}".format(n_penalties=self.n_penalties)
        s += ", scale_restoration={scale_restoration}"
        s += ", record_loss={record_loss}"
        if self.scale_restoration:
            s += ", reference_id={reference_id}"
        s += ")"
        return s.format(**self.__dict__)

    def _init_steps(self, rho, alpha, relaxation) -> None:
        self.rho = rho
        self._init_relaxation(alpha, relaxation)

    def _reset(self, **kwargs) -> None:
        """ref: ssspy/bss/admmbss.py:168-218, :357-408."""
        for old, new in (("aux1", "auxiliary1"), ("aux2", "auxiliary2")):
            if old in kwargs:
                warnings.warn("{} is deprecated. Use {} instead.".format(old, new),
                              DeprecationWarning)
                kwargs[new] = kwargs.pop(old)
        super()._reset(**kwargs)
        B, N, F, T = self._X.shape
        aux2 = self._penalty_state_shape()
        self._reset_states({"auxiliary1": (B, F, N, N), "dual1": (B, F, N, N), "auxiliary2": aux2,
                            "dual2": aux2})
        # (Q conj(X) X^T + I)^-1 per bin: constant over the iterations of this call
        self._Ainv = _ops.admmbss_gram_inverse(self._X, self.n_penalties)
        self._R = dv.empty((B, F, N, N), dv.c128, self._X.device)

    def _filter_step(self):
        """The contraction and the filter step: returns (W, auxiliary2, dual2), the last two as
        (B, Q, N, F, T)."""
        aux2, dual2 = self._state5("auxiliary2"), self._state5("dual2")
        W = self._state_dev("demix_filter")
        _ops.admmbss_contract(aux2, dual2, self._X, out=self._R)
        _ops.admmbss_filter_step(self._Ainv, self._R, W, self._state_dev("auxiliary1"),
                                 self._state_dev("dual1"), self.rho, self.relaxation)
        for name in ("demix_filter", "auxiliary1", "dual1"):
            self._state_touch(name)
        return W, aux2, dual2

    def _host_z(self, W, aux2, dual2, q):
        """Z of every mixture on the host, (B, N, F, T)."""
        Z = _ops.admmbss_form_z(self._X, W, aux2, dual2, q, self.relaxation)
        self._check_device_errors()
        return dv.to_host(Z)

    def _given_step(self, W, aux2, dual2, q, kind, values) -> None:
        """The auxiliary step with what the host formed from Z (the prox value or the mask)."""
        given = dv.to_device(values, dtype=np.complex128, dev=self._X.device)
        _ops.admmbss_aux_step(self._X, W, aux2, dual2, q, kind, 1 / self.rho, self.relaxation,
                              given=given)

    def compute_loss(self) -> float:
        """sum_q penalty_q(Y) - sum_i log|det W_i| (ref: ssspy/bss/proxbss.py:172-189).  The
        log-determinant is ``numpy.linalg.slogdet`` on a host copy of the filters: at ``W = 0`` (the
        first iteration from the zero state) it is ``-inf`` there and the loss ``+inf``, as in the
        reference; the elimination of the device sum multiplies by the reciprocal of the zero pivot
        and does not end at ``-inf``.  The
        penalties already run on a host copy of the estimate, (N, F, T) against these (F, N, N)."""
        W = self._state_dev("demix_filter")
        Y = _ops.separate(self._X, W)
        self._check_device_errors()
        values = [penalty - np.sum(self.compute_logdet(Wb))
                  for penalty, Wb in zip(self._host_penalties(Y), dv.to_host(W))]
        return self._loss_entry(np.asarray(values, dtype=np.float64).reshape(-1))


class ADMMBSS(ADMMBSSBase):
    """Blind source separation via alternative direction method of multiplier
    (ref: ssspy/bss/admmbss.py:55-257).

    ``prox_penalty``: a callable ``f(z, step_size=...)`` or a list of them, one per penalty.
    ``record_loss`` defaults to ``True`` as in the reference, so ``penalty_fn`` is needed unless
    ``record_loss=False`` is passed.
    """

    def __init__(
        self,
        rho: float = 1,
        alpha: float = None,
        relaxation: float = 1,
        penalty_fn: Optional[Callable[[np.ndarray], float]] = None,
        prox_penalty: Callable[[np.ndarray, float], np.ndarray] = None,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(
            penalty_fn=penalty_fn,
            prox_penalty=prox_penalty,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        self._init_steps(rho, alpha, relaxation)

    def __call__(
        self, input: np.ndarray, n_iter: int = 100, initial_call: bool = True, **kwargs
    ) -> np.ndarray:
        """Separate a frequency-domain multichannel mixture (ref: ssspy/bss/admmbss.py:121-151).
        ``demix_filter``, ``auxiliary1``, ``dual1``, ``auxiliary2`` and ``dual2`` may be injected by
        keyword; they are copied."""
        return self._run(input, n_iter, initial_call, kwargs)

    def __repr__(self) -> str:
        s = "ADMMBSS("
        s += "rho={rho}"
        s += ", relaxation={relaxation}"
        s += ", n_penalties={n_penalties}".format(n_penalties=self.n_penalties)
        s += ", scale_restoration={scale_restoration}"
        s += ", record_loss={record_loss}"
        if self.scale_restoration:
            s += ", reference_id={reference_id}"
        s += ")"
        return s.format(**self.__dict__)

    def update_once(self) -> None:
        """Update demixing filters, auxiliary parameters, and dual parameters once
        (ref: ssspy/bss/admmbss.py:220-257)."""
        W, aux2, dual2 = self._filter_step()
        step_size = 1 / self.rho
        for q, prox_penalty in enumerate(self.prox_penalty):
            kind = device_prox(prox_penalty)
            if kind is None:
                # the compatibility path: the callable on the host, once per mixture
                V = self._host_prox(self._host_z(W, aux2, dual2, q), prox_penalty, step_size)
                self._given_step(W, aux2, dual2, q, _lib.PROX_GIVEN, V)
                continue
            r2 = None
            if kind == _lib.PROX_L21_BINS:
                r2 = _ops.admmbss_bin_norms(self._X, W, aux2, dual2, q, self.relaxation)
            _ops.admmbss_aux_step(self._X, W, aux2, dual2, q, kind, step_size, self.relaxation,
                                  r2=r2)
        self._state_touch("auxiliary2")
        self._state_touch("dual2")


class MaskingADMMBSS(ADMMBSSBase):
    """Blind source separation via alternative direction method of multiplier with masking
    function (ref: ssspy/bss/admmbss.py:260-442).

    ``mask_fn(z)`` returns a mask that broadcasts against ``z`` (n_sources, n_bins, n_frames).
    ``record_loss=None`` records no loss, see ``ProxBSSBase``.  With ``record_loss=True`` the loss is
    ``penalty_fn(Y) - sum_i log|det W_i|`` (the reference's ``compute_loss`` iterates over the single
    callable and raises there).
    """

    _masking = True

    def __init__(
        self,
        rho: float = 1,
        alpha: float = None,
        relaxation: float = 1,
        penalty_fn: Optional[Callable[[np.ndarray], float]] = None,
        mask_fn: Callable[[np.ndarray], np.ndarray] = None,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: Optional[bool] = None,
        reference_id: int = 0,
    ) -> None:
        self._init_masking(penalty_fn, mask_fn, callbacks, scale_restoration, record_loss,
                           reference_id)
        self._init_steps(rho, alpha, relaxation)

    def __call__(
        self, input: np.ndarray, n_iter: int = 100, initial_call: bool = True, **kwargs
    ) -> np.ndarray:
        """Separate a frequency-domain multichannel mixture (ref: ssspy/bss/admmbss.py:342-355)."""
        return self._run(input, n_iter, initial_call, kwargs)

    def update_once(self) -> None:
        """Update demixing filters, auxiliary parameters, and dual parameters once
        (ref: ssspy/bss/admmbss.py:415-442)."""
        W, aux2, dual2 = self._filter_step()
        mask = self._host_mask_fn(self._host_z(W, aux2, dual2, 0))
        self._given_step(W, aux2, dual2, 0, _lib.PROX_MASK, mask)
        self._state_touch("auxiliary2")
        self._state_touch("dual2")
