"""Blind source separation by primal-dual splitting (PDSBSS, MaskingPDSBSS) on MI355X.

Drop-in classes for the reference's ``ssspy.bss.pdsbss`` (ssspy/bss/pdsbss.py).  The state is the
demixing filters W and a spectrogram-sized dual variable per penalty; an iteration is three passes
(csrc/pdsbss.hip):

* the contraction ``XY_i = (sum_q dual_q)_i X_i^H`` per bin,
* the filter step ``Wt = prox.neg_logdet(W - mu1 mu2 XY, mu1)`` (one N x N singular value
  decomposition per bin by a one-sided Jacobi) with the relaxation of W,
* per penalty the dual step ``Z = dual_q + (2 Wt - W) x``, ``Yt = Z - prox_q(Z, 1 / mu2)`` and the
  relaxation of ``dual_q``.

``prox.l1`` and ``prox.l21`` (over bins, frames or sources) are applied by the kernels when they are
passed as themselves or as a ``functools.partial`` that leaves ``step_size`` open
(``proxbss.device_prox``).  Any other callable takes the compatibility path: Z comes to the host, the
callable runs once per mixture on an ``(n_sources, n_bins, n_frames)`` array, Yt goes back up; the
contraction and the filter step stay on the device.  The mask of ``MaskingPDSBSS`` is always a user
callable: Z comes to the host, the mask goes up, ``Z - mask Z`` and the relaxation run on the device.

Extension over the reference: ``(n_mixtures, n_channels, n_bins, n_frames)`` input separates a batch,
``dual`` then carries the same leading axis.  2..16 sources.
"""

from typing import Callable, List, Optional, Union

import numpy as np

from .. import _device as dv
from .. import _lib, _ops
from ._device_state import Synced
from .proxbss import ProxBSSBase, device_prox

__all__ = ["PDSBSSBase", "PDSBSS", "MaskingPDSBSS"]


class PDSBSSBase(ProxBSSBase):
    """Base class of blind source separation via proximal splitting algorithm
    (ref: ssspy/bss/pdsbss.py:14-55).  ``record_loss=None`` records no loss, see ``ProxBSSBase``."""

    dual = Synced(dv.c128)  # (B, Q, N, F, T); (B, N, F, T) for the masking class

    def __repr__(self) -> str:
        s = "PDSBSS("
        s += "n_penalties={n_penalties}".format(n_penalties=self.n_penalties)
        s += ", scale_restoration={scale_restoration}"
        s += ", record_loss={record_loss}"
        if self.scale_restoration:
            s += ", reference_id={reference_id}"
        s += ")"
        return s.format(**self.__dict__)

    def _init_steps(self, mu1, mu2, alpha, relaxation) -> None:
        self.mu1, self.mu2 = mu1, mu2
        self._init_relaxation(alpha, relaxation)

    def _reset(self, **kwargs) -> None:
        """ref: ssspy/bss/pdsbss.py:173-195, :366-389."""
        super()._reset(**kwargs)
        self._reset_states({"dual": self._penalty_state_shape()})
        B, N, F, T = self._X.shape
        dev = self._X.device
        self._XY = dv.empty((B, F, N, N), dv.c128, dev)
        self._W2 = dv.empty((B, F, N, N), dv.c128, dev)

    def _filter_step(self):
        """Steps (a) and (b): returns (dual (B,Q,N,F,T), the filter 2 Wt - W of the dual step)."""
        dual = self._state5("dual")
        W = self._state_dev("demix_filter")
        _ops.pdsbss_contract(dual, self._X, out=self._XY)
        _ops.pdsbss_filter_step(W, self._XY, self._W2, self.mu1, self.mu2, self.relaxation)
        self._state_touch("demix_filter")
        return dual, self._W2

    def _host_z(self, dual, W2, q):
        """Z = dual_q + W2 x of every mixture on the host, (B, N, F, T)."""
        Z = _ops.pdsbss_form_z(self._X, W2, dual, q)
        self._check_device_errors()
        return dv.to_host(Z)

    def _given_step(self, dual, W2, q, kind, values) -> None:
        """The dual step with what the host formed from Z (Yt or the mask)."""
        aux = dv.to_device(values, dtype=np.complex128, dev=self._X.device)
        _ops.pdsbss_dual_step(self._X, W2, dual, q, kind, 1 / self.mu2, self.relaxation, aux=aux)


class PDSBSS(PDSBSSBase):
    """Blind source separation via proximal splitting algorithm (ref: ssspy/bss/pdsbss.py:58-219).

    ``prox_penalty``: a callable ``f(z, step_size=...)`` or a list of them, one per penalty.
    ``record_loss=None`` (the default) records no loss even with ``penalty_fn``, as in the reference
    (see ``ProxBSSBase``); pass ``record_loss=True``.
    """

    def __init__(
        self,
        mu1: float = 1,
        mu2: float = 1,
        alpha: float = None,
        relaxation: float = 1,
        penalty_fn: Optional[Callable[[np.ndarray], float]] = None,
        prox_penalty: Callable[[np.ndarray, float], np.ndarray] = None,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: Optional[bool] = None,
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
        self._init_steps(mu1, mu2, alpha, relaxation)

    def __call__(
        self, input: np.ndarray, n_iter: int = 100, initial_call: bool = True, **kwargs
    ) -> np.ndarray:
        """Separate a frequency-domain multichannel mixture (ref: ssspy/bss/pdsbss.py:126-156).
        ``demix_filter`` and ``dual`` may be injected by keyword; they are copied."""
        return self._run(input, n_iter, initial_call, kwargs)

    def __repr__(self) -> str:
        s = "PDSBSS("
        s += "mu1={mu1}, mu2={mu2}"
        s += ", relaxation={relaxation}"
        s += ", n_penalties={n_penalties}".format(n_penalties=self.n_penalties)
        s += ", scale_restoration={scale_restoration}"
        s += ", record_loss={record_loss}"
        if self.scale_restoration:
            s += ", reference_id={reference_id}"
        s += ")"
        return s.format(**self.__dict__)

    def update_once(self) -> None:
        """Update demixing filters and dual parameters once (ref: ssspy/bss/pdsbss.py:197-219)."""
        dual, W2 = self._filter_step()
        step_size = 1 / self.mu2
        for q, prox_penalty in enumerate(self.prox_penalty):
            kind = device_prox(prox_penalty)
            if kind is None:
                # the compatibility path: the callable on the host, once per mixture
                Z = self._host_z(dual, W2, q)
                Yt = self._host_prox(Z, prox_penalty, step_size, residual=True)
                self._given_step(dual, W2, q, _lib.PROX_GIVEN, Yt)
                continue
            r2 = None
            if kind == _lib.PROX_L21_BINS:
                r2 = _ops.pdsbss_bin_norms(self._X, W2, dual, q)
            _ops.pdsbss_dual_step(self._X, W2, dual, q, kind, step_size, self.relaxation, r2=r2)
        self._state_touch("dual")


class MaskingPDSBSS(PDSBSSBase):
    """Blind source separation via proximal splitting algorithm with masking
    (ref: ssspy/bss/pdsbss.py:222-412).

    ``mask_fn(z)`` returns a mask that broadcasts against ``z`` (n_sources, n_bins, n_frames).
    ``record_loss=None`` records no loss, see ``ProxBSSBase``.  With ``record_loss=True`` the loss is
    ``penalty_fn(Y) - sum_i log|det W_i|`` (the reference's ``compute_loss`` iterates over the single
    callable and raises there).
    """

    _masking = True

    def __init__(
        self,
        mu1: float = 1,
        mu2: float = 1,
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
        self._init_steps(mu1, mu2, alpha, relaxation)

    def __call__(
        self, input: np.ndarray, n_iter: int = 100, initial_call: bool = True, **kwargs
    ) -> np.ndarray:
        """Separate a frequency-domain multichannel mixture (ref: ssspy/bss/pdsbss.py:320-350)."""
        return self._run(input, n_iter, initial_call, kwargs)

    def __repr__(self) -> str:
        s = "MaskingPDSBSS("
        s += "mu1={mu1}, mu2={mu2}"
        s += ", relaxation={relaxation}"
        s += ", scale_restoration={scale_restoration}"
        s += ", record_loss={record_loss}"
        if self.scale_restoration:
            s += ", reference_id={reference_id}"
        s += ")"
        return s.format(**self.__dict__)

    def update_once(self) -> None:
        """Update demixing filters and dual parameters once (ref: ssspy/bss/pdsbss.py:396-412)."""
        dual, W2 = self._filter_step()
        mask = self._host_mask_fn(self._host_z(dual, W2, 0))
        self._given_step(dual, W2, 0, _lib.PROX_MASK, mask)
        self._state_touch("dual")
