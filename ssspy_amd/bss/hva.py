"""Harmonic vector analysis (MaskingPDSHVA, HVA) on MI355X.

Drop-in classes for the reference's ``ssspy.bss.hva`` (ssspy/bss/hva.py:20-155, :278-298):
``MaskingPDSBSS`` with one fixed mask, the cosine shrinkage of the cepstrum of every
(source, frame) column of ``Z``.  Per column, along the bins, with ``D`` the DCT-I (what both
``irfft`` calls of the reference compute on a real input of ``n_bins`` points)::

    zeta = log(flooring_fn(|Z|)),  m = mean(zeta),  rho = zeta - m
    nu = D(rho) / (2 (n_bins - 1))
    sigma = min(1, nu);  mask_iter times: sigma <- (1 - cos(pi sigma)) / 2
    varrho = D(sigma nu) + m
    mask_n = (exp(2 varrho_n) / sum_n' exp(2 varrho_n')) ** attenuation

Two routes per iteration, after the contraction and the filter step of ``PDSBSSBase``:

* the device route (csrc/hva.hip), taken when ``flooring_fn`` is ``None`` / ``identity``,
  ``max_flooring``, ``add_flooring`` or a ``functools.partial`` of those that fixes ``eps`` only
  (``utils.flooring.device_flooring``): a cepstral pass leaves the real ``varrho`` on the device, the
  masked dual step forms ``Z`` again, the mask and the relaxation of ``dual``.  Nothing crosses to
  the host.  The mask is formed as ``exp(2 g (varrho_n - max)) / (sum exp(2 (varrho - max))) ** g``
  with the maximum over sources subtracted; that equals the reference's expression wherever the
  reference's ``exp`` neither overflows nor underflows to 0 / 0, and stays finite where it does.
  2..16 sources, ``n_bins`` in 2..8192, any number of frames, ``mask_iter >= 0``.  The transform
  along the bins is an FFT resident in LDS when ``n_bins - 1`` is a power of two (up to 4097 bins),
  else the direct sum; ``transform_route()`` tells which.
* the compatibility route, for any other ``flooring_fn``: the inherited
  ``MaskingPDSBSS.update_once`` with the host ``mask_fn`` (``Z`` to the host, the mask back up).

``mask_fn`` stays a public attribute, the host NumPy form of the mask, for callbacks and users.
``n_bins == 1`` raises ``ValueError`` on either route, as the reference's ``irfft`` does.

``MaskingADMMHVA`` (ssspy/bss/hva.py:158-275) is the same mask inside the auxiliary step of
``MaskingADMMBSS``, with the same two routes under the same conditions; what the two classes share
is stated once, in ``HVAMask``.
"""

import functools
import math
from typing import Callable, List, Optional, Union

import numpy as np

from .. import _device as dv
from .. import _lib, _ops
from ..special.flooring import EPS, identity, max_flooring
from ..utils.flooring import device_flooring, host_floor
from .admmbss import MaskingADMMBSS
from .pdsbss import MaskingPDSBSS

# (MaskingADMMHVA is a module attribute and is listed in ssspy_amd.bss.__all__; this list stays as the
# tests of the PDS classes pin it, as admmbss.__all__ does)
__all__ = ["MaskingPDSHVA", "HVA"]


_SINGLE_BIN = ("Invalid number of FFT data points (0) specified: the mask of HVA needs two bins at "
               "least.")


class HVAMask:
    """What MaskingPDSHVA and MaskingADMMHVA share, stated once: the host mask, which ``flooring_fn``
    the kernels can apply, the transform route, the ``attenuation=None`` quirk, the refusal of a
    single bin and the device buffers of the cepstral pass.  Mixed in before the masking separator."""

    _transform_route = _lib.HVA_ROUTE_AUTO  # (the benchmark and the tests force the other one)

    def _init_hva(self, attenuation, mask_iter, flooring_fn) -> None:
        self.attenuation = attenuation
        self.mask_iter = mask_iter
        self.flooring_fn = identity if flooring_fn is None else flooring_fn

    def _resolve_attenuation(self, n_sources: int) -> None:
        """``attenuation=None`` becomes ``1 / n_sources`` on the instance, as in the reference."""
        if self.attenuation is None:
            self.attenuation = 1 / n_sources

    def _host_mask(self, y: np.ndarray) -> np.ndarray:
        """The mask of ``y`` (n_sources, n_bins, n_frames) in NumPy (ref: ssspy/bss/hva.py:81-115,
        :202-236)."""
        n_sources, n_bins, _ = y.shape
        if n_bins < 2:
            raise ValueError(_SINGLE_BIN)
        self._resolve_attenuation(n_sources)
        zeta = np.log(self.flooring_fn(np.abs(y)))
        zeta_mean = zeta.mean(axis=1, keepdims=True)
        nu = np.fft.irfft(zeta - zeta_mean, axis=1, norm="backward")[:, :n_bins]
        varsigma = np.minimum(1, nu)
        for _ in range(self.mask_iter):
            varsigma = (1 - np.cos(math.pi * varsigma)) / 2
        xi = np.fft.irfft(varsigma * nu, axis=1, norm="forward")[:, :n_bins]
        v = np.exp(2 * (xi + zeta_mean))
        return (v / v.sum(axis=0)) ** self.attenuation

    def _repr_tail(self) -> str:
        """The part of the ``repr`` both classes end with."""
        s = ", relaxation={relaxation}"
        if self.attenuation is not None:
            s += ", attenuation={attenuation}"
        s += ", mask_iter={mask_iter}"
        s += ", scale_restoration={scale_restoration}"
        s += ", record_loss={record_loss}"
        if self.scale_restoration:
            s += ", reference_id={reference_id}"
        s += ")"
        return s.format(**self.__dict__)

    def device_floor(self):
        """The ``(kind, eps)`` of ``flooring_fn`` when the kernels can apply it (the device route),
        else ``None`` (the compatibility route)."""
        floor = device_flooring(self.flooring_fn, allow_host=True)
        return None if host_floor(floor) is not None else floor

    def transform_route(self, n_bins: int) -> int:
        """The ``_lib.HVA_ROUTE_*`` the cepstral pass takes for ``n_bins`` bins."""
        return _ops.hva_route(n_bins, self._transform_route)

    def _reset(self, **kwargs) -> None:
        super()._reset(**kwargs)
        self._varrho = self._table = None
        B, N, F, T = self._X.shape
        if F < 2:
            raise ValueError(_SINGLE_BIN)
        if self.device_floor() is not None:
            self._varrho = dv.empty((B, N, F, T), dv.f64, self._X.device)
            self._table = _ops.hva_cos_table(F, self._X.device)

    def _device_mask_setup(self):
        """``(floor, mask_iter)`` of the device route with the attenuation resolved, or ``None`` where
        this call takes the compatibility route."""
        floor = self.device_floor()
        if floor is None or self._table is None:
            return None
        self._resolve_attenuation(self._X.shape[1])
        return floor, max(int(self.mask_iter), 0)


class MaskingPDSHVA(HVAMask, MaskingPDSBSS):
    """Harmonic vector analysis (ref: ssspy/bss/hva.py:20-155): K. Yatabe and D. Kitamura,
    "Determined BSS based on time-frequency masking and its application to harmonic vector
    analysis," IEEE/ACM Trans. ASLP, vol. 29, 2021.

    ``attenuation=None`` becomes ``1 / n_sources`` and is stored on the instance at the first
    evaluation of the mask, as in the reference: the ``repr`` shows it from then on.
    """

    _repr_name = "MaskingPDSHVA"

    def __init__(
        self,
        mu1: float = 1,
        mu2: float = 1,
        alpha: float = None,
        relaxation: float = 1,
        attenuation: Optional[float] = None,
        mask_iter: int = 1,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: Optional[bool] = None,
        reference_id: int = 0,
    ) -> None:
        super().__init__(
            mu1=mu1,
            mu2=mu2,
            alpha=alpha,
            relaxation=relaxation,
            penalty_fn=None,
            mask_fn=self._host_mask,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        self._init_hva(attenuation, mask_iter, flooring_fn)

    def __repr__(self) -> str:
        return (self._repr_name + "(mu1={mu1}, mu2={mu2}").format(**self.__dict__) + self._repr_tail()

    def update_once(self) -> None:
        """Update demixing filters and dual parameters once (ref: ssspy/bss/pdsbss.py:396-412 with
        the mask of ssspy/bss/hva.py:81-115)."""
        setup = self._device_mask_setup()
        if setup is None:
            return super().update_once()
        floor, mask_iter = setup
        dual, W2 = self._filter_step()
        _ops.hva_cepstrum(self._X, W2, dual, 0, self._table, floor, mask_iter,
                          route=self._transform_route, out=self._varrho)
        _ops.hva_dual_step(self._X, W2, dual, 0, self._varrho, self.attenuation, self.relaxation)
        self._state_touch("dual")


class MaskingADMMHVA(HVAMask, MaskingADMMBSS):
    """Harmonic vector analysis using ADMM with masking (ref: ssspy/bss/hva.py:158-275): the mask of
    ``MaskingPDSHVA`` inside the auxiliary step of ``MaskingADMMBSS``.

    Per iteration, after the contraction and the filter step of ``ADMMBSSBase``, with
    ``Z = relaxation W x + (1 - relaxation) auxiliary2 + dual2``:

    * the device route (the ``flooring_fn`` of ``MaskingPDSHVA``'s device route): the cepstral pass
      over ``Z`` leaves ``varrho`` on the device, the masked auxiliary step forms ``Z`` again, the
      mask, ``auxiliary2 <- mask Z`` and ``dual2 <- Z - auxiliary2``.  Nothing crosses to the host.
    * the compatibility route, for any other ``flooring_fn``: the inherited
      ``MaskingADMMBSS.update_once`` with the host ``mask_fn``.

    2..16 sources, ``n_bins`` in 2..8192 (``n_bins == 1`` raises ``ValueError`` on either route).

    From the default zero state the first iteration gives ``W = 0`` and so ``Z = 0`` exactly.  With a
    floor the mask there is the constant ``n_sources ** -attenuation`` and ``auxiliary2 = dual2 = 0``.
    With ``flooring_fn=None`` the reference's mask is NaN there (``log 0``: the column rule the
    cepstral pass keeps) and every state is NaN from then on, here as in the reference: without a
    floor, inject states.
    """

    def __init__(
        self,
        rho: float = 1,
        alpha: float = None,
        relaxation: float = 1,
        attenuation: Optional[float] = None,
        mask_iter: int = 1,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: Optional[bool] = None,
        reference_id: int = 0,
    ) -> None:
        super().__init__(
            rho=rho,
            alpha=alpha,
            relaxation=relaxation,
            penalty_fn=None,
            mask_fn=self._host_mask,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        self._init_hva(attenuation, mask_iter, flooring_fn)

    def __repr__(self) -> str:
        return "MaskingADMMHVA(rho={rho}".format(**self.__dict__) + self._repr_tail()

    def update_once(self) -> None:
        """Update demixing filters, auxiliary parameters, and dual parameters once
        (ref: ssspy/bss/admmbss.py:415-442 with the mask of ssspy/bss/hva.py:202-236)."""
        setup = self._device_mask_setup()
        if setup is None:
            return super().update_once()
        floor, mask_iter = setup
        W, aux2, dual2 = self._filter_step()
        _ops.hva_admm_cepstrum(self._X, W, aux2, dual2, 0, self._table, floor, mask_iter,
                               self.relaxation, route=self._transform_route, out=self._varrho)
        _ops.hva_aux_step(self._X, W, aux2, dual2, 0, self._varrho, self.attenuation, self.relaxation)
        self._state_touch("auxiliary2")
        self._state_touch("dual2")


class HVA(MaskingPDSHVA):
    """Alias of MaskingPDSHVA (ref: ssspy/bss/hva.py:278-298)."""

    _repr_name = "HVA"
