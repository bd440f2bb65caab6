"""Overdetermined AuxIVA (OverIVA) on MI355X: fewer sources than channels.

R. Scheibler and N. Ono, "Independent vector analysis with more microphones than sources", WASPAA
2019.  The reference has no such class: its IVA, ILRMA, FDICA and proximal classes take
``n_sources = n_channels`` (ssspy/bss/iva.py:153).  OverIVA is AuxIVA-IP1 with only ``n_sources``
demixing rows W_t (N x M per bin); the other M - N rows of the full filter W = [W_t ; [J, -I]] model a
Gaussian background and follow in closed form from the orthogonality constraint
[J, -I] C W_t^H = 0 with C the covariance of the mixture: J = (E2 C W_t^H)(E1 C W_t^H)^-1.

An iteration is the two read-only passes over the mixture of AuxIVA-IP1 -- frame powers of W_t x
(csrc/overiva.hip), N weighted covariances on the M channels (the shared covariance pass) -- and one
per-bin step (csrc/overiva.hip): the N sequential IP1 row updates on the full filter, J re-formed
after each.  The weights and the contrast term of the loss are ``AuxLaplaceIVA`` / ``AuxGaussIVA``'s
(same kernels, same flooring place).  With ``n_sources == n_channels`` nothing is left of the
background and every number is AuxIVA-IP1's.

Loss: sum_n mean_j G(r_nj) + sum_i Re tr(U_i C_i U_i^H) - 2 sum_i log|det W_i|, U = [J, -I].
"""

import functools
from typing import Callable, List, Optional, Union

import numpy as np

from .. import _device as dv
from .. import _lib, _ops
from ..special.flooring import identity, max_flooring
from ..utils.flooring import device_flooring
from ._device_state import Synced
from ._filter_base import _IP1, _MDP, _PROJECTION_BACK, DemixingFilterBase
from .base import IterativeMethodBase

__all__ = ["OverIVABase", "OverLaplaceIVA", "OverGaussIVA"]

EPS = 1e-10
MIN_CHANNELS, MAX_CHANNELS = 2, _lib.RT_MAX_SOURCES


def check_shape(n_channels: int, n_sources: int) -> None:
    """The limits of the kernels: 2..16 channels, 1..n_channels sources."""
    if not MIN_CHANNELS <= n_channels <= MAX_CHANNELS:
        raise NotImplementedError(
            "OverIVA is built for {}..{} channels, got {}".format(MIN_CHANNELS, MAX_CHANNELS,
                                                                 n_channels))
    if not 1 <= n_sources <= n_channels:
        raise NotImplementedError(
            "OverIVA separates 1..n_channels sources, got n_sources={} on {} channels".format(
                n_sources, n_channels))


class OverIVABase(DemixingFilterBase):
    """State and iteration of OverIVA; the subclasses name the contrast.

    ``demix_filter`` is W_t, (n_bins, n_sources, n_channels); ``background_filter`` is J,
    (n_bins, n_channels - n_sources, n_sources), derived from ``demix_filter`` and never given.
    Inputs are (n_channels, n_bins, n_frames) or a batch (n_mixtures, ...), NumPy or a complex128
    tensor on the device.
    """

    _contrast = None  # SSSPY_CONTRAST_* of the subclass
    variance = Synced(dv.f64)

    def __init__(
        self,
        n_sources: Optional[int] = None,
        spatial_algorithm: str = "IP",
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(callbacks=callbacks, record_loss=record_loss)
        if spatial_algorithm not in _IP1:
            raise ValueError("OverIVA supports spatial_algorithm 'IP' / 'IP1', got {!r}.".format(
                spatial_algorithm))
        if n_sources is not None and int(n_sources) < 1:
            raise ValueError("n_sources must be positive, got {}.".format(n_sources))
        self.n_sources = None if n_sources is None else int(n_sources)
        self._n_sources_given = self.n_sources
        self.spatial_algorithm = spatial_algorithm
        self.flooring_fn = identity if flooring_fn is None else flooring_fn
        # (custom flooring callables: NotImplementedError here, never a silently unfloored run)
        device_flooring(self.flooring_fn, what="OverIVA")
        self.input = None
        if type(scale_restoration) is str and scale_restoration in _MDP:
            raise NotImplementedError(
                "OverIVA restores the scale by projection back only: the minimal distortion "
                "principle re-fits a square filter")
        if type(scale_restoration) is str and scale_restoration not in _PROJECTION_BACK:
            raise ValueError("{} is not supported for scale restoration.".format(scale_restoration))
        self.scale_restoration = scale_restoration
        if reference_id is None and scale_restoration:
            raise ValueError("Specify 'reference_id' if scale_restoration=True.")
        self.reference_id = reference_id

    def __repr__(self) -> str:
        s = "{}(n_sources={}, spatial_algorithm={}, scale_restoration={}, record_loss={}".format(
            type(self).__name__, self._n_sources_given, self.spatial_algorithm,
            self.scale_restoration, self.record_loss)
        if self.scale_restoration:
            s += ", reference_id={}".format(self.reference_id)
        return s + ")"

    # -- the call --------------------------------------------------------------------------------
    def __call__(self, input, n_iter: int = 100, initial_call: bool = True, **kwargs):
        """Separate a frequency-domain multichannel mixture into ``n_sources`` estimates,
        (n_sources, n_bins, n_frames)."""
        if input.ndim not in (3, 4):
            raise ValueError("input must be (n_channels, n_bins, n_frames) or (n_mixtures, "
                             "n_channels, n_bins, n_frames), got shape {}".format(tuple(input.shape)))
        M = int(input.shape[-3])
        check_shape(M, M if self._n_sources_given is None else self._n_sources_given)
        self._bind_input(input)
        self._reset(**kwargs)
        n_iter = int(n_iter)
        if not (self._unobserved_loss(n_iter) and self._resident_loop(n_iter, initial_call)):
            IterativeMethodBase.__call__(self, n_iter=n_iter, initial_call=initial_call)
        return self._finish_call()

    def _reset(self, **kwargs) -> None:
        assert self._has_input(), "Specify data!"
        for key, value in kwargs.items():
            setattr(self, key, value)
        B, M, F, T = self._X.shape
        N = M if self._n_sources_given is None else self._n_sources_given
        check_shape(M, N)
        self.n_sources, self.n_channels = N, M
        self.n_bins, self.n_frames = F, T
        if not self._state_has("demix_filter"):
            self.demix_filter = np.tile(np.eye(N, M, dtype=np.complex128), self._lead() + (F, 1, 1))
        elif self._state_is_none("demix_filter"):
            raise ValueError("demix_filter=None cannot be given at reset.")
        else:
            self.demix_filter = np.array(self.demix_filter, dtype=np.complex128, copy=True)
        if tuple(self.demix_filter.shape) != self._lead() + (F, N, M):
            raise ValueError("demix_filter must be {}, got {}".format(
                self._lead() + (F, N, M), tuple(self.demix_filter.shape)))
        self._floor = device_flooring(self.flooring_fn, what="OverIVA")
        if self._contrast == _lib.CONTRAST_GAUSS:
            self.variance = np.ones(self._lead() + (N, T))
        self._import_filter()
        Y = dv.empty((B, N, F, T), dv.c128, self._X.device)
        _ops.overiva_frame_power(self._X, self._W_full, N, Y=Y)
        self._state_set_dev("output", Y)

    def _import_filter(self) -> None:
        """The full filter [W_t ; [J, -I]] from the ``demix_filter`` state, J formed on the device."""
        B, M, F, _ = self._X.shape
        N = self.n_sources
        Wt = self._state_dev("demix_filter")
        W = dv.zeros((B, F, M, M), dv.c128, self._X.device)
        W[:, :, :N, :].copy_(Wt)  # (data movement only)
        _ops.overiva_step(W, None, self._C(), N, self._floor, self._info_tensor())
        self._W_full = W
        self._filter_rev = self._state_rev("demix_filter")

    def _full_filter(self):
        """The full filter the kernels work on; rebuilt when ``demix_filter`` was assigned since."""
        if self._state_rev("demix_filter") != self._filter_rev:
            self._import_filter()
        return self._W_full

    def _filter_updated(self) -> None:
        """A kernel rewrote the full filter: ``demix_filter`` is its first rows, copied when read."""
        self._state_defer("demix_filter", self._fill_demix_filter)
        self._filter_rev = self._state_rev("demix_filter")

    def _fill_demix_filter(self) -> None:
        ent = self._state()["demix_filter"]
        rows = self._W_full[:, :, :self.n_sources, :]
        if ent["dev"] is None:
            ent["dev"] = rows.contiguous()
        else:
            ent["dev"].copy_(rows)

    @property
    def background_filter(self):
        """J, (n_bins, n_channels - n_sources, n_sources): read-only, a host copy."""
        W = self._full_filter()
        self._check_device_errors()
        J = dv.to_host(W[:, :, self.n_sources:, :self.n_sources].contiguous())
        return J if self._batched else J[0]

    def _variance_tensor(self):
        return self._state_dev("variance") if self._contrast == _lib.CONTRAST_GAUSS else None

    # -- iterations ------------------------------------------------------------------------------
    def _step(self, W, floor, data_out=None, logdet_out=None, trace_out=None) -> None:
        """One iteration on the full filter; with the three outputs (each (B,)) also the loss terms
        of the state it starts from, taken from the frame powers and the filter it reads anyway."""
        N, var = self.n_sources, self._variance_tensor()
        r2 = _ops.overiva_frame_power(self._X, W, N)
        if data_out is not None:
            _ops.iva_loss_data(r2, var, self.n_bins, self._contrast, out=data_out)
        weight = _ops.iva_weight(r2, self.n_bins, self._contrast, floor, variance=var)
        V = _ops.weighted_covariance(self._X, weight, _lib.WEIGHT_FRAME, N)
        _ops.overiva_step(W, V, self._C(), N, floor, self._info_tensor(), logdet_out, trace_out)

    def _terms(self, W, data_out, logdet_out, trace_out) -> None:
        """The three loss terms of the current state."""
        r2 = _ops.overiva_frame_power(self._X, W, self.n_sources)
        _ops.iva_loss_data(r2, self._variance_tensor(), self.n_bins, self._contrast, out=data_out)
        _ops.overiva_step(W, None, self._C(), self.n_sources, self._floor, self._info_tensor(),
                          logdet_out, trace_out)

    def _resident_loop(self, n_iter: int, initial_call: bool) -> bool:
        """All iterations enqueued, the loss terms of every state kept on the device and read once
        at the end (DeviceStateMixin._resident_loss).  False for subclasses that replace a step."""
        cls = type(self)
        if (cls.update_once is not OverIVABase.update_once
                or cls.compute_loss is not OverIVABase.compute_loss):
            return False
        B, dev = self._X.shape[0], self._X.device

        def prepare(data, logdet):
            W = self._full_filter()
            trace = dv.zeros((n_iter + 1, B), dv.f64, dev)

            def step(t, record):
                if record:
                    self._step(W, self._floor, data[t], logdet[t], trace[t])
                else:
                    self._step(W, self._floor)

            def end():
                self._terms(W, data[n_iter], logdet[n_iter], trace[n_iter])
                self._filter_updated()
                if self._contrast == _lib.CONTRAST_GAUSS:
                    self._state_touch("variance")
                return trace

            return step, end
        return self._resident_loss(n_iter, initial_call, prepare)

    def update_once(self, flooring_fn="self") -> None:
        floor = self._resolve_floor(flooring_fn)
        if getattr(floor, "host", None) is not None:
            raise NotImplementedError("OverIVA is built for identity / max_flooring / add_flooring")
        self._step(self._full_filter(), floor)
        self._filter_updated()
        if self._contrast == _lib.CONTRAST_GAUSS:
            self._state_touch("variance")

    def compute_loss(self) -> float:
        B, dev = self._X.shape[0], self._X.device
        data, logdet, trace = (dv.empty((B,), dv.f64, dev) for _ in range(3))
        self._terms(self._full_filter(), data, logdet, trace)
        return self._loss_entry(self._combine_loss(data, logdet, trace))

    # -- the tail of a call ----------------------------------------------------------------------
    def _finish_call(self):
        if self.scale_restoration:
            self.restore_scale()
        B, M, F, T = self._X.shape
        Y = dv.empty((B, self.n_sources, F, T), dv.c128, self._X.device)
        _ops.overiva_frame_power(self._X, self._full_filter(), self.n_sources, Y=Y)
        self._state_set_dev("output", Y)
        return self._final_output()

    def separate(self, input: np.ndarray, demix_filter: np.ndarray) -> np.ndarray:
        """y_ij = W_t,i x_ij; NumPy in, NumPy out.  demix_filter (..., n_bins, n_sources, n_channels)."""
        batched = input.ndim == 4
        X = dv.to_device(input if batched else input[None], dtype=np.complex128)
        W = dv.to_device(demix_filter if batched else demix_filter[None], dtype=np.complex128)
        B, M, F, T = X.shape
        N = W.shape[2]
        check_shape(M, N)
        Y = dv.empty((B, N, F, T), dv.c128, X.device)
        _ops.overiva_frame_power(X, W, N, Y=Y, packed=True)
        Y = dv.to_host(Y)
        return Y if batched else Y[0]

    def apply_projection_back(self) -> None:
        """Projection back on the full M x M filter (algorithm/projection_back.py:87-99 of the
        reference, on [W_t ; [J, -I]]): row n of W_t is scaled by (W^-1)[reference_id, n].  The
        background rows keep their form [J, -I]."""
        assert self.scale_restoration, "Set self.scale_restoration=True."
        W = self._full_filter()
        scaled = W.clone()
        _ops.projection_back_filter(scaled, self.reference_id, self._info_tensor())
        N = self.n_sources
        W[:, :, :N, :].copy_(scaled[:, :, :N, :])
        self._filter_updated()

    def apply_minimal_distortion_principle(self) -> None:
        raise NotImplementedError("OverIVA restores the scale by projection back only")


class OverLaplaceIVA(OverIVABase):
    """OverIVA with the spherical Laplace source model, G(r) = 2 r (weights of ``AuxLaplaceIVA``)."""

    _contrast = _lib.CONTRAST_LAPLACE


class OverGaussIVA(OverIVABase):
    """OverIVA with the time-varying Gauss source model, G = n_bins log(alpha) + r^2 / alpha, alpha
    refreshed from the estimate at every iteration (weights and variance of ``AuxGaussIVA``)."""

    _contrast = _lib.CONTRAST_GAUSS
