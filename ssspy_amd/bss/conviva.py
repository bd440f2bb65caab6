"""IVA with joint dereverberation (convolutional AuxIVA) on MI355X: 2..8 channels.

T. Nakatani et al., "Computationally efficient and versatile framework for joint optimization of
blind speech separation and dereverberation", Interspeech 2020 (the source-wise factorisation);
R. Ikeshita, N. Ito, T. Nakatani, K. Kinoshita, "Independent low-rank matrix analysis with
decorrelation learning", WASPAA 2019.  The reference has no such class.  It is the blind counterpart
of ``beamform.WPD``: one filter per source over the current frame and ``taps`` delayed frames, a WPE
prediction filter and an IP1 demixing row optimised under one IVA objective.

Per mixture, with ``M`` channels, ``N = M`` sources, ``K = taps >= 0``, ``D = delay >= 1``,
``L = K M``, ``Lb = (K + 1) M`` and the stacked vector ``xb_t`` of WPD (block 0 is ``x_t``, block
``j = 1..K`` is ``x_{t - D - (j - 1)}``, zero before the first frame): the state is ``W``
``(F, N, Lb)``, ``y_nft = sum_l W[f, n, l] xb_ft[l]``, ``W[f, n, :M] = e_n`` first.  One iteration:

1. the frame powers ``r_nt^2 = sum_f |y_nft|^2`` and the weights ``phi_nt`` of ``AuxLaplaceIVA`` /
   ``AuxGaussIVA`` (the same kernels and flooring place; Gauss refreshes ``variance``);
2. per (bin, source) ``Rb = (1 / T) sum_t phi_nt xb_t xb_t^H``, ``C = Rb[:M, :M]``, ``P = Rb[M:, :M]``,
   ``R = Rb[M:, M:] + diagonal_loading (Re tr R / L) I``, ``G_n = R^-1 P`` by Cholesky and the Schur
   complement ``Sigma_n = C - P^H G_n`` (csrc/conviva.hip);
3. per bin the IP1 sweep (``update_by_ip1``) on ``Q = W[f, :, :M]`` with ``Sigma`` as the weighted
   covariances;
4. ``wb_n = [q_n; -G_n q_n]``, ``W[f, n, :] = conj(wb_n)``;
5. ``Y = W xb`` (``ssspy_wpd_apply``).

Loss: ``sum_n mean_t G(r_nt) - 2 sum_f log|det Q_f|``.  With ``diagonal_loading = 0`` the iteration
is a majorise-minimise scheme and the loss does not increase.  There is no host path.
"""

import functools
from typing import Callable, List, Optional, Union

import numpy as np

from .. import _device as dv
from .. import _lib, _ops
from ..special.flooring import identity, max_flooring
from ..utils.flooring import device_flooring
from ._device_state import Synced
from ._filter_base import _MDP, _PROJECTION_BACK, DemixingFilterBase
from .base import IterativeMethodBase

__all__ = ["ConvIVABase", "ConvLaplaceIVA", "ConvGaussIVA"]

EPS = 1e-10


def _is_device_tensor(value) -> bool:
    return type(value).__module__.split(".")[0] == "torch"


class ConvIVABase(DemixingFilterBase):
    """State and iteration of ConvIVA; the subclasses name the contrast.

    Args:
        taps: number of delayed blocks ``K >= 0`` behind the current frame (0: AuxIVA-IP1);
            ``(taps + 1) * n_channels <= 64``.
        delay: prediction delay ``D >= 1`` in frames.
        diagonal_loading: ``R += diagonal_loading (Re tr R / L) I``; 0 keeps the iteration monotone.
        flooring_fn: ``None`` / ``identity``, ``max_flooring``, ``add_flooring`` or a
            ``functools.partial`` of those fixing ``eps``.
        scale_restoration: ``True`` / ``"projection_back"`` or ``False``.

    Inputs are ``(n_channels, n_bins, n_frames)`` or a batch ``(n_mixtures, ...)``, NumPy or a
    complex128 tensor on the device; the output ``(n_sources, n_bins, n_frames)`` comes back in the
    same container.  After a call: ``output``, ``convolutional_filter`` ``(n_bins, n_sources,
    taps + 1, n_channels)`` in WPD's layout (given by keyword it is copied and used as the start
    state), ``demix_filter`` = ``convolutional_filter[:, :, 0, :]``, ``prediction_filter``
    ``(n_bins, n_sources, taps, n_channels, n_channels)`` in WPE's layout per source (what the last
    iteration formed; read-only), ``loss`` and ``apply(input)``.  An ``R`` with a Cholesky pivot that
    is not positive and finite raises ``numpy.linalg.LinAlgError`` with the number of (mixture, bin,
    source) triples; those keep their filter row and ``output`` stays finite.
    """

    _contrast = None  # SSSPY_CONTRAST_* of the subclass
    convolutional_filter = Synced(dv.c128)
    variance = Synced(dv.f64)

    def __init__(
        self,
        taps: int = 5,
        delay: int = 3,
        diagonal_loading: float = 0.0,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(callbacks=callbacks, record_loss=record_loss)
        self.taps, self.delay = self._checked_taps_delay(taps, delay)
        self.diagonal_loading = self._checked_loading(diagonal_loading)
        self.flooring_fn = identity if flooring_fn is None else flooring_fn
        # (custom flooring callables: NotImplementedError here, never a silently unfloored run)
        device_flooring(self.flooring_fn, what="ConvIVA")
        self.input = None
        if type(scale_restoration) is str and scale_restoration in _MDP:
            raise NotImplementedError(
                "ConvIVA restores the scale by projection back only: the minimal distortion "
                "principle re-fits an instantaneous filter")
        if type(scale_restoration) is str and scale_restoration not in _PROJECTION_BACK:
            raise ValueError("{} is not supported for scale restoration.".format(scale_restoration))
        self.scale_restoration = scale_restoration
        if reference_id is None and scale_restoration:
            raise ValueError("Specify 'reference_id' if scale_restoration=True.")
        if reference_id is not None and (isinstance(reference_id, bool)
                                         or int(reference_id) != reference_id):
            raise ValueError("reference_id must be an integer, got {!r}.".format(reference_id))
        self.reference_id = reference_id

    def __repr__(self) -> str:
        s = ("{}(taps={}, delay={}, diagonal_loading={}, scale_restoration={}, record_loss={}"
             .format(type(self).__name__, self.taps, self.delay, self.diagonal_loading,
                     self.scale_restoration, self.record_loss))
        if self.scale_restoration:
            s += ", reference_id={}".format(self.reference_id)
        return s + ")"

    # -- the host contract -----------------------------------------------------------------------
    @staticmethod
    def _checked_taps_delay(taps, delay):
        if isinstance(taps, bool) or int(taps) != taps or taps < 0:
            raise ValueError("taps must be an integer >= 0, got {!r}.".format(taps))
        if isinstance(delay, bool) or int(delay) != delay or delay < 1:
            raise ValueError("delay must be an integer >= 1, got {!r}.".format(delay))
        return int(taps), int(delay)

    @staticmethod
    def _checked_loading(diagonal_loading):
        loading = float(diagonal_loading)
        if not (0.0 <= loading < float("inf")):
            raise ValueError(
                "diagonal_loading must be finite and >= 0, got {!r}.".format(diagonal_loading))
        return loading

    def _check_shape(self, shape) -> None:
        """Rank, empty axes and the limits of the kernel; nothing is uploaded before this passes."""
        shape = tuple(shape)
        if len(shape) not in (3, 4):
            raise ValueError(
                "input must be (n_channels, n_bins, n_frames) or (n_mixtures, n_channels, n_bins, "
                "n_frames), got shape {}".format(shape))
        if min(shape) < 1:
            raise ValueError("input has an empty axis: shape {}".format(shape))
        M = shape[-3]
        if not _lib.CONVIVA_MIN_CHANNELS <= M <= _lib.CONVIVA_MAX_CHANNELS:
            raise NotImplementedError("ConvIVA takes {}..{} channels, got {}.".format(
                _lib.CONVIVA_MIN_CHANNELS, _lib.CONVIVA_MAX_CHANNELS, M))
        if (self.taps + 1) * M > _lib.CONVIVA_MAX_ORDER:
            raise NotImplementedError(
                "ConvIVA takes (taps + 1) * n_channels <= {}, got {} * {} = {}.".format(
                    _lib.CONVIVA_MAX_ORDER, self.taps + 1, M, (self.taps + 1) * M))
        ref = self.reference_id
        if self.scale_restoration and not 0 <= ref < M:
            raise ValueError("reference_id {} is out of range for {} channels.".format(ref, M))

    # -- the call --------------------------------------------------------------------------------
    def __call__(self, input, n_iter: int = 100, initial_call: bool = True, **kwargs):
        """Separate and dereverberate a frequency-domain multichannel mixture:
        (n_sources, n_bins, n_frames) in the container of ``input``."""
        self.taps, self.delay = self._checked_taps_delay(self.taps, self.delay)
        self.diagonal_loading = self._checked_loading(self.diagonal_loading)
        self._floor = device_flooring(self.flooring_fn, what="ConvIVA")
        self._check_shape(input.shape)
        is_tensor = _is_device_tensor(input)
        self._bind_input(input)
        self._reset(**kwargs)
        n_iter = int(n_iter)
        if not (self._unobserved_loss(n_iter) and self._resident_loop(n_iter, initial_call)):
            IterativeMethodBase.__call__(self, n_iter=n_iter, initial_call=initial_call)
        if self.scale_restoration:
            self.restore_scale()
        out = self._current_output()
        self._check_device_errors()  # the status words of the kernels, once per call
        if is_tensor:
            return out if self._batched else out[0]
        return self._final_output()

    def _reset(self, **kwargs) -> None:
        assert self._has_input(), "Specify data!"
        for key, value in kwargs.items():
            setattr(self, key, value)
        B, M, F, T = self._X.shape
        K = self.taps
        dev = self._X.device
        self.n_sources = self.n_channels = M
        self.n_bins, self.n_frames = F, T
        self._floor = device_flooring(self.flooring_fn, what="ConvIVA")
        shape = self._lead() + (F, M, K + 1, M)
        if not self._state_has("convolutional_filter") or "convolutional_filter" not in kwargs:
            start = dv.zeros((B, F, M, K + 1, M), dv.c128, dev)
            start[:, :, :, 0, :] = dv.eye_filters(B, F, M, dev)  # W[f, n, :M] = e_n
            self._state_set_dev("convolutional_filter", start)
        else:
            if self._state_is_none("convolutional_filter"):
                raise ValueError("convolutional_filter=None cannot be given at reset.")
            given = np.array(self.convolutional_filter, dtype=np.complex128, copy=True)
            if given.shape != shape:
                raise ValueError(
                    "convolutional_filter must be {}, got {}.".format(shape, given.shape))
            self.convolutional_filter = given  # (a copy: the filter given by keyword is kept)
        if self._contrast == _lib.CONTRAST_GAUSS:
            self.variance = np.ones(self._lead() + (M, T))
        # what an iteration hands from one kernel to the next, kept for the call.  Sigma starts as
        # the identity: a triple that fails before it was ever written leaves IP1 a regular matrix
        self._Sigma = dv.eye_filters(B, F * M, M, dev).reshape(B, F, M, M, M)
        self._G = dv.zeros((B, F, M, K * M, M), dv.c128, dev)
        self._failed = dv.zeros((B, F, M), dv.i32, dev)
        self._conv_info = dv.zeros((1,), dv.i32, dev)
        self._state_set_dev("output", dv.empty((B, M, F, T), dv.c128, dev))
        self._form_output()

    def _W(self):
        B, M, F, _ = self._X.shape
        return self._state_dev("convolutional_filter").reshape(B, F, M, (self.taps + 1) * M)

    def _form_output(self) -> None:
        """Y = W xb into the ``output`` buffer."""
        ent = self._state()["output"]
        ent.pop("lazy", None)
        _ops.wpd_apply(self._X, self._W(), self.taps, self.delay, Y=ent["dev"])
        self._state_touch("output")
        self._output_rev = (self._state_rev("convolutional_filter"), self._state_rev("output"))

    def _current_output(self):
        """The ``output`` buffer, formed again when the filters or it were assigned since."""
        if self._output_rev != (self._state_rev("convolutional_filter"),
                                self._state_rev("output")):
            self._form_output()
        return self._state_dev("output")

    @property
    def demix_filter(self):
        """``convolutional_filter[:, :, 0, :]``, (n_bins, n_sources, n_channels): a host copy."""
        return np.array(self.convolutional_filter[..., 0, :])

    @property
    def prediction_filter(self):
        """G of the last iteration, (n_bins, n_sources, taps, n_channels, n_channels): the WPE filter
        of every source in WPE's layout, y_n = q_n^H (x - G_n^H xs).  Read-only, a host copy; zeros
        before the first iteration of a call."""
        B, M, F, _ = self._X.shape
        self._check_device_errors()
        G = dv.to_host(self._G).reshape(B, F, M, self.taps, M, M)
        return G if self._batched else G[0]

    def _variance_tensor(self):
        return self._state_dev("variance") if self._contrast == _lib.CONTRAST_GAUSS else None

    def _check_device_errors(self):
        info = self.__dict__.get("_conv_info")
        if info is not None:
            failed = int(info[0].item())  # synchronises
            if failed:
                info.zero_()
                raise np.linalg.LinAlgError(
                    "ConvIVA: R of {} of {} (mixture, bin, source) triple(s) has a Cholesky pivot "
                    "that is not positive and finite; they keep the filter row the iteration "
                    "started from".format(failed, self._failed.numel()))
        super()._check_device_errors()

    # -- iterations ------------------------------------------------------------------------------
    def _step(self, floor, data_out=None, logdet_out=None) -> None:
        """One iteration; with the two outputs (each (B,)) also the loss terms of the state it
        starts from, taken from the frame powers and the demixing rows it reads anyway."""
        M, K = self.n_channels, self.taps
        var = self._variance_tensor()
        W = self._W()
        r2 = _ops.iva_frame_power(self._current_output(), None)
        Q = W[..., :M].clone()  # (data movement only; a copy also with taps = 0)
        if data_out is not None:
            _ops.iva_loss_data(r2, var, self.n_bins, self._contrast, out=data_out)
            _ops.sum_logdet(Q, out=logdet_out)
        phi = _ops.iva_weight(r2, self.n_bins, self._contrast, floor, variance=var)
        _ops.conviva_statistics(self._X, phi, K, self.delay, self.diagonal_loading, self._conv_info,
                                Sigma=self._Sigma, G=self._G, failed=self._failed)
        _ops.update_by_ip1(Q, self._Sigma, floor, self._info_tensor())
        _ops.conviva_compose(Q, self._G, W, K, self._failed)
        self._state_touch("convolutional_filter")
        if var is not None:
            self._state_touch("variance")
        self._form_output()

    def _terms(self, data_out, logdet_out) -> None:
        """The two loss terms of the current state."""
        r2 = _ops.iva_frame_power(self._current_output(), None)
        _ops.iva_loss_data(r2, self._variance_tensor(), self.n_bins, self._contrast, out=data_out)
        Q = self._W()[..., :self.n_channels].contiguous()
        _ops.sum_logdet(Q, out=logdet_out)

    def _resident_loop(self, n_iter: int, initial_call: bool) -> bool:
        """All iterations enqueued, the loss terms of every state kept on the device and read once
        at the end (DeviceStateMixin._resident_loss).  False for subclasses that replace a step."""
        cls = type(self)
        if (cls.update_once is not ConvIVABase.update_once
                or cls.compute_loss is not ConvIVABase.compute_loss):
            return False

        def prepare(data, logdet):
            def step(t, record):
                if record:
                    self._step(self._floor, data[t], logdet[t])
                else:
                    self._step(self._floor)

            def end():
                self._terms(data[n_iter], logdet[n_iter])

            return step, end
        return self._resident_loss(n_iter, initial_call, prepare)

    def update_once(self, flooring_fn="self") -> None:
        floor = self._resolve_floor(flooring_fn)
        if getattr(floor, "host", None) is not None:
            raise NotImplementedError("ConvIVA is built for identity / max_flooring / add_flooring")
        self._step(floor)

    def compute_loss(self) -> float:
        B, dev = self._X.shape[0], self._X.device
        data, logdet = (dv.empty((B,), dv.f64, dev) for _ in range(2))
        self._terms(data, logdet)
        return self._host_loss(data, logdet)

    # -- the tail of a call ----------------------------------------------------------------------
    def apply_projection_back(self) -> None:
        """Projection back on the demixing rows Q (algorithm/projection_back.py:87-99 of the
        reference): row n is scaled by (Q^-1)[reference_id, n], and the convolutional filters are
        composed again from the scaled rows and the kept G."""
        assert self.scale_restoration, "Set self.scale_restoration=True."
        W = self._W()
        Q = W[..., :self.n_channels].clone()
        _ops.projection_back_filter(Q, self.reference_id, self._info_tensor())
        _ops.conviva_compose(Q, self._G, W, self.taps, self._failed)
        self._state_touch("convolutional_filter")

    def apply_minimal_distortion_principle(self) -> None:
        raise NotImplementedError("ConvIVA restores the scale by projection back only")

    def apply(self, input):
        """The stored ``convolutional_filter`` on another spectrogram of the same
        ``(n_channels, n_bins)``: ``(n_sources, n_bins, n_frames')`` in the container of ``input``."""
        if not self._state_has("convolutional_filter") or not self._has_input():
            raise ValueError("apply() needs the filters of a call.")
        shape = tuple(input.shape)
        lead = self._lead()
        if len(shape) != len(lead) + 3 or shape[:-1] != lead + (self.n_channels, self.n_bins) \
                or shape[-1] < 1:
            raise ValueError("input must be {}, got {}.".format(
                lead + (self.n_channels, self.n_bins, "n_frames"), shape))
        if _is_device_tensor(input):
            if not input.is_cuda or input.dtype != dv.c128:
                raise ValueError("a tensor input must be complex128 on the HIP device")
            X = (input if self._batched else input[None]).contiguous()
        else:
            arr = np.asarray(input)
            X = dv.to_device(arr if self._batched else arr[None], dtype=np.complex128)
        Y = _ops.wpd_apply(X, self._W(), self.taps, self.delay)
        Y = Y if self._batched else Y[0]
        return Y if _is_device_tensor(input) else dv.to_host(Y)

    def separate(self, input, demix_filter):
        raise NotImplementedError("ConvIVA applies convolutional filters: use apply(input)")


class ConvLaplaceIVA(ConvIVABase):
    """ConvIVA with the spherical Laplace source model, G(r) = 2 r (weights of ``AuxLaplaceIVA``)."""

    _contrast = _lib.CONTRAST_LAPLACE


class ConvGaussIVA(ConvIVABase):
    """ConvIVA with the time-varying Gauss source model, G = n_bins log(alpha) + r^2 / alpha, alpha
    refreshed from the estimate at every iteration (weights and variance of ``AuxGaussIVA``)."""

    _contrast = _lib.CONTRAST_GAUSS
