"""The convolutional beamformer (WPD) on MI355X: denoising and dereverberation by one filter.

Nakatani and Kinoshita, "A unified convolutional beamformer for simultaneous denoising and
dereverberation", IEEE SPL 26(6), 2019; Boeddeker, Nakatani, Kinoshita and Haeb-Umbach, "Jointly
optimal dereverberation and beamforming", ICASSP 2020, for the form that needs no steering vector.
Per (mixture, bin, source), with ``x_t`` the ``M`` channels of frame ``t``, ``K = taps >= 0``,
``D = delay >= 1`` and ``Lb = (K + 1) M``:

* the stacked vector ``xb_t`` in C^Lb: block 0 is ``x_t``, block ``j = 1..K`` is
  ``x_{t - D - (j - 1)}``, zero before the first frame;
* the filter ``wb`` in C^Lb and the output ``y_t = wb^H xb_t``; the start filter is ``e_ref``;
* once per call ``Phi_s = sum_t m_t x_t x_t^H / max(sum_t m_t, 1e-10)`` (``masked_covariance``);
* one iteration: ``lambda_t = floor(|y_t|^2)``,
  ``R = (1 / T) sum_t xb_t xb_t^H / lambda_t + diagonal_loading (tr R / Lb) I``, and
  - mask form: ``A = (R^-1)[:, :M] Phi_s`` through the Cholesky factor of ``R``,
    ``wb = A[:, ref] / Re tr(A[:M, :])``;
  - steering form (``steering_vector=`` given): ``vb = [v; 0]``, ``a = R^-1 vb``,
    ``wb = a conj(v_ref) / (vb^H a)``, so that ``wb^H vb = v_ref``;
  a denominator that is zero or not finite (an all-zero mask) gives ``wb = 0``; then the new ``y``.

The sources of a bin share nothing but the mixture, so a workgroup owns one (mixture, bin, source) and
keeps ``wb`` and ``R`` on chip (csrc/wpd.hip).  Without callbacks ``__call__`` runs all ``n_iter``
iterations in ONE launch (``ssspy_wpd_steps``) and fills the loss list afterwards; with callbacks, or
when ``update_once()`` is called by hand, the same kernel runs one iteration per launch
(``ssspy_wpd_step``).  There is no host path: a shape or a floor the kernel does not take raises
``NotImplementedError``.
"""

import functools
from typing import Callable, List, Optional, Union

import numpy as np

from .. import _device as dv
from .. import _lib, _ops
from ..bss._device_state import DeviceStateMixin, LossShares, Synced
from ..bss.base import IterativeMethodBase
from ..special.flooring import identity, max_flooring
from ..utils.flooring import device_flooring
from .mask import _device_input, _device_mask, _host_mask, _is_device_tensor

__all__ = ["WPD"]

EPS = 1e-6


class WPD(DeviceStateMixin, IterativeMethodBase):
    """Weighted power minimisation distortionless response convolutional beamformer.

    Args:
        taps: number of delayed blocks ``K >= 0`` behind the current frame (0: the variance-weighted
            MPDR beamformer); ``(taps + 1) * n_channels <= 64``.
        delay: prediction delay ``D >= 1`` in frames.
        reference_id: the channel the output is referred to; negative values count from the end.
        diagonal_loading: ``R += diagonal_loading (tr R / Lb) I``.
        flooring_fn: floor of the frame powers: ``None`` / ``identity``, ``max_flooring``,
            ``add_flooring`` or a ``functools.partial`` of those fixing ``eps``.
        callbacks: callable or list of callables ``f(method)``.
        record_loss: record ``compute_loss()`` before the first iteration and after each one.

    ``__call__(input, mask=None, n_iter=3, steering_vector=None)`` takes ``input``
    ``(n_channels, n_bins, n_frames)`` or a batch ``(n_mixtures, n_channels, n_bins, n_frames)`` and
    ``mask`` ``(n_sources, n_bins, n_frames)`` (with the same leading axis for a batch), 1..8 channels
    and 1..16 sources.  ``steering_vector`` ``(n_bins, n_sources, n_channels)`` (with the leading axis
    for a batch) chooses the steering form; the masks are then not needed and may be ``None``.  All
    are NumPy arrays (any real dtype of a mask is converted to float64 and checked to be finite and
    ``>= 0``) or all are tensors on the HIP device (complex128 / float64, NOT checked), and the output
    ``(n_sources, n_bins, n_frames)`` comes in the same container.

    After a call: ``output``, ``convolutional_filter`` ``(n_bins, n_sources, taps + 1, n_channels)``
    holding the conjugated entries of ``wb``, ``y = sum_{j, m} convolutional_filter[f, n, j, m]
    xb[j M + m]`` (given by keyword it is copied and used as the start filter),
    ``signal_covariance`` ``(n_bins, n_sources, n_channels, n_channels)`` (``None`` in the steering
    form), ``loss``, and ``apply(input)``.  An ``R`` with a Cholesky pivot that is not positive and
    finite (too few frames without loading) raises ``numpy.linalg.LinAlgError`` with the number of
    (mixture, bin, source) triples; those keep the filter the failing iteration started from and
    ``output`` stays finite.  An all-zero mask gives a zero filter and a zero output, and no error.
    """

    convolutional_filter = Synced(dv.c128)
    output = Synced(dv.c128)
    signal_covariance = Synced(dv.c128)

    def __init__(
        self,
        taps: int = 5,
        delay: int = 3,
        reference_id: int = 0,
        diagonal_loading: float = 1e-6,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        record_loss: bool = True,
    ) -> None:
        super().__init__(callbacks=callbacks, record_loss=record_loss)
        self.taps, self.delay = self._checked_taps_delay(taps, delay)
        if isinstance(reference_id, bool) or int(reference_id) != reference_id:
            raise ValueError("reference_id must be an integer, got {!r}.".format(reference_id))
        self.reference_id = int(reference_id)
        self.diagonal_loading = self._checked_loading(diagonal_loading)
        self.flooring_fn = identity if flooring_fn is None else flooring_fn
        device_flooring(self.flooring_fn, what="WPD")  # (a floor the kernel cannot apply: now)
        self.input = None

    def __repr__(self) -> str:
        s = ("WPD(taps={taps}, delay={delay}, reference_id={reference_id}, "
             "diagonal_loading={diagonal_loading}, record_loss={record_loss})")
        return s.format(**self.__dict__)

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

    def _reference(self, n_channels: int) -> int:
        ref = self.reference_id
        if not -n_channels <= ref < n_channels:
            raise ValueError(
                "reference_id {} is out of range for {} channels.".format(ref, n_channels))
        return ref % n_channels

    def _check_shapes(self, input_shape, mask_shape, steering_shape) -> None:
        """Ranks, matching axes and the limits of the kernel; nothing is uploaded before this passes."""
        input_shape = tuple(input_shape)
        if len(input_shape) not in (3, 4):
            raise ValueError(
                "input must be (n_channels, n_bins, n_frames) or (n_mixtures, n_channels, n_bins, "
                "n_frames), got shape {}".format(input_shape))
        if min(input_shape) < 1:
            raise ValueError("input has an empty axis: shape {}".format(input_shape))
        lead, (M, F, T) = input_shape[:-3], input_shape[-3:]
        n_sources = None
        if mask_shape is not None:
            mask_shape = tuple(mask_shape)
            if len(mask_shape) != len(input_shape) or min(mask_shape) < 1 \
                    or mask_shape[:-3] != lead or mask_shape[-2:] != (F, T):
                raise ValueError(
                    "mask must be (n_sources, n_bins, n_frames), with the leading mixture axis of input "
                    "if it has one: input {} and mask {}".format(input_shape, mask_shape))
            n_sources = mask_shape[-3]
        if steering_shape is not None:
            steering_shape = tuple(steering_shape)
            if len(steering_shape) != len(input_shape) or min(steering_shape) < 1 \
                    or steering_shape[:-2] != lead + (F,) or steering_shape[-1] != M \
                    or n_sources not in (None, steering_shape[-2]):
                raise ValueError(
                    "steering_vector must be (n_bins, n_sources, n_channels), with the leading mixture "
                    "axis of input if it has one: input {}, mask {} and steering_vector {}".format(
                        input_shape, mask_shape, steering_shape))
            n_sources = steering_shape[-2]
        if M > _lib.WPD_MAX_CHANNELS:
            raise NotImplementedError(
                "WPD takes 1..{} channels, got {}.".format(_lib.WPD_MAX_CHANNELS, M))
        if (self.taps + 1) * M > _lib.WPD_MAX_ORDER:
            raise NotImplementedError(
                "WPD takes (taps + 1) * n_channels <= {}, got {} * {} = {}.".format(
                    _lib.WPD_MAX_ORDER, self.taps + 1, M, (self.taps + 1) * M))
        if n_sources > _lib.WPD_MAX_SOURCES:
            raise NotImplementedError(
                "WPD takes 1..{} sources, got {}.".format(_lib.WPD_MAX_SOURCES, n_sources))

    def __call__(self, input, mask=None, n_iter: int = 3, steering_vector=None,
                 initial_call: bool = True, **kwargs):
        self.taps, self.delay = self._checked_taps_delay(self.taps, self.delay)
        self.diagonal_loading = self._checked_loading(self.diagonal_loading)
        self._floor = device_flooring(self.flooring_fn, what="WPD")
        if mask is None and steering_vector is None:
            raise ValueError("WPD needs a mask or a steering_vector.")
        given = [v for v in (input, mask, steering_vector) if v is not None]
        tensors = [_is_device_tensor(v) for v in given]
        if any(tensors) and not all(tensors):
            raise ValueError("input, mask and steering_vector must all be NumPy arrays or all be "
                             "tensors on the HIP device.")
        is_tensor = tensors[0]
        self._check_shapes(input.shape, None if mask is None else mask.shape,
                           None if steering_vector is None else steering_vector.shape)
        self._ref = self._reference(input.shape[-3])
        if mask is not None and not is_tensor:
            mask = _host_mask(mask, "mask")
        self._bind_input(input)
        batched = self._batched
        # the steering form does not read the masks
        self._V = None if steering_vector is None else _device_input(steering_vector, batched)
        self._mask = None if self._V is not None else _device_mask(mask, "mask", batched, is_tensor)
        self.n_sources = (self._V.shape[2] if self._V is not None else self._mask.shape[1])
        self._reset(**kwargs)
        n_iter = int(n_iter)
        if not self._iterate_in_one_launch(n_iter, initial_call):
            IterativeMethodBase.__call__(self, n_iter=n_iter, initial_call=initial_call)
        out = self._state_dev("output")
        self._check_device_errors()  # the status word of the kernel, once per call
        if is_tensor:
            return out if batched else out[0]
        return self._final_output()

    def _reset(self, **kwargs) -> None:
        assert self._has_input(), "Specify data!"
        for key, value in kwargs.items():
            setattr(self, key, value)
        B, M, F, T = self._X.shape
        N, K = self.n_sources, self.taps
        self.n_channels, self.n_bins, self.n_frames = M, F, T
        shape = self._lead() + (F, N, K + 1, M)
        if not self._state_has("convolutional_filter") or "convolutional_filter" not in kwargs:
            start = dv.zeros((B, F, N, K + 1, M), dv.c128, self._X.device)
            start[:, :, :, 0, self._ref] = 1.0  # wb = e_ref
            self._state_set_dev("convolutional_filter", start)
        else:
            if self._state_is_none("convolutional_filter"):
                raise ValueError("convolutional_filter=None cannot be given at reset.")
            given = np.array(self.convolutional_filter, dtype=np.complex128, copy=True)
            if given.shape != shape:
                raise ValueError(
                    "convolutional_filter must be {}, got {}.".format(shape, given.shape))
            self.convolutional_filter = given  # (a copy: the filter given by keyword is kept)
        self._state_set_dev("output", dv.empty((B, N, F, T), dv.c128, self._X.device))
        self._state_defer("output", self._fill_output)
        if self._V is None:
            self._state_set_dev("signal_covariance", dv.zeros((B, F, N, M, M), dv.c128, self._X.device))
            self._state_defer("signal_covariance", self._fill_covariance)
        else:
            self.signal_covariance = None

    def _W(self):
        B, M, F, _ = self._X.shape
        return self._state_dev("convolutional_filter").reshape(
            B, F, self.n_sources, (self.taps + 1) * M)

    def _Phi(self):
        """The buffer the kernel leaves Phi_s in (mask form), or None."""
        if self._V is not None:
            return None
        ent = self._state()["signal_covariance"]
        ent.pop("lazy", None)  # (the launch rewrites all of it)
        ent["host"] = ent["host_rw"] = None
        return ent["dev"]

    def _fill_output(self) -> None:
        _ops.wpd_apply(self._X, self._W(), self.taps, self.delay, Y=self._state()["output"]["dev"])

    def _fill_covariance(self) -> None:
        self._state()["signal_covariance"]["dev"] = _ops.beamform_covariances(
            self._X, self._mask, normalize=True)[0]

    def _check_device_errors(self):
        _ops.check_workspace_canaries()  # no-op unless SSSPY_AMD_WS_CANARY is set
        info = self.__dict__.get("_info")
        if info is not None:
            failed = int(info[0].item())  # synchronises
            if failed:
                info.zero_()
                raise np.linalg.LinAlgError(
                    "WPD: R of {} (mixture, bin, source) triple(s) has a Cholesky pivot that is not "
                    "positive and finite; they keep the filter the iteration started from".format(
                        failed))

    # -- iterations ------------------------------------------------------------------------------
    def update_once(self) -> None:
        """One iteration in one launch: ``convolutional_filter`` and ``output`` are rewritten.  Raises
        ``numpy.linalg.LinAlgError`` at once if a pivot of this iteration failed."""
        ent = self._state()["output"]
        ent.pop("lazy", None)  # (the launch rewrites all of it)
        _ops.wpd_step(self._X, self._mask, self._V, self._W(), self.taps, self.delay, self._ref,
                      self.diagonal_loading, self._floor, self._info_tensor(), Y=ent["dev"],
                      Phi_s=self._Phi())
        self._state_touch("convolutional_filter")
        self._state_touch("output")
        # a failed triple would be counted again by the next launch: the status word is read after
        # every launch of this path, so the count in the LinAlgError is of distinct triples
        self._check_device_errors()

    def compute_loss(self):
        """(1 / T) sum_n sum_f sum_t [log lambda_nft + |y_nft|^2 / lambda_nft], lambda formed (and
        floored) from the current output; bins and sources are added in the order f N + n."""
        B, _, F, _ = self._X.shape
        rows = F * self.n_sources
        dev = self._X.device
        slots = dv.zeros((rows, B), dv.f64, dev)
        _ops.wpd_apply(self._X, self._W(), self.taps, self.delay, self._floor, loss_data=slots,
                       slot_stride=B, want_output=False)
        total = _ops.fold_scalar_slots(slots, B, rows, dv.empty((B,), dv.f64, dev))
        self._check_device_errors()
        return self._loss_entry(dv.to_host(total))

    def _iterate_in_one_launch(self, n_iter: int, initial_call: bool) -> bool:
        """All ``n_iter`` iterations in one launch when nothing can look in between: no callbacks and
        the methods this module defines.  With ``record_loss`` the per-(bin, source) terms of every
        state stay in HBM and are added in the order f N + n at the end.  False: one launch per
        iteration."""
        cls = type(self)
        stock = all(getattr(getattr(cls, name, None), "__module__", __name__) == __name__
                    for name in ("update_once", "compute_loss"))
        if self.callbacks or n_iter <= 0 or not stock:
            return False
        B, _, F, _ = self._X.shape
        rows = F * self.n_sources
        if self.record_loss and not LossShares.fit(rows, n_iter + 1, B):
            return False
        ent = self._state()["output"]
        ent.pop("lazy", None)
        slots, stride = None, 0
        if self.record_loss:
            stride = (n_iter + 1) * B
            slots = dv.zeros((rows, stride), dv.f64, self._X.device)
        _ops.wpd_steps(self._X, self._mask, self._V, self._W(), self.taps, self.delay, self._ref,
                       self.diagonal_loading, self._floor, n_iter, self._info_tensor(), Y=ent["dev"],
                       Phi_s=self._Phi(), loss_data=slots, slot_stride=stride)
        self._state_touch("convolutional_filter")
        self._state_touch("output")
        if self.record_loss:
            terms = _ops.fold_scalar_slots(slots, stride, rows,
                                           dv.empty((stride,), dv.f64, self._X.device))
            self._check_device_errors()
            values = dv.to_host(terms).reshape(n_iter + 1, B)
            self.loss.extend(self._loss_entry(v) for v in (values if initial_call else values[1:]))
        return True

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
        X = _device_input(input, self._batched)
        Y = _ops.wpd_apply(X, self._W(), self.taps, self.delay)
        Y = Y if self._batched else Y[0]
        return Y if _is_device_tensor(input) else dv.to_host(Y)
