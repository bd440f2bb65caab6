"""Dereverberation by weighted prediction error (WPE) on MI355X.

Nakatani, Yoshioka, Kinoshita, Miyoshi and Juang, "Speech dereverberation based on
variance-normalized delayed linear prediction", IEEE TASLP 18(7), 2010.  Per bin, with ``x_t`` the
``M`` channels of frame ``t``, ``K`` taps, delay ``D`` and ``L = K M``:

* the stacked history ``xs_t`` in C^L, entry ``k M + m`` equal to ``x[m, t - D - k]`` and zero
  before the first frame;
* the output ``y_t = x_t - G^H xs_t`` with the prediction filter ``G`` (L, M), zero at the start;
* one iteration: ``lambda_t = floor(mean_m |y_mt|^2)``, ``R = sum_t xs_t xs_t^H / lambda_t``,
  ``P = sum_t xs_t x_t^H / lambda_t``, ``G = R^-1 P`` by a Cholesky factorisation, the new ``y``.

The bins never talk to each other, so a workgroup owns one (mixture, bin) and keeps ``G``, ``R`` and
``P`` on chip (csrc/wpe.hip).  Without callbacks ``__call__`` runs all ``n_iter`` iterations in ONE
launch (``ssspy_wpe_steps``) and fills the loss list afterwards; with callbacks, or when
``update_once()`` is called by hand, the same kernel runs one iteration per launch
(``ssspy_wpe_step``) and ``prediction_filter`` and ``output`` exist in between.  There is no host
path: a shape or a floor the kernel does not take raises ``NotImplementedError``.
"""

import functools
from typing import Callable, List, Optional, Union

import numpy as np
import torch

from .. import _device as dv
from .. import _lib, _ops
from ..bss._device_state import DeviceStateMixin, LossShares, Synced
from ..bss.base import IterativeMethodBase
from ..special.flooring import identity, max_flooring
from ..utils.flooring import device_flooring

__all__ = ["WPE"]

EPS = 1e-10


class WPE(DeviceStateMixin, IterativeMethodBase):
    """Weighted prediction error dereverberation.

    Args:
        taps: number of prediction taps ``K >= 1``; ``taps * n_channels <= 64``.
        delay: prediction delay ``D >= 1`` in frames.
        flooring_fn: floor of the frame variances: ``None`` / ``identity``, ``max_flooring``,
            ``add_flooring`` or a ``functools.partial`` of those fixing ``eps``.
        callbacks: callable or list of callables ``f(method)``.
        record_loss: record ``compute_loss()`` before the first iteration and after each one.

    ``__call__(input, n_iter=3)`` takes ``(n_channels, n_bins, n_frames)`` or a batch
    ``(n_mixtures, n_channels, n_bins, n_frames)``, 1..8 channels, as a NumPy array or a complex128
    tensor on the HIP device, and returns the dereverberated spectrograms in the same kind of
    container.  ``prediction_filter`` is ``(n_bins, taps, n_channels, n_channels)`` (with a leading
    mixture axis for a batch), ``prediction_filter[f, k, m, :]`` being row ``k M + m`` of ``G``; given
    by keyword it is copied and used as the starting filter.  A singular or indefinite ``R``
    (``delay >= n_frames``, too few frames, a silent channel) raises ``numpy.linalg.LinAlgError``.
    """

    prediction_filter = Synced(dv.c128)
    output = Synced(dv.c128)

    def __init__(
        self,
        taps: int = 10,
        delay: int = 3,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        record_loss: bool = True,
    ) -> None:
        super().__init__(callbacks=callbacks, record_loss=record_loss)
        if int(taps) != taps or taps < 1:
            raise ValueError("taps must be a positive integer, got {!r}.".format(taps))
        if int(delay) != delay or delay < 1:
            raise ValueError("delay must be an integer >= 1, got {!r}.".format(delay))
        self.taps, self.delay = int(taps), int(delay)
        self.flooring_fn = identity if flooring_fn is None else flooring_fn
        device_flooring(self.flooring_fn, what="WPE")  # (a floor the kernel cannot apply: now)
        self.input = None

    def __repr__(self) -> str:
        s = "WPE(taps={taps}, delay={delay}, record_loss={record_loss})"
        return s.format(**self.__dict__)

    # -- limits ----------------------------------------------------------------------------------
    def _check_shape(self, shape) -> None:
        if len(shape) not in (3, 4):
            raise ValueError(
                "input must be (n_channels, n_bins, n_frames) or (n_mixtures, n_channels, n_bins, "
                "n_frames), got shape {}".format(tuple(shape)))
        M = shape[-3]
        if min(shape) < 1:
            raise ValueError("input has an empty axis: shape {}".format(tuple(shape)))
        if M > _lib.WPE_MAX_CHANNELS:
            raise NotImplementedError(
                "WPE takes 1..{} channels, got {}.".format(_lib.WPE_MAX_CHANNELS, M))
        if self.taps * M > _lib.WPE_MAX_ORDER:
            raise NotImplementedError(
                "WPE takes taps * n_channels <= {}, got {} * {} = {}.".format(
                    _lib.WPE_MAX_ORDER, self.taps, M, self.taps * M))

    def __call__(self, input, n_iter: int = 3, initial_call: bool = True, **kwargs):
        if int(self.taps) < 1:
            raise ValueError("taps must be a positive integer, got {!r}.".format(self.taps))
        if int(self.delay) < 1:
            raise ValueError("delay must be an integer >= 1, got {!r}.".format(self.delay))
        self._floor = device_flooring(self.flooring_fn, what="WPE")
        self._check_shape(tuple(input.shape))
        self._bind_input(input)
        self._reset(**kwargs)
        n_iter = int(n_iter)
        if not self._iterate_in_one_launch(n_iter, initial_call):
            IterativeMethodBase.__call__(self, n_iter=n_iter, initial_call=initial_call)
        out = self._state_dev("output")
        self._check_device_errors()  # the status word of the kernels, once per call
        if isinstance(input, torch.Tensor):
            return out if self._batched else out[0]
        return self._final_output()

    def _reset(self, **kwargs) -> None:
        assert self._has_input(), "Specify data!"
        for key, value in kwargs.items():
            setattr(self, key, value)
        B, M, F, T = self._X.shape
        self.n_channels, self.n_bins, self.n_frames = M, F, T
        shape = self._lead() + (F, self.taps, M, M)
        if not self._state_has("prediction_filter") or "prediction_filter" not in kwargs:
            self._state_set_dev("prediction_filter",
                                dv.zeros((B, F, self.taps, M, M), dv.c128, self._X.device))
        else:
            if self._state_is_none("prediction_filter"):
                raise ValueError("prediction_filter=None cannot be given at reset.")
            given = np.array(self.prediction_filter, dtype=np.complex128, copy=True)
            if given.shape != shape:
                raise ValueError("prediction_filter must be {}, got {}.".format(shape, given.shape))
            self.prediction_filter = given  # (a copy: the filter given by keyword is not overwritten)
        self._state_set_dev("output", dv.empty((B, M, F, T), dv.c128, self._X.device))
        self._state_defer("output", self._fill_output)

    def _G(self):
        B, M, F, _ = self._X.shape
        return self._state_dev("prediction_filter").reshape(B, F, self.taps * M, M)

    def _fill_output(self) -> None:
        _ops.wpe_apply(self._X, self._G(), self.taps, self.delay, Y=self._state()["output"]["dev"])

    # -- iterations ------------------------------------------------------------------------------
    def update_once(self) -> None:
        """One iteration in one launch: ``prediction_filter`` and ``output`` are rewritten."""
        ent = self._state()["output"]
        ent.pop("lazy", None)  # (the launch rewrites all of it)
        _ops.wpe_step(self._X, self._G(), self.taps, self.delay, self._floor, self._info_tensor(),
                      Y=ent["dev"])
        self._state_touch("prediction_filter")
        self._state_touch("output")

    def compute_loss(self):
        """(1 / T) sum_f sum_t [M log lambda_ft + sum_m |y_mft|^2 / lambda_ft], lambda formed (and
        floored) from the current output; the bins are added in bin order."""
        B, _, F, _ = self._X.shape
        dev = self._X.device
        slots = dv.zeros((F, B), dv.f64, dev)
        _ops.wpe_apply(self._X, self._G(), self.taps, self.delay, self._floor, loss_data=slots,
                       slot_stride=B, want_output=False)
        total = _ops.fold_scalar_slots(slots, B, F, dv.empty((B,), dv.f64, dev))
        self._check_device_errors()
        return self._loss_entry(dv.to_host(total))

    def _iterate_in_one_launch(self, n_iter: int, initial_call: bool) -> bool:
        """All ``n_iter`` iterations in one launch when nothing can look in between: no callbacks and
        the methods this module defines.  With ``record_loss`` the per-bin terms of every state stay
        in HBM and are added over the bins in bin order at the end.  False: one launch per iteration."""
        cls = type(self)
        stock = all(getattr(getattr(cls, name, None), "__module__", __name__) == __name__
                    for name in ("update_once", "compute_loss"))
        if self.callbacks or n_iter <= 0 or not stock:
            return False
        B, _, F, _ = self._X.shape
        if self.record_loss and not LossShares.fit(F, n_iter + 1, B):
            return False
        ent = self._state()["output"]
        ent.pop("lazy", None)
        slots, stride = None, 0
        if self.record_loss:
            stride = (n_iter + 1) * B
            slots = dv.zeros((F, stride), dv.f64, self._X.device)
        _ops.wpe_steps(self._X, self._G(), self.taps, self.delay, self._floor, n_iter,
                       self._info_tensor(), Y=ent["dev"], loss_data=slots, slot_stride=stride)
        self._state_touch("prediction_filter")
        self._state_touch("output")
        if self.record_loss:
            terms = _ops.fold_scalar_slots(slots, stride, F,
                                           dv.empty((stride,), dv.f64, self._X.device))
            self._check_device_errors()
            values = dv.to_host(terms).reshape(n_iter + 1, B)
            self.loss.extend(self._loss_entry(v) for v in (values if initial_call else values[1:]))
        return True
