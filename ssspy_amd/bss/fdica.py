"""Frequency-domain independent component analysis (FDICA) on MI355X.

Drop-in separator classes for the reference's ``ssspy.bss.fdica`` (ssspy/bss/fdica.py): ``FDICABase``,
``GradFDICABase``, ``GradFDICA``, ``NaturalGradFDICA``, ``AuxFDICA`` (``IP`` / ``IP1`` / ``IP2``) and
the three classes with the Laplace model, ``GradLaplaceFDICA``, ``NaturalGradLaplaceFDICA`` and
``AuxLaplaceFDICA``.

The bins of FDICA never talk to each other, so the iterations of one (mixture, bin) are a closed
problem on its slab of the mixture.  Two paths:

* the bin-resident kernel (csrc/fdica.hip, ``ssspy_fdica_steps``): a workgroup owns one
  (mixture, bin) and runs whole iterations on chip.  Without callbacks ``__call__`` runs all
  ``n_iter`` iterations in ONE launch and fills the loss list afterwards; with callbacks, or when
  ``update_once()`` is called by hand, the same kernel runs one step per launch.  2..4 sources (at
  5..8 it is measured slower than the operators below, profiles/fdica.txt), the three Laplace
  classes with gradient, natural gradient or IP1, a floor the kernels can apply.
* the composed path, correct everywhere (2..16 sources, IP2, user closures, arbitrary flooring
  callables): separate -> weight (``ssspy_fdica_weight``) -> weighted covariance -> IP1 / IP2 /
  gradient step, the operators the other separators use.

``ssspy_fdica_route`` decides between them, once.  User closures follow the compatibility path of
``GradIVABase``: ``score_fn`` sees the whole estimate on the host, ``d_contrast_fn`` sees ``|Y|`` on the
host and the weights go back up, ``contrast_fn`` runs on the host only when the loss is recorded.
Permutation alignment runs on the device, once per call (csrc/permutation.hip: 2..8 sources, the
built-in floors; route ``device_alignment``), and on the host beyond that.
"""

import functools
from typing import Callable, Iterable, List, Optional, Tuple, Union

import numpy as np

from .. import _device as dv
from .. import _lib, _ops, _routes
from ..algorithm.permutation_alignment import (
    correlation_based_permutation_solver,
    device_correlation_permutation,
)
from ..special.flooring import identity, max_flooring
from ..utils.flooring import choose_flooring_fn, device_flooring, host_floor
from ..utils.select_pair import resolve_pairs, sequential_pair_selector
from ._device_state import LossShares
from ._filter_base import _IP1, _IP2, DemixingFilterBase
from .base import IterativeMethodBase

__all__ = [
    "FDICABase",
    "GradFDICABase",
    "GradFDICA",
    "NaturalGradFDICA",
    "AuxFDICA",
    "GradLaplaceFDICA",
    "NaturalGradLaplaceFDICA",
    "AuxLaplaceFDICA",
]

spatial_algorithms = ["IP", "IP1", "IP2"]
EPS = 1e-10
_LAPLACE = "laplace"


def _own_model(method, names):
    """The built-in source model the separator's callables stand for, or None for user closures.
    The named classes tag the closures they build with the model and with the instance they belong
    to: closures borrowed from another instance read that instance's floor, so they count as user
    closures and take the compatibility path."""
    fns = [getattr(method, name, None) for name in names]
    tags = [(getattr(fn, "_ssspy_amd_contrast", None), getattr(fn, "_ssspy_amd_owner", None))
            for fn in fns]
    if tags[0][0] is None or any(t[0] != tags[0][0] or t[1] is not method for t in tags):
        return None
    return tags[0][0]


class FDICABase(DemixingFilterBase):
    """ref: ssspy/bss/fdica.py:32-326."""

    _model_callables = ("contrast_fn",)
    _stock_methods = ("update_once", "compute_loss", "separate")

    def __init__(
        self,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        permutation_alignment: bool = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(callbacks=callbacks, record_loss=record_loss)
        if contrast_fn is None:
            raise ValueError("Specify contrast function.")
        self.contrast_fn = contrast_fn
        self.flooring_fn = identity if flooring_fn is None else flooring_fn
        self.input = None
        self.permutation_alignment = permutation_alignment
        self.scale_restoration = scale_restoration
        if reference_id is None and scale_restoration:
            raise ValueError("Specify 'reference_id' if scale_restoration=True.")
        self.reference_id = reference_id

    def __call__(
        self, input: np.ndarray, n_iter: int = 100, initial_call: bool = True, **kwargs
    ) -> np.ndarray:
        """ref: ssspy/bss/fdica.py:100-126 (the base class does not know how to finish)."""
        self._bind_input(input)
        self._reset(**kwargs)
        IterativeMethodBase.__call__(self, n_iter=n_iter, initial_call=initial_call)
        raise NotImplementedError("Implement '__call__' method.")

    def _run(self, input, n_iter, initial_call, kwargs):
        """``__call__`` of the classes that have an update: iterations, permutation, scale, output
        (ref: ssspy/bss/fdica.py:422-437, :1003-1022)."""
        self._bind_input(input)
        self._reset(**kwargs)
        if not self._iterate_in_one_launch(int(n_iter), initial_call):
            IterativeMethodBase.__call__(self, n_iter=n_iter, initial_call=initial_call)
        if self.permutation_alignment:
            self.solve_permutation()
        return self._finish_call()

    def __repr__(self) -> str:
        s = "FDICA("
        s += ", permutation_alignment={permutation_alignment}"
        s += ", scale_restoration={scale_restoration}"
        s += ", record_loss={record_loss}"
        if self.scale_restoration:
            s += ", reference_id={reference_id}"
        s += ")"
        return s.format(**self.__dict__)

    def _reset(self, **kwargs) -> None:
        """ref: ssspy/bss/fdica.py:141-172."""
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
        self._floor = device_flooring(self.flooring_fn, allow_host=True)
        self._model = _own_model(self, self._model_callables)

    def separate(self, input: np.ndarray, demix_filter: np.ndarray) -> np.ndarray:
        """y_ij = W_i x_ij (ref: ssspy/bss/fdica.py:174-197); NumPy in, NumPy out."""
        batched = input.ndim == 4
        X = dv.to_device(input if batched else input[None], dtype=np.complex128)
        W = dv.to_device(demix_filter if batched else demix_filter[None], dtype=np.complex128)
        Y = dv.to_host(_ops.separate(X, W))
        return Y if batched else Y[0]

    # -- the loss ------------------------------------------------------------------------------
    def compute_loss(self) -> float:
        """sum_i (mean_j sum_n G(y_ijn) - 2 log|det W_i|) (ref: ssspy/bss/fdica.py:199-223)."""
        W = self._state_dev("demix_filter")
        logdet = _ops.sum_logdet(W)
        Y = _ops.separate(self._X, W)
        if self._model == _LAPLACE:
            B, _, F, _ = Y.shape
            slots = dv.empty((F, B), dv.f64, Y.device)
            _ops.fdica_weight(Y, False, device_flooring(identity), contrast=slots, contrast_stride=B,
                              want_weight=False)
            data = _ops.fold_scalar_slots(slots, B, F, dv.empty((B,), dv.f64, Y.device))
            return self._host_loss(data, logdet)
        self._check_device_errors()
        values = np.array([np.sum(np.mean(self.contrast_fn(Yb), axis=2)) for Yb in dv.to_host(Y)])
        return self._loss_entry(values - 2.0 * dv.to_host(logdet))

    def compute_logdet(self, demix_filter: np.ndarray) -> np.ndarray:
        """log|det W_i| per bin (ref: ssspy/bss/fdica.py:225-237)."""
        _, logdet = np.linalg.slogdet(demix_filter)
        return logdet

    # -- permutation alignment (once per call) ---------------------------------------------------
    def solve_permutation(self) -> None:
        """ref: ssspy/bss/fdica.py:239-255."""
        permutation_alignment = self.permutation_alignment
        assert permutation_alignment, "Set permutation_alignment=True."
        if type(permutation_alignment) is bool:
            permutation_alignment = "spectrogram_correlation"
        if permutation_alignment == "spectrogram_correlation":
            self.solve_permutation_by_correlation()
        else:
            raise NotImplementedError(
                "permutation_alignment {} is not implemented.".format(permutation_alignment)
            )

    def solve_permutation_by_correlation(self, flooring_fn="self") -> None:
        """Align the rows of the filters over the bins by the correlation of the amplitude envelopes
        (ref: ssspy/bss/fdica.py:257-281).  On the device where ``ssspy_permutation_route`` allows:
        only the per-bin overlaps come to the host, to be sorted, and the rows of the filters are
        gathered in place of a round trip.  Otherwise (route ``device_alignment`` off, more than 8
        sources, a flooring callable) the estimate and the filters come to the host once and the
        aligned filters go back up.  ``output`` follows the filters when it is read."""
        if flooring_fn is not None:  # (None: the identity, as the solver itself takes it)
            flooring_fn = choose_flooring_fn(flooring_fn, method=self)
        Wd = self._state_dev("demix_filter")
        Yd = _ops.separate(self._X, Wd)
        self._check_device_errors()
        floor = device_flooring(flooring_fn, allow_host=True)
        if _routes.get("device_alignment") and _ops.permutation_route(
                Yd.shape[1], Yd.shape[3], _lib.PERM_SOLVER_CORRELATION, floor):
            perm = device_correlation_permutation(Yd, floor)
            self._state_set_dev("demix_filter",
                                _ops.permute_sources(Wd, perm, _lib.PERM_LAYOUT_BIN_SOURCE))
            self._filters_stepped()
            return
        Y, W = dv.to_host(Yd), np.array(dv.to_host(Wd))
        for b in range(Y.shape[0]):
            Yb = np.array(Y[b].transpose(1, 0, 2))  # (n_bins, n_sources, n_frames)
            correlation_based_permutation_solver(Yb, W[b], flooring_fn=flooring_fn)
        self._state_set_dev("demix_filter", dv.to_device(W, dtype=np.complex128, dev=Wd.device))
        self._filters_stepped()

    # -- the state behind a step -----------------------------------------------------------------
    def _fill_output(self) -> None:
        ent = self._state()["output"]
        if ent["dev"] is None:
            ent["dev"] = dv.empty(tuple(self._X.shape), dv.c128, self._X.device)
        _ops.separate(self._X, self._state_dev("demix_filter"), out=ent["dev"])

    def _filters_stepped(self) -> None:
        """Behind a step: the filters moved, ``output`` follows them when it is read."""
        self._state_touch("demix_filter")
        self._state_defer("output", self._fill_output)

    # -- the bin-resident kernel -----------------------------------------------------------------
    def _algorithm(self):
        """The _lib.FDICA_* this configuration runs, or None when only closures know."""
        return None

    def _kernel_route(self, floor=None):
        """The _lib.FDICA_ROUTE_* of this call: RESIDENT or STREAMING when ssspy_fdica_steps runs it,
        COMPOSED for the per-iteration operators."""
        floor = self._floor if floor is None else floor
        algorithm = self._algorithm()
        if (algorithm is None or self._model != _LAPLACE or host_floor(floor) is not None
                or not _routes.get("fdica_kernel")):
            return _lib.FDICA_ROUTE_COMPOSED
        B, N, F, T = self._X.shape
        return _ops.fdica_route(B, N, F, T, algorithm)

    def _kernel_steps(self, n_steps, floor, loss_data=None, logdet=None, slot_stride=0) -> None:
        _ops.fdica_steps(self._X, self._state_dev("demix_filter"), self._algorithm(),
                         getattr(self, "is_holonomic", False), getattr(self, "step_size", 0.0),
                         floor, n_steps, self._info_tensor(), loss_data, logdet, slot_stride)
        self._filters_stepped()

    def _iterate_in_one_launch(self, n_iter: int, initial_call: bool) -> bool:
        """All ``n_iter`` iterations in one launch when nothing can look in between: no callbacks,
        the methods this module defines, the Laplace model of the instance itself and a floor the
        kernels apply.  With ``record_loss`` the per-bin terms of every state stay in HBM and are
        added over the bins in bin order at the end.  False: the reference's loop."""
        cls = type(self)
        stock = all(getattr(getattr(cls, name, None), "__module__", __name__) == __name__
                    for name in self._stock_methods)
        if self.callbacks or n_iter <= 0 or not stock:
            return False
        if self._kernel_route() == _lib.FDICA_ROUTE_COMPOSED:
            return False
        if not self.record_loss:
            self._kernel_steps(n_iter, self._floor)
            return True
        B, F, dev = self._X.shape[0], self.n_bins, self._X.device
        if not LossShares.fit(2 * F, n_iter + 1, B):
            return False
        stride = (n_iter + 1) * B
        slots = dv.empty((2, F, stride), dv.f64, dev)
        self._kernel_steps(n_iter, self._floor, slots[0], slots[1], stride)
        terms = dv.empty((2, n_iter + 1, B), dv.f64, dev)
        for k in range(2):
            _ops.fold_scalar_slots(slots[k], stride, F, terms[k].reshape(-1))
        values = self._combine_loss(terms[0], terms[1])
        self.loss.extend(self._loss_entry(v) for v in (values if initial_call else values[1:]))
        return True

    # -- the composed path -----------------------------------------------------------------------
    def _laplace_weight(self, Y, aux_form, floor):
        """Weights (B, S, F, T) of the Laplace model on the estimate (or a pair of its rows)."""
        host = host_floor(floor)
        if host is None:
            return _ops.fdica_weight(Y, aux_form, floor)
        # a flooring callable the kernels cannot run: on the host, on the array the reference
        # applies it to (|y|, resp. 2 |y|; ssspy/bss/fdica.py:1110, :1354)
        self._check_device_errors()
        scale = 2.0 if aux_form else 1.0
        weight = np.stack([scale / np.asarray(host(scale * np.abs(Yb)), dtype=np.float64)
                           for Yb in dv.to_host(Y)])
        return dv.to_device(weight, dtype=np.float64, dev=Y.device)


class GradFDICABase(FDICABase):
    """FDICA by (natural) gradient descent (ref: ssspy/bss/fdica.py:329-455)."""

    _natural = False
    _model_callables = ("contrast_fn", "score_fn")

    def __init__(
        self,
        step_size: float = 1e-1,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        score_fn: Callable[[np.ndarray], np.ndarray] = None,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        permutation_alignment: bool = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(
            contrast_fn=contrast_fn,
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            permutation_alignment=permutation_alignment,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        self.step_size = step_size
        if score_fn is None:
            raise ValueError("Specify score function.")
        self.score_fn = score_fn

    def __call__(
        self, input: np.ndarray, n_iter: int = 100, initial_call: bool = True, **kwargs
    ) -> np.ndarray:
        """Separate a frequency-domain multichannel mixture (ref: ssspy/bss/fdica.py:402-437)."""
        return self._run(input, n_iter, initial_call, kwargs)

    def __repr__(self) -> str:
        s = "GradFDICA("
        s += "step_size={step_size}"
        s += ", permutation_alignment={permutation_alignment}"
        s += ", scale_restoration={scale_restoration}"
        s += ", record_loss={record_loss}"
        if self.scale_restoration:
            s += ", reference_id={reference_id}"
        s += ")"
        return s.format(**self.__dict__)

    def _repr_with_holonomic(self, name) -> str:
        s = name + "("
        s += "step_size={step_size}"
        s += ", is_holonomic={is_holonomic}"
        s += ", permutation_alignment={permutation_alignment}"
        s += ", scale_restoration={scale_restoration}"
        s += ", record_loss={record_loss}"
        if self.scale_restoration:
            s += ", reference_id={reference_id}"
        s += ")"
        return s.format(**self.__dict__)

    def update_once(self) -> None:
        raise NotImplementedError("Implement 'update_once' method.")

    def _algorithm(self):
        if not hasattr(self, "is_holonomic"):
            return None
        return _lib.FDICA_NATURAL_GRAD if self._natural else _lib.FDICA_GRAD

    def _update_once(self) -> None:
        """One (natural) gradient step (ref: ssspy/bss/fdica.py:629-650, :824-843)."""
        if self._kernel_route() != _lib.FDICA_ROUTE_COMPOSED:
            self._kernel_steps(1, self._floor)
            return
        W = self._state_dev("demix_filter")
        Y = _ops.separate(self._X, W)
        if self._model == _LAPLACE:
            # phi(y) = weight * y with one real weight per (source, bin, frame): row n of
            # mean_j phi(y) y^H is (W U_n W^H)[n, :] with the weighted covariances of the mixture
            weight = self._laplace_weight(Y, False, self._floor)
            stats = _ops.weighted_covariance(self._X, weight, _lib.WEIGHT_BIN_FRAME, self.n_sources)
        else:
            self._check_device_errors()
            Phi = np.stack([np.asarray(self.score_fn(Yb), dtype=np.complex128)
                            for Yb in dv.to_host(Y)])
            if Phi.shape != tuple(Y.shape):
                raise ValueError("score_fn must map (n_sources, n_bins, n_frames) to the same shape.")
            stats = _ops.cross_covariance(dv.to_device(Phi, dtype=np.complex128, dev=Y.device), Y)
        _ops.iva_grad_step(W, stats, self._natural, self.is_holonomic, self.step_size,
                           self._info_tensor())
        self._filters_stepped()


class GradFDICA(GradFDICABase):
    """FDICA by gradient descent, W <- W - eta D W^-H (ref: ssspy/bss/fdica.py:458-650).

    With ``contrast_fn`` / ``score_fn`` closures this is the compatibility path (see the module)."""

    def __init__(
        self,
        step_size: float = 1e-1,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        score_fn: Callable[[np.ndarray], np.ndarray] = None,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        is_holonomic: bool = False,
        permutation_alignment: bool = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(
            step_size=step_size,
            contrast_fn=contrast_fn,
            score_fn=score_fn,
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            permutation_alignment=permutation_alignment,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        self.is_holonomic = is_holonomic

    def __repr__(self) -> str:
        return self._repr_with_holonomic("GradFDICA")

    def update_once(self) -> None:
        """ref: ssspy/bss/fdica.py:598-650."""
        self._update_once()


class NaturalGradFDICA(GradFDICABase):
    """FDICA by natural gradient descent, W <- W - eta D W (ref: ssspy/bss/fdica.py:653-843).

    With ``contrast_fn`` / ``score_fn`` closures this is the compatibility path (see the module)."""

    _natural = True

    def __init__(
        self,
        step_size: float = 1e-1,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        score_fn: Callable[[np.ndarray], np.ndarray] = None,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        is_holonomic: bool = False,
        permutation_alignment: bool = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(
            step_size=step_size,
            contrast_fn=contrast_fn,
            score_fn=score_fn,
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            permutation_alignment=permutation_alignment,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        self.is_holonomic = is_holonomic

    def __repr__(self) -> str:
        return self._repr_with_holonomic("NaturalGradFDICA")

    def update_once(self) -> None:
        """ref: ssspy/bss/fdica.py:793-843."""
        self._update_once()


class AuxFDICA(FDICABase):
    """Auxiliary-function-based FDICA (ref: ssspy/bss/fdica.py:846-1245)."""

    _model_callables = ("contrast_fn", "d_contrast_fn")
    _stock_methods = FDICABase._stock_methods + ("update_once_ip1", "update_once_ip2")

    def __init__(
        self,
        spatial_algorithm: str = "IP",
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        d_contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        pair_selector: Optional[Callable[[int], Iterable[Tuple[int, int]]]] = None,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        permutation_alignment: bool = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(
            contrast_fn=contrast_fn,
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            permutation_alignment=permutation_alignment,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        assert spatial_algorithm in spatial_algorithms, "Not support {}.".format(spatial_algorithms)
        self.spatial_algorithm = spatial_algorithm
        self.d_contrast_fn = d_contrast_fn
        if pair_selector is None:
            if spatial_algorithm == "IP2":
                self.pair_selector = sequential_pair_selector
        else:
            self.pair_selector = pair_selector

    def __call__(
        self, input: np.ndarray, n_iter: int = 100, initial_call: bool = True, **kwargs
    ) -> np.ndarray:
        """Separate a frequency-domain multichannel mixture (ref: ssspy/bss/fdica.py:983-1022)."""
        return self._run(input, n_iter, initial_call, kwargs)

    def __repr__(self) -> str:
        return self._repr_named("AuxFDICA")

    def _repr_named(self, name) -> str:
        s = name + "("
        s += "spatial_algorithm={spatial_algorithm}"
        s += ", permutation_alignment={permutation_alignment}"
        s += ", scale_restoration={scale_restoration}"
        s += ", record_loss={record_loss}"
        if self.scale_restoration:
            s += ", reference_id={reference_id}"
        s += ")"
        return s.format(**self.__dict__)

    def _reset(self, **kwargs) -> None:
        super()._reset(**kwargs)
        if self._model is None and self.d_contrast_fn is None:
            raise ValueError("Specify d_contrast_fn.")

    def _algorithm(self):
        if self.spatial_algorithm in _IP1:
            return _lib.FDICA_AUX_IP1
        return _lib.FDICA_AUX_IP2

    def update_once(self, flooring_fn="self") -> None:
        """ref: ssspy/bss/fdica.py:1038-1063."""
        if self.spatial_algorithm in _IP1:
            self.update_once_ip1(flooring_fn=flooring_fn)
        elif self.spatial_algorithm in _IP2:
            self.update_once_ip2(flooring_fn=flooring_fn)
        else:
            raise NotImplementedError("Not support {}.".format(self.spatial_algorithm))

    def _aux_weight(self, Y, floor):
        """varphi = G'(|y|) / floor(2 |y|) on the estimate or a pair of its rows
        (ref: ssspy/bss/fdica.py:1109-1112, :1231-1234)."""
        if self._model == _LAPLACE:
            return self._laplace_weight(Y, True, floor)
        # user closures: |Y| comes to the host, the weights go back up
        self._check_device_errors()
        host = host_floor(floor)
        if host is None:
            kind, eps = floor
            host = {_lib.FLOOR_NONE: lambda x: x, _lib.FLOOR_MAX: lambda x: np.maximum(x, eps),
                    _lib.FLOOR_ADD: lambda x: x + eps}[kind]
        weight = []
        for Yb in dv.to_host(Y):
            Y_abs = np.abs(Yb)
            weight.append(np.asarray(self.d_contrast_fn(Y_abs), dtype=np.float64)
                          / np.asarray(host(2 * Y_abs), dtype=np.float64))
        return dv.to_device(np.stack(weight), dtype=np.float64, dev=Y.device)

    def update_once_ip1(self, flooring_fn="self") -> None:
        """One iterative-projection sweep (ref: ssspy/bss/fdica.py:1065-1116)."""
        floor = self._resolve_floor(flooring_fn)
        if self.spatial_algorithm in _IP1 and self._kernel_route(floor) != _lib.FDICA_ROUTE_COMPOSED:
            self._kernel_steps(1, floor)
            return
        W = self._state_dev("demix_filter")
        weight = self._aux_weight(_ops.separate(self._X, W), floor)
        U = _ops.weighted_covariance(self._X, weight, _lib.WEIGHT_BIN_FRAME, self.n_sources)
        _ops.update_by_ip1(W, U, floor, self._info_tensor())
        self._filters_stepped()

    def update_once_ip2(self, flooring_fn="self") -> None:
        """One pairwise sweep: per pair the two rows are separated with the CURRENT filters, their
        weights and two covariances formed, and the pair updated (ref: ssspy/bss/fdica.py:1118-1245)."""
        floor = self._resolve_floor(flooring_fn)
        W = self._state_dev("demix_filter")
        for pair in resolve_pairs(getattr(self, "pair_selector", None), self.n_sources):
            rows = _ops.separate(self._X, W)[:, list(pair)].contiguous()  # (B, 2, F, T)
            weight = self._aux_weight(rows, floor)
            U = _ops.weighted_covariance(self._X, weight, _lib.WEIGHT_BIN_FRAME, 2)
            _ops.update_by_ip2(W, U, [pair], floor, self._info_tensor(), pair_only=True)
        self._filters_stepped()


def _laplace_closures(method, aux):
    """The Laplace model: G = 2 |y|, phi = y / floor(|y|), G' = 2
    (ref: ssspy/bss/fdica.py:1332-1355, :1618-1640)."""
    def contrast_fn(y: np.ndarray) -> np.ndarray:
        return 2 * np.abs(y)

    def score_fn(y: np.ndarray) -> np.ndarray:
        denom = method.flooring_fn(np.abs(y))
        return y / denom

    def d_contrast_fn(y: np.ndarray) -> np.ndarray:
        return 2 * np.ones_like(y)

    other = d_contrast_fn if aux else score_fn
    contrast_fn._ssspy_amd_contrast = other._ssspy_amd_contrast = _LAPLACE
    contrast_fn._ssspy_amd_owner = other._ssspy_amd_owner = method
    return contrast_fn, other


class GradLaplaceFDICA(GradFDICA):
    """Gradient FDICA with the Laplace model (ref: ssspy/bss/fdica.py:1248-1383)."""

    def __init__(
        self,
        step_size: float = 1e-1,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        is_holonomic: bool = False,
        permutation_alignment: bool = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        contrast_fn, score_fn = _laplace_closures(self, aux=False)
        super().__init__(
            step_size=step_size,
            contrast_fn=contrast_fn,
            score_fn=score_fn,
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            is_holonomic=is_holonomic,
            permutation_alignment=permutation_alignment,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )

    def __repr__(self) -> str:
        return self._repr_with_holonomic("GradLaplaceFDICA")


class NaturalGradLaplaceFDICA(NaturalGradFDICA):
    """Natural-gradient FDICA with the Laplace model (ref: ssspy/bss/fdica.py:1386-1524)."""

    def __init__(
        self,
        step_size: float = 1e-1,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        is_holonomic: bool = False,
        permutation_alignment: bool = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        contrast_fn, score_fn = _laplace_closures(self, aux=False)
        super().__init__(
            step_size=step_size,
            contrast_fn=contrast_fn,
            score_fn=score_fn,
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            is_holonomic=is_holonomic,
            permutation_alignment=permutation_alignment,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )

    def __repr__(self) -> str:
        return self._repr_with_holonomic("NaturalGradLaplaceFDICA")


class AuxLaplaceFDICA(AuxFDICA):
    """Auxiliary-function-based FDICA with the Laplace model (ref: ssspy/bss/fdica.py:1527-1667)."""

    def __init__(
        self,
        spatial_algorithm: str = "IP",
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        pair_selector: Optional[Callable[[int], Iterable[Tuple[int, int]]]] = None,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        permutation_alignment: bool = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        contrast_fn, d_contrast_fn = _laplace_closures(self, aux=True)
        super().__init__(
            spatial_algorithm=spatial_algorithm,
            contrast_fn=contrast_fn,
            d_contrast_fn=d_contrast_fn,
            flooring_fn=flooring_fn,
            pair_selector=pair_selector,
            callbacks=callbacks,
            permutation_alignment=permutation_alignment,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )

    def __repr__(self) -> str:
        return self._repr_named("AuxLaplaceFDICA")
