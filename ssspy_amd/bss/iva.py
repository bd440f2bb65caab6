"""Independent vector analysis (IVA) on MI355X: the auxiliary-function and the gradient families.

Drop-in separator classes for the ``AuxIVA`` family of the reference's ``ssspy.bss.iva``
(ssspy/bss/iva.py:553-641, :1403-2214, :2976-3473): ``AuxIVA``, ``AuxLaplaceIVA`` and
``AuxGaussIVA`` with every ``spatial_algorithm`` of the reference.  The contrast
functions of the reference are Python closures; the kernels implement the two the
reference ships (Laplace: G = 2r; time-varying Gauss: G = F log(alpha) + r^2/alpha).  A
user-supplied ``d_contrast_fn`` is evaluated on the host on the (n_sources, n_frames) frame norms
the device produces (a few KB per iteration; both passes over the spectrogram stay in the kernels);
a user-supplied ``contrast_fn`` takes the whole estimate and is evaluated on a host copy of it,
only when the loss is recorded.

The gradient family (ssspy/bss/iva.py:284-406, :644-988, :2341-2973): ``GradIVA``,
``NaturalGradIVA`` and the four classes with a built-in source model, ``GradLaplaceIVA``,
``GradGaussIVA``, ``NaturalGradLaplaceIVA`` and ``NaturalGradGaussIVA``.  The score of the four is
one real weight per (source, frame) times the estimate, so an iteration is the two read-only passes
over the mixture of AuxIVA-IP1 and a per-bin step (csrc/grad_iva.hip); the two generic classes
take Python closures on the whole estimate and run a compatibility path (see ``GradIVABase``).

The fixed-point family (ssspy/bss/iva.py:409-550, :991-1400): ``FastIVA`` and ``FasterIVA`` on the
whitened mixture with unitary filters (csrc/fast_iva.hip, see ``FastIVABase``).

The proximal front ends (ssspy/bss/iva.py:2217-2338): ``PDSIVA`` and ``ADMMIVA``, thin subclasses of
``PDSBSS`` and ``ADMMBSS`` whose default penalty is ``prox.l21`` over the bins, in the form the
kernels of those classes apply themselves.
"""

import functools
from typing import Callable, Iterable, List, Optional, Tuple, Union

import numpy as np

from .. import _device as dv
from .. import _lib, _ops
from ..linalg import prox
from ..special.flooring import identity, max_flooring
from ..utils.flooring import choose_flooring_fn, device_flooring, host_floor, require_device_floor
from ..utils.select_pair import resolve_pairs, sequential_pair_selector
from ._device_state import LossShares, Synced
from ._filter_base import _IP1, _IP2, _IPA, _ISS1, _ISS2, DemixingFilterBase, filter_logdet
from .admmbss import ADMMBSS
from .base import IterativeMethodBase
from .pdsbss import PDSBSS

__all__ = [
    "GradIVABase",
    "FastIVABase",
    "GradIVA",
    "NaturalGradIVA",
    "FastIVA",
    "FasterIVA",
    "AuxIVA",
    "PDSIVA",
    "ADMMIVA",
    "GradLaplaceIVA",
    "GradGaussIVA",
    "NaturalGradLaplaceIVA",
    "NaturalGradGaussIVA",
    "AuxLaplaceIVA",
    "AuxGaussIVA",
]

spatial_algorithms = ["IP", "IP1", "IP2", "ISS", "ISS1", "ISS2", "IPA"]
EPS = 1e-10


class IVABase(DemixingFilterBase):
    """ref: ssspy/bss/iva.py:48-281."""

    def __init__(
        self,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks=None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(callbacks=callbacks, record_loss=record_loss)
        self.flooring_fn = identity if flooring_fn is None else flooring_fn
        self.input = None
        self.scale_restoration = scale_restoration
        if reference_id is None and scale_restoration:
            raise ValueError("Specify 'reference_id' if scale_restoration=True.")
        self.reference_id = reference_id

    def _reset(self, **kwargs) -> None:
        """ref: ssspy/bss/iva.py:138-169."""
        assert self._has_input(), "Specify data!"
        for key, value in kwargs.items():
            setattr(self, key, value)
        B, N, F, T = self._X.shape
        self.n_sources, self.n_channels = N, N
        self.n_bins, self.n_frames = F, T
        if not self._state_has("demix_filter"):
            self.demix_filter = np.tile(np.eye(N, dtype=np.complex128), self._lead() + (F, 1, 1))
        elif not self._state_is_none("demix_filter"):
            self.demix_filter = np.array(self.demix_filter, dtype=np.complex128, copy=True)
        if self._state_is_none("demix_filter"):
            raise ValueError("demix_filter=None cannot be given at reset.")
        self._state_set_dev("output", _ops.separate(self._X, self._state_dev("demix_filter")))
        self._floor = device_flooring(self.flooring_fn, allow_host=True)

    def separate(self, input: np.ndarray, demix_filter: np.ndarray) -> np.ndarray:
        """y_ij = W_i x_ij (ref: ssspy/bss/iva.py:171-194); NumPy in, NumPy out."""
        batched = input.ndim == 4
        X = dv.to_device(input if batched else input[None], dtype=np.complex128)
        W = dv.to_device(demix_filter if batched else demix_filter[None], dtype=np.complex128)
        Y = dv.to_host(_ops.separate(X, W))
        return Y if batched else Y[0]

    def compute_logdet(self, demix_filter: np.ndarray) -> np.ndarray:
        """log|det W_i| per bin (ref: ssspy/bss/iva.py:224-236): NumPy on the host, a complex128
        device tensor on the device (see ``filter_logdet``)."""
        return filter_logdet(demix_filter)


class AuxIVABase(IVABase):
    """ref: ssspy/bss/iva.py:553-641."""

    def __init__(
        self,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        d_contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks=None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        self.contrast_fn = contrast_fn
        self.d_contrast_fn = d_contrast_fn


def _device_contrast(contrast_fn, d_contrast_fn):
    """Which built-in contrast the pair of callables stands for (tag set by the subclasses), or
    None for user closures.  A closure cannot run inside a kernel, and it does not have to: the
    reference applies ``d_contrast_fn`` to the (n_sources, n_frames) frame norms only
    (ssspy/bss/iva.py:1787-1789), a few KB that the frame-power kernel produces -- the closure runs
    on the host on that array between the two passes over the spectrogram, which stay on the device."""
    a = getattr(contrast_fn, "_ssspy_amd_contrast", None)
    b = getattr(d_contrast_fn, "_ssspy_amd_contrast", None)
    if a is None or a != b:
        if d_contrast_fn is None:
            raise ValueError("Specify d_contrast_fn (and contrast_fn when record_loss=True).")
        return None
    return a


class AuxIVA(AuxIVABase):
    """Auxiliary-function-based IVA (ref: ssspy/bss/iva.py:1403-2214)."""

    _ipa_default_kwargs = {"lqpqm_normalization": True, "newton_iter": 1}
    _default_kwargs = _ipa_default_kwargs

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
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
        **kwargs,
    ) -> None:
        super().__init__(
            contrast_fn=contrast_fn,
            d_contrast_fn=d_contrast_fn,
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        assert spatial_algorithm in spatial_algorithms, "Not support {}.".format(spatial_algorithm)
        self.spatial_algorithm = spatial_algorithm
        if pair_selector is None:
            if spatial_algorithm in ["IP2", "ISS2"]:
                self.pair_selector = sequential_pair_selector
        else:
            self.pair_selector = pair_selector
        valid_keys = set(self._ipa_default_kwargs) if spatial_algorithm == "IPA" else set()
        invalid_keys = set(kwargs) - valid_keys
        assert invalid_keys == set(), "Invalid keywords {} are given.".format(invalid_keys)
        for key, value in kwargs.items():
            setattr(self, key, value)
        for key in valid_keys:
            if not hasattr(self, key):
                setattr(self, key, self._default_kwargs[key])
        device_flooring(self.flooring_fn, allow_host=True)

    def __call__(
        self, input: np.ndarray, n_iter: int = 100, initial_call: bool = True, **kwargs
    ) -> np.ndarray:
        """Separate a frequency-domain multichannel mixture (ref: ssspy/bss/iva.py:1637-1672)."""
        self._contrast = _device_contrast(self.contrast_fn, self.d_contrast_fn)
        self._bind_input(input)
        self._reset(**kwargs)
        if not self._iterate_with_resident_loss(int(n_iter), initial_call):
            IterativeMethodBase.__call__(self, n_iter=n_iter, initial_call=initial_call)
        return self._finish_call()

    def _iterate_with_resident_loss(self, n_iter: int, initial_call: bool) -> bool:
        """IP1 with ``record_loss=True`` (the reference's default) at the cost of ``record_loss=False``.

        ``compute_loss()`` needs the frame powers of the current estimate -- a pass over the mixture
        -- and so does the next ``update_once()``: here the loss of the state after iteration t is
        taken from the frame powers iteration t + 1 forms anyway (_resident_loss).  Only when
        nothing can look at ``self.loss`` in between (no callbacks, stock methods, a contrast that
        runs on the device and keeps no variance state); else the plain step of
        _iterate_with_resident_terms, if that applies, or (returns False) the reference's loop.
        ref: ssspy/bss/base.py:68-77, ssspy/bss/iva.py:200-222, :1736-1793."""
        cls = type(self)
        B, N = self._X.shape[0], self.n_sources
        # (round 6) sum_i log|det W_i| of the state an update starts from is a by-product of that
        # update: one share per 16-bin tile from the latency form of IP1 for a handful of mixtures
        # (the one-block sum_logdet launch was 13 us of a 65 us iteration), else the finished sum;
        # folded once at the end, only the last state needs sum_logdet
        nld = _ops.update_by_ip1_logdet_slots(B, self.n_bins, N)
        if not (self._unobserved_loss(n_iter)
                and self.spatial_algorithm in _IP1 and self._contrast is not None
                and host_floor(self._floor) is None
                and self._variance_tensor() is None
                and cls.update_once is AuxIVA.update_once
                and cls.update_once_ip1 is AuxIVA.update_once_ip1
                and cls.compute_loss is AuxIVA.compute_loss
                and LossShares.fit(nld, n_iter + 1, B)):
            # the same for every other spatial algorithm (round 6): one mixture of configs[2]
            # (ISS, 8 sources) spent 0.9-1.2 ms of wall time per 0.2 ms iteration waiting for the
            # loss; the fused ISS sweep's frame powers and tracked log-determinant serve as they come
            return (self._unobserved_loss(n_iter) and self._contrast is not None
                    and cls.update_once in (AuxIVA.update_once, AuxGaussIVA.update_once)
                    and cls.compute_loss is AuxIVA.compute_loss
                    and self._iterate_with_resident_terms(n_iter, initial_call))

        def prepare(data, logdet):
            W = self._state_dev("demix_filter")
            floor = self._resolve_floor("self")
            ld = LossShares(nld, n_iter + 1, B, self._X.device, logdet)

            def step(t, record):
                r2 = _ops.iva_frame_power(self._X, W)
                if record:
                    _ops.iva_loss_data(r2, None, self.n_bins, self._contrast, out=data[t])
                weight = _ops.iva_weight(r2, self.n_bins, self._contrast, floor, variance=None)
                U = _ops.weighted_covariance(self._X, weight, _lib.WEIGHT_FRAME, N)
                _ops.update_by_ip1_logdet(W, U, floor, self._info_tensor(), ld.at(t), ld.stride)

            def end():
                _ops.iva_loss_data(_ops.iva_frame_power(self._X, W), None, self.n_bins,
                                   self._contrast, out=data[n_iter])
                ld.fold()
                _ops.sum_logdet(W, out=logdet[n_iter])
                self._state_touch("demix_filter")

            return step, end
        return self._resident_loss(n_iter, initial_call, prepare)

    def __repr__(self) -> str:
        s = "AuxIVA(spatial_algorithm={}, scale_restoration={}, record_loss={}".format(
            self.spatial_algorithm, self.scale_restoration, self.record_loss
        )
        if self.scale_restoration:
            s += ", reference_id={}".format(self.reference_id)
        return s + ")"

    def _reset(self, **kwargs) -> None:
        """ref: ssspy/bss/iva.py:1687-1697."""
        super()._reset(**kwargs)
        # (also here, not only in __call__: update_once() after a manual _bind_input() / _reset() --
        #  the benchmarks do that, and the reference allows it -- must find the contrast code)
        self._contrast = _device_contrast(self.contrast_fn, self.d_contrast_fn)
        self._reset_output_state()
        # frame powers of the output (ISS state) as (tensor, revision of `output` they describe): any
        # later write to the output -- a kernel, scale restoration, an assignment by a callback --
        # changes the revision and retires the cache
        self._r2_cache = None

    def _implied_route_wanted(self) -> bool:
        return self.spatial_algorithm in _ISS2 + _IPA

    def _variance_tensor(self):
        return None

    def _weights(self, flooring_fn):
        """Auxiliary weights varphi_nj = G'(r_nj) / floor(2 r_nj), (B, N, T)."""
        return self._weights_from_power(self._frame_power(), self._contrast, flooring_fn)

    def _weights_from_power(self, r2, contrast, flooring_fn):
        floor = self._resolve_floor(flooring_fn)
        if contrast is None or host_floor(floor) is not None:
            # a user closure, or a flooring callable the kernels cannot run: on the host, on the
            # (n_sources, n_frames) norms
            if self._variance_tensor() is not None:
                return self._host_weights_gauss(r2, contrast, flooring_fn)
            return self._host_weights(r2, flooring_fn)
        return _ops.iva_weight(r2, self.n_bins, contrast, self._resolve_floor(flooring_fn),
                               variance=self._variance_tensor())

    def _host_weights(self, r2, flooring_fn):
        """User closure on the frame norms: r (n_sources, n_frames) per mixture comes down, the
        weights go back up (ref: ssspy/bss/iva.py:1787-1789, :1962-1964)."""
        if type(flooring_fn) is str and flooring_fn == "self":
            flooring_fn = self.flooring_fn
        flooring_fn = choose_flooring_fn(flooring_fn, method=self)
        self._check_device_errors()
        r = np.sqrt(dv.to_host(r2))  # (B, N, T)
        weight = np.stack([np.asarray(self.d_contrast_fn(rb) / flooring_fn(2 * rb), dtype=np.float64)
                           for rb in r])
        if weight.shape != r.shape:
            raise ValueError("d_contrast_fn must map (n_sources, n_frames) to the same shape.")
        return dv.to_device(weight, dtype=np.float64, dev=r2.device)

    def _host_weights_gauss(self, r2, contrast, flooring_fn):
        """AuxGaussIVA with a flooring callable the kernels cannot run: the variance refresh
        alpha = r^2 / n_bins (ssspy/bss/iva.py:3465-3473) unless the pair loop of IP2 keeps it fixed,
        then varphi = (2 r / alpha) / flooring_fn(2 r) on the (n_sources, n_frames) norms
        (:3273-3288, :1787-1789) -- host arithmetic on B N T numbers, as for user closures."""
        flooring_fn = choose_flooring_fn(self.flooring_fn if (type(flooring_fn) is str and
                                                              flooring_fn == "self") else flooring_fn,
                                         method=self)
        self._check_device_errors()
        r2h = dv.to_host(r2)  # (B, N, T)
        var_dev = self._variance_tensor()
        if contrast == _lib.CONTRAST_GAUSS_FIXED:
            var = dv.to_host(var_dev)
        else:
            var = r2h / float(self.n_bins)
            var_dev.copy_(dv.to_device(var, dtype=np.float64, dev=r2.device))
        r = np.sqrt(r2h)
        weight = np.stack([np.asarray((2 * rb / vb) / flooring_fn(2 * rb), dtype=np.float64)
                           for rb, vb in zip(r, var)])
        return dv.to_device(weight, dtype=np.float64, dev=r2.device)

    def _frame_power(self):
        """r_nj^2 = sum_i |y_nij|^2 of the current estimate, (B, N, T)."""
        if self._uses_filter():
            return _ops.iva_frame_power(self._X, self._state_dev("demix_filter"))
        cache = self._r2_cache
        if cache is None or cache[1] != self._state_rev("output"):
            W = self._implied_filter()
            if W is not None:
                r2 = _ops.iva_frame_power(self._X, W)
            else:
                r2 = _ops.iva_frame_power(self._state_dev("output"), None)
            cache = (r2, self._state_rev("output"))
            self._r2_cache = cache
        return cache[0]

    def update_once(self, flooring_fn="self") -> None:
        """ref: ssspy/bss/iva.py:1699-1734."""
        if self.spatial_algorithm in _IP1:
            self.update_once_ip1(flooring_fn=flooring_fn)
        elif self.spatial_algorithm in _ISS1:
            self.update_once_iss1(flooring_fn=flooring_fn)
        elif self.spatial_algorithm in _IP2:
            self.update_once_ip2(flooring_fn=flooring_fn)
        elif self.spatial_algorithm in _ISS2:
            self.update_once_iss2(flooring_fn=flooring_fn)
        elif self.spatial_algorithm in _IPA:
            self.update_once_ipa(flooring_fn=flooring_fn)
        else:
            raise NotImplementedError("Not support {}.".format(self.spatial_algorithm))

    def update_once_ipa(self, flooring_fn="self") -> None:
        """Iterative projection with adjustment.  ref: ssspy/bss/iva.py:2068-2175."""
        floor = self._resolve_floor(flooring_fn)
        require_device_floor(floor, "IPA")
        if self._update_once_implied(flooring_fn):
            return
        Y = self._state_dev("output")
        weight = self._weights(flooring_fn)
        r2 = _ops.update_by_ipa(Y, weight, _lib.WEIGHT_FRAME, self.lqpqm_normalization,
                                self.newton_iter, floor, self._newton_words(Y.device),
                                self._info_tensor(), not_converged=self._newton_counter(),
                                frame_power=True)
        self._state_touch("output")
        self._r2_cache = None if r2 is None else (r2, self._state_rev("output"))

    def _pair_weight_contrast(self):
        """Contrast code for the per-pair weights of IP2 (the Gauss model keeps its variance)."""
        return self._contrast

    def update_once_ip2(self, flooring_fn="self") -> None:
        """Pairwise iterative projection; the auxiliary weights are recomputed for every pair from
        the current filters.  ref: ssspy/bss/iva.py:1795-1915."""
        N = self.n_sources
        floor = self._resolve_floor(flooring_fn)
        W = self._state_dev("demix_filter")
        for m, n in resolve_pairs(getattr(self, "pair_selector", None), N):
            r2 = _ops.iva_frame_power(self._X, W)
            weight = self._weights_from_power(r2, self._pair_weight_contrast(), flooring_fn)
            B, _, F, _ = self._X.shape
            if N <= 4 and B * ((F + 31) // 32) >= 512:
                # (batches: the tuned frame-weight covariance forms all N sets in 241 us where the
                #  generic kernel takes 325 for the pair's two -- 32 mixtures of configs[1])
                U = _ops.weighted_covariance(self._X, weight, _lib.WEIGHT_FRAME, N)
                _ops.update_by_ip2(W, U, [(m, n)], floor, self._info_tensor())
                continue
            w_pair = weight[:, [m, n], :].contiguous()  # gather of two rows (data movement only)
            U_pair = _ops.weighted_covariance(self._X, w_pair, _lib.WEIGHT_FRAME, 2)
            _ops.update_by_ip2(W, U_pair, [(m, n)], floor, self._info_tensor(), pair_only=True)
        self._state_touch("demix_filter")

    def update_once_iss2(self, flooring_fn="self") -> None:
        """Pairwise iterative source steering.  ref: ssspy/bss/iva.py:1968-2066."""
        N = self.n_sources
        if self._update_once_implied(flooring_fn):
            return
        Y = self._state_dev("output")
        floor = self._resolve_floor(flooring_fn)
        weight = self._weights(flooring_fn)
        Vc = _ops.weighted_covariance(Y, weight, _lib.WEIGHT_FRAME, N)
        G = _ops.iss2_transform(Vc, resolve_pairs(getattr(self, "pair_selector", None), N), floor,
                                self._info_tensor())
        self._separate_output(Y, G)

    def _update_once_implied(self, flooring_fn) -> bool:
        """ISS2 / IPA iteration without touching Y (round 5).  The reference keeps only the separated
        spectrogram and rewrites it (iva.py:1968-2175): weights from its frame powers, statistics
        mean phi y y^H, Y <- G Y -- three spectrogram-sized transfers per iteration even with the
        frame powers taken in the rewrite.  With output = W x the frame powers are |W x|^2 (the IP1
        pass), the statistics W U W^H with the weighted covariances U of the MIXTURE, the update
        W <- G W on (F, N, N): two read-only passes, Y formed when ``output`` is read
        (_state_defer).  False: not applicable, the caller runs the literal form."""
        W = self._implied_filter()
        floor = self._resolve_floor(flooring_fn)
        if W is None or host_floor(floor) is not None or self._contrast is None:
            return False
        if self._amp_exceeded():
            self._leave_implied_route()
            self._r2_cache = None
            return False
        weight = self._weights(flooring_fn)  # (frame powers through _frame_power(): |W x|^2)
        self._implied_step(_ops.weighted_covariance(self._X, weight, _lib.WEIGHT_FRAME,
                                                    self._X.shape[1]), floor)
        self._r2_cache = None
        return True

    def update_once_ip1(self, flooring_fn="self") -> None:
        """ref: ssspy/bss/iva.py:1736-1793."""
        N = self.n_sources
        weight = self._weights(flooring_fn)
        U = _ops.weighted_covariance(self._X, weight, _lib.WEIGHT_FRAME, N)
        _ops.update_by_ip1(self._state_dev("demix_filter"), U, self._resolve_floor(flooring_fn),
                           self._info_tensor())
        self._state_touch("demix_filter")

    def update_once_iss1(self, flooring_fn="self") -> None:
        """ref: ssspy/bss/iva.py:1917-1966 and _update_spatial_model.py:146-194."""
        N = self.n_sources
        Y = self._state_dev("output")
        weight = self._weights(flooring_fn)
        floor = self._resolve_floor(flooring_fn)
        if host_floor(floor) is not None:
            _ops.update_by_iss1_host_floor(Y, weight, _lib.WEIGHT_FRAME, floor.host)
            self._state_touch("output")
            self._restamp_logdet(None)
        elif self.n_frames <= _ops.iss1_fused_max_frames(N):
            # one read + one write of Y; the kernel also leaves the next iteration's frame powers
            r2_next = dv.empty(tuple(weight.shape), dv.f64, Y.device)
            tracked = self._tracked_logdet()
            _ops.iss1_fused(Y, weight, _lib.WEIGHT_FRAME, floor, r2_next, logdet=tracked)
            self._state_touch("output")
            self._r2_cache = (r2_next, self._state_rev("output"))
            self._restamp_logdet(tracked)
        else:
            Vc = _ops.weighted_covariance(Y, weight, _lib.WEIGHT_FRAME, N)
            G = _ops.iss1_transform(Vc, floor)
            self._separate_output(Y, G)

    def _separate_output(self, Y, G) -> None:
        """Y <- G Y in place; the walk also leaves sum_i |y|^2 of the new Y, which the next
        iteration's weights would otherwise fetch with a pass of their own (round 5)."""
        r2 = _ops.separate_frame_power(Y, G)
        if r2 is None:
            _ops.separate(Y, G, out=Y)
        self._state_touch("output")
        self._r2_cache = None if r2 is None else (r2, self._state_rev("output"))

    def _logdet_sum(self):
        """sum_i log|det W_i| (B,) on the device, and the filters if they had to be formed."""
        if self._uses_filter():
            W = self._state_dev("demix_filter")
            return _ops.sum_logdet(W), W
        W = self._implied_filter()
        if W is not None:
            return _ops.sum_logdet(W), W
        tracked = self._tracked_logdet()
        if tracked is not None:
            return tracked, None
        W = _ops.demix_from_covariance(_ops.cross_covariance(self._state_dev("output"), self._X),
                                       self._C(), self._info_tensor())
        return _ops.sum_logdet(W), W

    def compute_loss(self) -> float:
        """ref: ssspy/bss/iva.py:200-222 (filter state), :2177-2192 (ISS state)."""
        if self._contrast is None:
            logdet, W = self._logdet_sum()
            return self._host_contrast_loss(W, logdet)
        return self._host_loss(*self._loss_terms())

    def _loss_terms(self, data_out=None, logdet_out=None):
        """(contrast term, sum_i log|det W_i|) of the current state on the device, each (B,)."""
        logdet, _ = self._logdet_sum()
        data = _ops.iva_loss_data(self._frame_power(), self._variance_tensor(), self.n_bins,
                                  self._contrast, out=data_out)
        if logdet_out is not None:
            logdet_out.copy_(logdet)  # (the tracked sum is moved in place by the next sweep)
            logdet = logdet_out
        return data, logdet

    def _host_contrast_loss(self, W, logdet_dev):
        """Loss with a user ``contrast_fn``: the closure takes the whole separated spectrogram
        (ssspy/bss/iva.py:216, :2181), so the estimate crosses PCIe once per recorded loss -- the
        price of an opaque Python callable, paid only with ``record_loss=True``."""
        if self.contrast_fn is None:
            raise ValueError("Specify contrast_fn to record the loss.")
        if self._uses_filter():
            Y = dv.to_host(_ops.separate(self._X, W))
        else:
            Y = dv.to_host(self._state_dev("output"))
        self._check_device_errors()
        logdet = dv.to_host(logdet_dev)
        values = np.array([np.sum(np.mean(self.contrast_fn(Yb), axis=1), axis=0) for Yb in Y])
        values = values - 2.0 * logdet
        return values.copy() if self._batched else values[0].item()


class AuxLaplaceIVA(AuxIVA):
    """AuxIVA with the spherical Laplace source model (ref: ssspy/bss/iva.py:2976-3128)."""

    def __init__(
        self,
        spatial_algorithm: str = "IP",
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        pair_selector: Optional[Callable[[int], Iterable[Tuple[int, int]]]] = None,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
        **kwargs,
    ) -> None:
        def contrast_fn(y: np.ndarray) -> np.ndarray:
            """G(y) = 2 ||y||_2 over bins; y (n_sources, n_bins, n_frames)."""
            return 2 * np.linalg.norm(y, axis=1)

        def d_contrast_fn(y: np.ndarray) -> np.ndarray:
            """G'(r) = 2."""
            return 2 * np.ones_like(y)

        contrast_fn._ssspy_amd_contrast = _lib.CONTRAST_LAPLACE
        d_contrast_fn._ssspy_amd_contrast = _lib.CONTRAST_LAPLACE
        super().__init__(
            spatial_algorithm=spatial_algorithm,
            contrast_fn=contrast_fn,
            d_contrast_fn=d_contrast_fn,
            flooring_fn=flooring_fn,
            pair_selector=pair_selector,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
            **kwargs,
        )

    def __repr__(self) -> str:
        return "AuxLaplaceIVA" + super().__repr__()[len("AuxIVA"):]


class AuxGaussIVA(AuxIVA):
    """AuxIVA with the time-varying Gauss source model (ref: ssspy/bss/iva.py:3131-3473)."""

    variance = Synced(dv.f64)

    def __init__(
        self,
        spatial_algorithm: str = "IP",
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        pair_selector: Optional[Callable[[int], Iterable[Tuple[int, int]]]] = None,
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
        **kwargs,
    ) -> None:
        def contrast_fn(y: np.ndarray) -> np.ndarray:
            """G(y) = n_bins log(alpha) + ||y||^2 / alpha."""
            norm = np.linalg.norm(y, axis=1)
            return self.n_bins * np.log(self.variance) + (norm**2) / self.variance

        def d_contrast_fn(y: np.ndarray, variance: np.ndarray = None) -> np.ndarray:
            """G'(r) = 2 r / alpha."""
            alpha = self.variance if variance is None else variance
            return 2 * y / alpha

        contrast_fn._ssspy_amd_contrast = _lib.CONTRAST_GAUSS
        d_contrast_fn._ssspy_amd_contrast = _lib.CONTRAST_GAUSS
        super().__init__(
            spatial_algorithm=spatial_algorithm,
            contrast_fn=contrast_fn,
            d_contrast_fn=d_contrast_fn,
            flooring_fn=flooring_fn,
            pair_selector=pair_selector,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
            **kwargs,
        )

    def __repr__(self) -> str:
        return "AuxGaussIVA" + super().__repr__()[len("AuxIVA"):]

    def _reset(self, **kwargs) -> None:
        """ref: ssspy/bss/iva.py:3304-3317."""
        super()._reset(**kwargs)
        self.variance = np.ones(self._lead() + (self.n_sources, self.n_frames))

    def _variance_tensor(self):
        return self._state_dev("variance")

    def update_once(self, flooring_fn="self") -> None:
        """Refresh the variance, then the spatial update (ref: ssspy/bss/iva.py:3319-3337).

        The variance refresh alpha_nj = mean_i |y_nij|^2 (:3465-3473) is fused into the weight
        kernel (it is r^2 / n_bins of the same frame power).
        """
        super().update_once(flooring_fn=flooring_fn)
        self._state_touch("variance")

    def update_source_model(self) -> None:
        """alpha_nj = mean_i |y_nij|^2 (ref: ssspy/bss/iva.py:3465-3473)."""
        if host_floor(self._floor) is not None:  # (no floor acts on the variance itself)
            var = dv.to_host(self._frame_power()) / float(self.n_bins)
            self._variance_tensor().copy_(dv.to_device(var, dtype=np.float64))
        else:
            _ops.iva_weight(self._frame_power(), self.n_bins, _lib.CONTRAST_GAUSS, self._floor,
                            variance=self._variance_tensor())
        self._state_touch("variance")

    def _pair_weight_contrast(self):
        return _lib.CONTRAST_GAUSS_FIXED

    def update_once_ip2(self, flooring_fn="self") -> None:
        """ref: ssspy/bss/iva.py:3319-3337 (variance refresh) + :3339-3463 (pairs, fixed variance)."""
        self.update_source_model()
        super().update_once_ip2(flooring_fn=flooring_fn)


# ------------------------------------------------------------------ fixed point (Fast / Faster)
class FastIVABase(IVABase):
    """IVA by fixed-point iterations on the whitened mixture (ref: ssspy/bss/iva.py:409-550).

    ``_reset`` whitens the input once (covariance pass, per-bin filter, one correction of it,
    ``separate``; all on the device) into ``whitened_input``; ``demix_filter`` acts on that, not on ``input``, and stays
    unitary, so the loss has no log-determinant term.  ``whitened_input`` and ``demix_filter`` are
    defined up to a unit factor per (channel, bin): the phase of the eigenvectors is the
    decomposition's (the reference's is LAPACK's, just as arbitrary).

    The reference has no named Fast classes, so the contrast is always a set of Python closures:
    ``d_contrast_fn`` / ``dd_contrast_fn`` run on the host on the (n_sources, n_frames) frame norms
    between the two device passes of an iteration (a few KB down, a few KB up per mixture), and
    ``contrast_fn`` takes the whole estimate, so a host copy of it is formed whenever the loss is
    recorded (``record_loss=True``: once per iteration) -- the price of opaque callables.  The three
    built-in floors run inside the weight kernel; any other flooring callable runs on the host on
    the norms.

    Where the reference's ``np.linalg.svd`` never raises, a bin whose W W^H is singular to working
    precision (an injected singular ``demix_filter``) raises ``numpy.linalg.LinAlgError``.
    """

    whitened_input = Synced(dv.c128)

    def __init__(
        self,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[
            Union[Callable[["IVABase"], None], List[Callable[["IVABase"], None]]]
        ] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )

    def __call__(
        self, input: np.ndarray, n_iter: int = 100, initial_call: bool = True, **kwargs
    ) -> np.ndarray:
        """Separate a frequency-domain multichannel mixture (ref: ssspy/bss/iva.py:1102-1136)."""
        self._bind_input(input)
        self._reset(**kwargs)
        IterativeMethodBase.__call__(self, n_iter=n_iter, initial_call=initial_call)
        if self.scale_restoration:
            self.restore_scale()
        self._state_set_dev("output", _ops.separate(self._state_dev("whitened_input"),
                                                    self._state_dev("demix_filter")))
        return self._final_output()

    def __repr__(self) -> str:
        s = "FastIVA(scale_restoration={}, record_loss={}".format(
            self.scale_restoration, self.record_loss
        )
        if self.scale_restoration:
            s += ", reference_id={}".format(self.reference_id)
        return s + ")"

    def _reset(self, **kwargs) -> None:
        """ref: ssspy/bss/iva.py:466-476."""
        assert self._has_input(), "Specify data!"
        n_sources = self._X.shape[1]
        if not 2 <= n_sources <= _lib.RT_MAX_SOURCES:
            raise NotImplementedError(
                "{} takes 2 to {} sources, got {}.".format(
                    type(self).__name__, _lib.RT_MAX_SOURCES, n_sources))
        super()._reset(**kwargs)
        Z = _ops.whitened(self._X, self._info_tensor())
        self._state_set_dev("whitened_input", Z)
        self._state_set_dev("output", _ops.separate(Z, self._state_dev("demix_filter")))

    def separate(
        self, input: np.ndarray, demix_filter: np.ndarray, use_whitening: bool = True
    ) -> np.ndarray:
        """y_ij = W_i z_ij with z the whitened ``input``, or ``input`` itself
        (ref: ssspy/bss/iva.py:478-509)."""
        if use_whitening:
            from ..transform import whiten

            whitened_input = whiten(input)
        else:
            whitened_input = input
        return super().separate(whitened_input, demix_filter=demix_filter)

    def _norm_weights(self, flooring_fn, want_psi: bool):
        """(phi, psi) (B, N, T) on the device: the frame-power pass, the closures on the host on the
        norms, the floor in the weight kernel or, for a callable it cannot run, on the host too
        (ref: ssspy/bss/iva.py:1187-1188, :1196, :1390-1391)."""
        r2 = _ops.iva_frame_power(self._state_dev("whitened_input"), self._state_dev("demix_filter"))
        floor = self._resolve_floor(flooring_fn)
        self._check_device_errors()
        norm = np.sqrt(dv.to_host(r2))  # (B, N, T)

        def on_norms(fn):
            out = np.stack([np.asarray(fn(rb), dtype=np.float64) for rb in norm])
            if out.shape != norm.shape:
                raise ValueError(
                    "the contrast derivatives must map (n_sources, n_frames) to the same shape.")
            return out

        d = on_norms(self.d_contrast_fn)
        dd = on_norms(self.dd_contrast_fn) if want_psi else None
        if host_floor(floor) is not None:
            denom = on_norms(lambda rb: host_floor(floor)(2 * rb))
            phi = d / denom
            psi = (2 * phi - dd) / denom if want_psi else None
            up = functools.partial(dv.to_device, dtype=np.float64, dev=r2.device)
            return up(phi), (up(psi) if want_psi else None)
        up = functools.partial(dv.to_device, dtype=np.float64, dev=r2.device)
        return _ops.fast_iva_weights(r2, up(d), up(dd) if want_psi else None, floor,
                                     want_psi=want_psi)

    def compute_loss(self) -> float:
        """sum_n mean_j G(y)_nj; no log-determinant, the filters are unitary
        (ref: ssspy/bss/iva.py:511-531)."""
        Y = dv.to_host(_ops.separate(self._state_dev("whitened_input"),
                                     self._state_dev("demix_filter")))
        self._check_device_errors()
        values = np.array([np.sum(np.mean(self.contrast_fn(Yb), axis=1), axis=0) for Yb in Y],
                          dtype=np.float64)
        return self._loss_entry(values)

    def apply_projection_back(self) -> None:
        """The estimate scaled against the unwhitened input, the filters re-fitted on the whitened
        one as Y Z^H (Z Z^H)^-1 (ref: ssspy/bss/iva.py:533-550)."""
        assert self.scale_restoration, "Set self.scale_restoration=True."
        Z = self._state_dev("whitened_input")
        Y = _ops.separate(Z, self._state_dev("demix_filter"))
        G = _ops.projection_back_scale(_ops.cross_covariance(self._X, Y),
                                       _ops.cross_covariance(Y, Y), self.reference_id,
                                       self._info_tensor())
        _ops.separate(Y, G, out=Y)
        W = _ops.demix_from_covariance(_ops.cross_covariance(Y, Z), _ops.cross_covariance(Z, Z),
                                       self._info_tensor())
        self._state_set_dev("demix_filter", W)
        self._state_set_dev("output", Y)

    def apply_minimal_distortion_principle(self) -> None:
        """As the reference does it (IVABase's method, whose ``separate`` call whitens;
        ssspy/bss/iva.py:269-281): the estimate W z scaled against the unwhitened input, the filters
        re-fitted on the UNWHITENED input as Y X^H (X X^H)^-1 -- ``__call__`` then applies them to
        the whitened one (:1132-1134)."""
        assert self.scale_restoration, "Set self.scale_restoration=True."
        Y = _ops.separate(self._state_dev("whitened_input"), self._state_dev("demix_filter"))
        G = _ops.mdp_scale(_ops.cross_covariance(Y, self._X), _ops.cross_covariance(Y, Y),
                           self.reference_id)
        _ops.separate(Y, G, out=Y)
        W = _ops.demix_from_covariance(_ops.cross_covariance(Y, self._X), self._C(),
                                       self._info_tensor())
        self._state_set_dev("demix_filter", W)
        self._state_set_dev("output", Y)


class FastIVA(FastIVABase):
    """Fast independent vector analysis (ref: ssspy/bss/iva.py:991-1207).

    An iteration reads the whitened mixture twice: the frame-power pass, and one pass that leaves the
    three moments per (bin, source) the update needs (``_ops.fast_iva_stats``); the per-bin step forms
    the new filters and orthonormalises their rows.  Host costs: see ``FastIVABase``."""

    def __init__(
        self,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        d_contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        dd_contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[
            Union[Callable[["FastIVA"], None], List[Callable[["FastIVA"], None]]]
        ] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        if contrast_fn is None:
            raise ValueError("Specify contrast function.")
        self.contrast_fn = contrast_fn
        if d_contrast_fn is None:
            raise ValueError("Specify derivative of contrast function.")
        self.d_contrast_fn = d_contrast_fn
        if dd_contrast_fn is None:
            raise ValueError("Specify second order derivative of contrast function.")
        self.dd_contrast_fn = dd_contrast_fn

    def update_once(
        self,
        flooring_fn: Optional[Union[str, Callable[[np.ndarray], np.ndarray]]] = "self",
    ) -> None:
        """ref: ssspy/bss/iva.py:1150-1207."""
        Z, W = self._state_dev("whitened_input"), self._state_dev("demix_filter")
        phi, psi = self._norm_weights(flooring_fn, want_psi=True)
        c, b, a = _ops.fast_iva_stats(Z, W, phi, psi)
        _ops.fast_iva_step(W, c, b, a, self.n_frames, self._info_tensor())
        self._state_touch("demix_filter")


class FasterIVA(FastIVABase):
    """Faster independent vector analysis (ref: ssspy/bss/iva.py:1210-1400).

    An iteration is the frame-power pass, the frame-weighted covariance pass of AuxIVA-IP1 on the
    whitened mixture and a per-bin step: the principal eigenvector of every U_in into row n, then
    the row orthonormalisation.  Host costs: see ``FastIVABase``."""

    def __init__(
        self,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        d_contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[
            Union[Callable[["FasterIVA"], None], List[Callable[["FasterIVA"], None]]]
        ] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        if contrast_fn is None:
            raise ValueError("Specify contrast function.")
        self.contrast_fn = contrast_fn
        if d_contrast_fn is None:
            raise ValueError("Specify derivative of contrast function.")
        self.d_contrast_fn = d_contrast_fn

    def __repr__(self) -> str:
        return "FasterIVA" + super().__repr__()[len("FastIVA"):]

    def update_once(
        self,
        flooring_fn: Optional[Union[str, Callable[[np.ndarray], np.ndarray]]] = "self",
    ) -> None:
        """ref: ssspy/bss/iva.py:1354-1400."""
        Z, W = self._state_dev("whitened_input"), self._state_dev("demix_filter")
        phi, _ = self._norm_weights(flooring_fn, want_psi=False)
        U = _ops.weighted_covariance(Z, phi, _lib.WEIGHT_FRAME, self.n_sources)
        _ops.faster_iva_step(W, U, self._info_tensor())
        self._state_touch("demix_filter")


# ------------------------------------------------------------------ gradient / natural gradient
def _device_score(method):
    """Which built-in source model the separator's pair of callables stands for, or None for user
    closures.  The four named classes tag the closures they build with the model and with the
    instance they belong to: closures borrowed from another instance read that instance's floor or
    variance, so they count as user closures and take the compatibility path."""
    tags = [(getattr(fn, "_ssspy_amd_contrast", None), getattr(fn, "_ssspy_amd_owner", None))
            for fn in (method.contrast_fn, method.score_fn)]
    if tags[0][0] is None or tags[0][0] != tags[1][0] or any(t[1] is not method for t in tags):
        return None
    return tags[0][0]


class GradIVABase(IVABase):
    """IVA by (natural) gradient descent (ref: ssspy/bss/iva.py:284-406).

    With the source models of the four named subclasses the score is phi_nj y_inj with one real
    weight per (source, frame), hence mean_j phi(y) y^H = W U_n W^H (row n) with the frame-weighted
    covariances U_n of the mixture: an iteration is the frame-power pass, the covariance pass and one
    per-bin step, all on the device, and ``output`` is formed when somebody reads it.

    With user closures (``GradIVA`` / ``NaturalGradIVA`` constructed directly) this is the
    compatibility path, not the fast one: ``score_fn`` takes the whole (n_sources, n_bins, n_frames)
    estimate, so the estimate comes to the host once per iteration and the scores go back up;
    mean_j phi(y) y^H is then the cross-covariance operator and the step kernel takes it as it is.
    ``contrast_fn`` is evaluated on a host copy of the estimate, only when the loss is recorded.
    """

    _natural = False
    variance = None  # (the Gauss classes keep one)

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
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        super().__init__(
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        self.step_size = step_size
        if contrast_fn is None:
            raise ValueError("Specify contrast function.")
        self.contrast_fn = contrast_fn
        if score_fn is None:
            raise ValueError("Specify score function.")
        self.score_fn = score_fn
        self.is_holonomic = is_holonomic

    def __call__(
        self, input: np.ndarray, n_iter: int = 100, initial_call: bool = True, **kwargs
    ) -> np.ndarray:
        """Separate a frequency-domain multichannel mixture (ref: ssspy/bss/iva.py:359-392)."""
        self._bind_input(input)
        self._reset(**kwargs)
        if not self._iterate_with_resident_loss(int(n_iter), initial_call):
            IterativeMethodBase.__call__(self, n_iter=n_iter, initial_call=initial_call)
        return self._finish_call()

    def __repr__(self) -> str:
        s = "GradIVA(step_size={}, is_holonomic={}, scale_restoration={}, record_loss={}".format(
            self.step_size, self.is_holonomic, self.scale_restoration, self.record_loss
        )
        if self.scale_restoration:
            s += ", reference_id={}".format(self.reference_id)
        return s + ")"

    def _reset(self, **kwargs) -> None:
        """ref: ssspy/bss/iva.py:138-169."""
        assert self._has_input(), "Specify data!"
        if self._X.shape[1] > _lib.RT_MAX_SOURCES:
            raise NotImplementedError(
                "{} takes up to {} sources, got {}.".format(
                    type(self).__name__, _lib.RT_MAX_SOURCES, self._X.shape[1]))
        super()._reset(**kwargs)
        self._score = _device_score(self)

    def _variance_tensor(self):
        return None

    def _fill_output(self) -> None:
        ent = self._state()["output"]
        if ent["dev"] is None:
            ent["dev"] = dv.empty(tuple(self._X.shape), dv.c128, self._X.device)
        _ops.separate(self._X, self._state_dev("demix_filter"), out=ent["dev"])

    def _filters_stepped(self) -> None:
        """Behind a step: the filters moved, ``output`` follows them when it is read
        (the reference's ``self.output = Y`` at the end of update_once, ssspy/bss/iva.py:815-818)."""
        self._state_touch("demix_filter")
        self._state_defer("output", self._fill_output)
        if self._variance_tensor() is not None:
            self._state_touch("variance")

    def _score_weights(self, r2, refresh=True):
        """phi_nj (B, N, T) from the frame powers; the Gauss model refreshes its variance on the
        way unless ``refresh`` is False (an overridden ``update_source_model`` has set it)."""
        if self._score == _lib.CONTRAST_LAPLACE and host_floor(self._floor) is not None:
            # a flooring callable the kernels cannot run: on the host, on the (n_sources, 1,
            # n_frames) norms it sees in the reference (ssspy/bss/iva.py:2448-2451)
            self._check_device_errors()
            r = np.sqrt(dv.to_host(r2))  # (B, N, T)
            weight = np.stack([
                1.0 / np.asarray(self.flooring_fn(rb[:, np.newaxis, :]), dtype=np.float64)[:, 0, :]
                for rb in r])
            return dv.to_device(weight, dtype=np.float64, dev=r2.device)
        floor = self._floor if host_floor(self._floor) is None else device_flooring(identity)
        contrast = self._score
        if contrast == _lib.CONTRAST_GAUSS and not refresh:
            contrast = _lib.CONTRAST_GAUSS_FIXED
        return _ops.iva_score_weight(r2, self.n_bins, contrast, floor,
                                     variance=self._variance_tensor())

    def _step(self, r2=None, logdet=None, logdet_stride=0, refresh=True) -> None:
        """One update of the filters with a built-in source model, on the device."""
        W = self._state_dev("demix_filter")
        if r2 is None:
            r2 = _ops.iva_frame_power(self._X, W)
        weight = self._score_weights(r2, refresh)
        U = _ops.weighted_covariance(self._X, weight, _lib.WEIGHT_FRAME, self.n_sources)
        _ops.iva_grad_step(W, U, self._natural, self.is_holonomic, self.step_size,
                           self._info_tensor(), logdet=logdet, logdet_stride=logdet_stride)

    def update_once(self) -> None:
        """ref: ssspy/bss/iva.py:764-818 (gradient), :936-988 (natural gradient)."""
        if self._score is not None:
            own = getattr(type(self), "update_source_model", None)
            if own is not None and own is not _GradGaussMixin.update_source_model:
                # a subclass's own source model, as the reference calls it before the step
                # (ssspy/bss/iva.py:2640-2644); the step then takes the variance as it stands
                self.update_source_model()
                self._step(refresh=False)
            else:
                # (the stock refresh alpha = r^2 / n_bins runs inside the step's weight kernel)
                self._step()
        else:
            W = self._state_dev("demix_filter")
            Y = _ops.separate(self._X, W)
            self._check_device_errors()
            Phi = np.stack([np.asarray(self.score_fn(Yb), dtype=np.complex128)
                            for Yb in dv.to_host(Y)])
            if Phi.shape != tuple(Y.shape):
                raise ValueError("score_fn must map (n_sources, n_bins, n_frames) to the same shape.")
            PhiY = _ops.cross_covariance(dv.to_device(Phi, dtype=np.complex128, dev=Y.device), Y)
            _ops.iva_grad_step(W, PhiY, self._natural, self.is_holonomic, self.step_size,
                               self._info_tensor())
        self._filters_stepped()

    def compute_loss(self) -> float:
        """ref: ssspy/bss/iva.py:200-222."""
        W = self._state_dev("demix_filter")
        logdet = _ops.sum_logdet(W)
        if self._score is not None:
            data = _ops.iva_loss_data(_ops.iva_frame_power(self._X, W), self._variance_tensor(),
                                      self.n_bins, self._score)
            return self._host_loss(data, logdet)
        Y = dv.to_host(_ops.separate(self._X, W))
        self._check_device_errors()
        values = np.array([np.sum(np.mean(self.contrast_fn(Yb), axis=1), axis=0) for Yb in Y])
        return self._loss_entry(values - 2.0 * dv.to_host(logdet))

    def _iterate_with_resident_loss(self, n_iter: int, initial_call: bool) -> bool:
        """``record_loss=True`` at the cost of ``record_loss=False`` when nothing can look at
        ``self.loss`` in between (no callbacks, stock methods, a source model and a floor that run on
        the device): the contrast term of the state after iteration t comes from the frame powers
        iteration t + 1 forms anyway, sum_i log|det W_i| from the step kernel's shares, and the
        terms stay in HBM until the end (_resident_loss).  The Gauss term is evaluated with the
        variance as it stands BEFORE the step refreshes it: the reference's ``compute_loss`` sees the
        variance of the start of the iteration against the new filters (ssspy/bss/iva.py:2625-2651).
        False: the reference's loop."""
        cls = type(self)
        B, N = self._X.shape[0], self.n_sources
        nld = _ops.iva_grad_step_logdet_slots(B, self.n_bins, N)
        # (stock methods: the ones this module defines, the Gauss classes' own included)
        methods = [getattr(cls, name, None) for name in (
            "update_once", "compute_loss", "update_source_model", "_step", "_score_weights")]
        stock = all(fn is None or fn.__module__ == __name__ for fn in methods)
        if not (self._unobserved_loss(n_iter) and self._score is not None and stock
                and host_floor(self._floor) is None and LossShares.fit(nld, n_iter + 1, B)):
            return False

        def prepare(data, logdet):
            W = self._state_dev("demix_filter")
            ld = LossShares(nld, n_iter + 1, B, self._X.device, logdet)

            def step(t, record):
                r2 = _ops.iva_frame_power(self._X, W)
                if record:
                    _ops.iva_loss_data(r2, self._variance_tensor(), self.n_bins, self._score,
                                       out=data[t])
                self._step(r2, ld.at(t), ld.stride)

            def end():
                _ops.iva_loss_data(_ops.iva_frame_power(self._X, W), self._variance_tensor(),
                                   self.n_bins, self._score, out=data[n_iter])
                ld.fold()
                _ops.sum_logdet(W, out=logdet[n_iter])
                self._filters_stepped()

            return step, end
        return self._resident_loss(n_iter, initial_call, prepare)


class GradIVA(GradIVABase):
    """IVA by gradient descent, W <- W - eta D W^-H (ref: ssspy/bss/iva.py:644-818).

    With ``contrast_fn`` / ``score_fn`` closures this is the compatibility path of ``GradIVABase``."""

    def __init__(
        self,
        step_size: float = 1e-1,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        score_fn: Callable[[np.ndarray], np.ndarray] = None,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        is_holonomic: bool = True,
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
            is_holonomic=is_holonomic,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )


class NaturalGradIVA(GradIVABase):
    """IVA by natural gradient descent, W <- W - eta D W (ref: ssspy/bss/iva.py:821-988).

    With ``contrast_fn`` / ``score_fn`` closures this is the compatibility path of ``GradIVABase``."""

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
        is_holonomic: bool = True,
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
            is_holonomic=is_holonomic,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )


def _laplace_closures(method):
    """The spherical Laplace model: G = 2 ||y||_2, phi = y / floor(||y||_2)
    (ref: ssspy/bss/iva.py:2429-2451, :2733-2760)."""
    def contrast_fn(y: np.ndarray) -> np.ndarray:
        return 2 * np.linalg.norm(y, axis=1)

    def score_fn(y: np.ndarray) -> np.ndarray:
        norm = np.linalg.norm(y, axis=1, keepdims=True)
        return y / method.flooring_fn(norm)

    contrast_fn._ssspy_amd_contrast = score_fn._ssspy_amd_contrast = _lib.CONTRAST_LAPLACE
    contrast_fn._ssspy_amd_owner = score_fn._ssspy_amd_owner = method
    return contrast_fn, score_fn


def _gauss_closures(method):
    """The time-varying Gauss model: G = n_bins log(alpha) + ||y||^2 / alpha, phi = y / alpha
    (ref: ssspy/bss/iva.py:2586-2611, :2908-2935)."""
    def contrast_fn(y: np.ndarray) -> np.ndarray:
        alpha = method.variance
        norm = np.linalg.norm(y, axis=1)
        return method.n_bins * np.log(alpha) + (norm**2) / alpha

    def score_fn(y: np.ndarray) -> np.ndarray:
        return y / method.variance[:, np.newaxis, :]

    contrast_fn._ssspy_amd_contrast = score_fn._ssspy_amd_contrast = _lib.CONTRAST_GAUSS
    contrast_fn._ssspy_amd_owner = score_fn._ssspy_amd_owner = method
    return contrast_fn, score_fn


class _GradGaussMixin:
    """Variance state of the two Gauss classes (ref: ssspy/bss/iva.py:2613-2651, :2937-2973)."""

    variance = Synced(dv.f64)

    def _reset(self, **kwargs) -> None:
        super()._reset(**kwargs)
        self.variance = np.ones(self._lead() + (self.n_sources, self.n_frames))

    def _variance_tensor(self):
        return self._state_dev("variance")

    def update_source_model(self) -> None:
        """alpha_nj = mean_i |y_nij|^2 (ref: ssspy/bss/iva.py:2646-2651)."""
        r2 = _ops.iva_frame_power(self._X, self._state_dev("demix_filter"))
        _ops.iva_score_weight(r2, self.n_bins, _lib.CONTRAST_GAUSS, device_flooring(identity),
                              variance=self._variance_tensor())
        self._state_touch("variance")


class GradLaplaceIVA(GradIVA):
    """Gradient IVA with the spherical Laplace source model (ref: ssspy/bss/iva.py:2341-2501)."""

    def __init__(
        self,
        step_size: float = 1e-1,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        is_holonomic: bool = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        contrast_fn, score_fn = _laplace_closures(self)
        super().__init__(
            step_size=step_size,
            contrast_fn=contrast_fn,
            score_fn=score_fn,
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            is_holonomic=is_holonomic,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )


class GradGaussIVA(_GradGaussMixin, GradIVA):
    """Gradient IVA with the time-varying Gauss source model (ref: ssspy/bss/iva.py:2504-2651)."""

    def __init__(
        self,
        step_size: float = 1e-1,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        is_holonomic: bool = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        contrast_fn, score_fn = _gauss_closures(self)
        super().__init__(
            step_size=step_size,
            contrast_fn=contrast_fn,
            score_fn=score_fn,
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            is_holonomic=is_holonomic,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )


class NaturalGradLaplaceIVA(NaturalGradIVA):
    """Natural-gradient IVA with the spherical Laplace source model
    (ref: ssspy/bss/iva.py:2654-2820)."""

    def __init__(
        self,
        step_size: float = 1e-1,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        is_holonomic: bool = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        contrast_fn, score_fn = _laplace_closures(self)
        super().__init__(
            step_size=step_size,
            contrast_fn=contrast_fn,
            score_fn=score_fn,
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            is_holonomic=is_holonomic,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )


class NaturalGradGaussIVA(_GradGaussMixin, NaturalGradIVA):
    """Natural-gradient IVA with the time-varying Gauss source model
    (ref: ssspy/bss/iva.py:2823-2973)."""

    def __init__(
        self,
        step_size: float = 1e-1,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        is_holonomic: bool = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        contrast_fn, score_fn = _gauss_closures(self)
        super().__init__(
            step_size=step_size,
            contrast_fn=contrast_fn,
            score_fn=score_fn,
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            is_holonomic=is_holonomic,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )


def _vector_penalty(contrast_fn, prox_penalty):
    """(contrast_fn, prox_penalty, penalty_fn) of PDSIVA / ADMMIVA (ref: ssspy/bss/iva.py:2233-2262,
    :2295-2324).  The default penalty is ``prox.l21`` over the bins as a ``functools.partial`` that
    leaves ``step_size`` open (the reference wraps it in a local function): ``proxbss.device_prox``
    recognises it, so the default classes run on the device."""
    if contrast_fn is not None and prox_penalty is None:
        raise ValueError("Set prox_penalty.")
    if contrast_fn is None and prox_penalty is not None:
        raise ValueError("Set contrast_fn.")
    if contrast_fn is None:

        def contrast_fn(y: np.ndarray) -> np.ndarray:
            return np.linalg.norm(y, axis=1)

        prox_penalty = functools.partial(prox.l21, axis2=1)

    def penalty_fn(y: np.ndarray) -> float:
        """Sum of contrast function; ``y`` is (n_sources, n_bins, n_frames)."""
        G = contrast_fn(y)  # (n_sources, n_frames)
        return np.sum(G, axis=(0, 1)).item()

    return contrast_fn, prox_penalty, penalty_fn


class PDSIVA(PDSBSS):
    """IVA by primal-dual splitting (ref: ssspy/bss/iva.py:2217-2277)."""

    def __init__(
        self,
        mu1: float = 1,
        mu2: float = 1,
        alpha: float = None,
        relaxation: float = 1,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        prox_penalty: Callable[[np.ndarray, float], np.ndarray] = None,
        callbacks=None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        contrast_fn, prox_penalty, penalty_fn = _vector_penalty(contrast_fn, prox_penalty)
        super().__init__(
            mu1=mu1,
            mu2=mu2,
            alpha=alpha,
            relaxation=relaxation,
            penalty_fn=penalty_fn,
            prox_penalty=prox_penalty,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        self.contrast_fn = contrast_fn


class ADMMIVA(ADMMBSS):
    """IVA by the alternating direction method of multipliers (ref: ssspy/bss/iva.py:2280-2338)."""

    def __init__(
        self,
        rho: float = 1,
        alpha: float = None,
        relaxation: float = 1,
        contrast_fn: Callable[[np.ndarray], np.ndarray] = None,
        prox_penalty: Callable[[np.ndarray, float], np.ndarray] = None,
        callbacks=None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
    ) -> None:
        contrast_fn, prox_penalty, penalty_fn = _vector_penalty(contrast_fn, prox_penalty)
        super().__init__(
            rho=rho,
            alpha=alpha,
            relaxation=relaxation,
            penalty_fn=penalty_fn,
            prox_penalty=prox_penalty,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
        )
        self.contrast_fn = contrast_fn
