"""What ILRMA and AuxIVA share: a demixing-filter state or the separated spectrogram it implies.

Both families keep either the filters W (IP / IP2) or only ``output`` (ISS / ISS2 / IPA, as the
reference does); scale restoration, the implied-filter route and the tracked log-determinant of
the ISS state are the same for both and live here.
"""

import numpy as np

from .. import _device as dv
from .. import _lib, _ops, _routes
from ..utils.flooring import choose_flooring_fn, device_flooring
from ..utils.select_pair import resolve_pairs
from ._device_state import DeviceStateMixin, Synced
from .base import IterativeMethodBase

_IP1 = ("IP", "IP1")
_ISS1 = ("ISS", "ISS1")
_IP2 = ("IP2",)
_ISS2 = ("ISS2",)
_IPA = ("IPA",)
_PROJECTION_BACK = ("projection_back",)
_MDP = ("minimal_distortion_principle",)


def filter_logdet(demix_filter):
    """log|det W_i| per bin, the ``compute_logdet`` of IVABase and ILRMABase (ref:
    ssspy/bss/iva.py:224-236, ilrma.py:524-536).  A NumPy argument is the reference's own line,
    ``numpy.linalg.slogdet`` on the host.  A complex128 torch tensor on the device, (n_bins,
    n_sources, n_sources) or with a leading mixture axis, goes through one LU per lane there and a
    float64 tensor of the leading shape comes back (``-inf`` for a singular filter)."""
    if type(demix_filter).__module__.split(".")[0] != "torch":
        return np.linalg.slogdet(demix_filter)[1]
    W = demix_filter
    limit = _lib.RT_MAX_SOURCES
    if (not W.is_cuda or W.dtype != dv.c128 or W.ndim not in (3, 4) or W.shape[-1] != W.shape[-2]
            or not 1 <= W.shape[-1] <= limit):
        raise NotImplementedError(
            "compute_logdet on the device takes a complex128 tensor (n_bins, n, n) or (n_mixtures, "
            "n_bins, n, n) on a HIP device with n in 1..{}, got {} {} on {} (convert to NumPy for "
            "the host form)".format(limit, W.dtype, tuple(W.shape), W.device))
    return _ops.logdet(W.contiguous())


class DemixingFilterBase(DeviceStateMixin, IterativeMethodBase):
    """State handling shared by ILRMABase and IVABase."""

    demix_filter = Synced(dv.c128)
    output = Synced(dv.c128)

    def _resolve_floor(self, flooring_fn):
        if type(flooring_fn) is str and flooring_fn == "self":
            return self._floor
        return device_flooring(choose_flooring_fn(flooring_fn, method=self), allow_host=True)

    def _uses_filter(self) -> bool:
        return not self._state_is_none("demix_filter")

    def _finish_call(self):
        """The tail of ``__call__``: scale restoration, output = W x on a filter state, the result."""
        if self.scale_restoration:
            self.restore_scale()
        if self._uses_filter():
            self._state_set_dev("output", _ops.separate(self._X, self._state_dev("demix_filter")))
        return self._final_output()

    # -- the ISS state ---------------------------------------------------------------------------
    def _implied_route_wanted(self) -> bool:
        """Whether this configuration reads the mixture through the filters its output implies."""
        return False

    def _reset_output_state(self) -> None:
        """ISS / ISS2 / IPA keep only ``output``: drop the filters, keep what the route and the
        loss need of them."""
        self._logdet_cache = None
        self._implied = None
        self._amp_reset()
        if 2 <= self._X.shape[1] <= 4 and self._implied_route_wanted():
            # the filters the output state implies (output = W x), kept next to it: the iterations
            # read the mixture through them (_implied_step).  Up to 4 sources, where the passes over
            # (X, W) are the tuned IP1 ones (8 sources, 16 mixtures: ISS2 4.0 against 2.9 ms on Y);
            # from 2, where the tracked congruence exists.  W U W^H rounds like eps |W|^2 |U| where
            # the direct sum over Y rounds like eps |y|^2: how far the product can round is measured
            # by every launch that forms it and the route is left past its bound (_amp_exceeded)
            self._implied = (self._state_dev("demix_filter").clone(), self._state_rev("output"))
        if self.spatial_algorithm in _ISS1 + _ISS2 + _IPA:
            if self.record_loss:  # (else nothing reads the log-determinant: no tracker)
                # sum_i log|det W_i| of the filters the ISS state stops carrying, as (tensor,
                # revision of `output` it describes): the fused sweep and the power normalisation
                # move it along, so compute_loss() need not rebuild W from Y X^H
                self._logdet_cache = (_ops.sum_logdet(self._state_dev("demix_filter")),
                                      self._state_rev("output"))
            self.demix_filter = None

    def _tracked_logdet(self):
        """The tracked sum_i log|det W_i| if it describes the current output, else None."""
        cache = getattr(self, "_logdet_cache", None)
        if cache is not None and cache[1] == self._state_rev("output"):
            return cache[0]
        return None

    def _restamp_logdet(self, tracked) -> None:
        self._logdet_cache = None if tracked is None else (tracked, self._state_rev("output"))

    # -- the implied-filter route (round 5) ----------------------------------------------------------
    def _implied_filter(self):
        """W with output = W x while nothing else rewrote ``output`` since, else None."""
        kept = getattr(self, "_implied", None)
        if (kept is None or kept[1] != self._state_rev("output")
                or not _routes.get("implied_filter")):
            return None
        return kept[0]

    def _fill_output_from_implied_filter(self) -> None:
        _ops.separate(self._X, self._implied[0], out=self._state()["output"]["dev"])

    def _leave_implied_route(self) -> None:
        """Form Y = W x now and go on with the iterations that rewrite it (the reference's)."""
        W = self._implied[0]
        self._state_dev("output")  # (runs the deferred fill)
        if getattr(self, "_logdet_cache", None) is not None:  # (the on-Y updates move it along)
            self._logdet_cache = (_ops.sum_logdet(W), self._state_rev("output"))
        self._implied = None

    def _spare(self, name, like):
        """The buffer kept as ``name`` if it has the shape of ``like`` and is not ``like`` itself,
        else a fresh one: the other half of a ping-pong pair."""
        spare = getattr(self, name, None)
        if spare is None or spare.shape != like.shape or spare.data_ptr() == like.data_ptr():
            spare = dv.empty(tuple(like.shape), dv.c128, like.device)
        return spare

    def _spatial_transform(self, Vc, floor):
        """Update matrices G (B, F, N, N) of an ISS / ISS2 / IPA step from the per-bin statistics
        Vc (B, F, N, N, N) (overwritten by IPA)."""
        if self.spatial_algorithm in _ISS1:
            return _ops.iss1_transform(Vc, floor)
        if self.spatial_algorithm in _ISS2:
            pairs = resolve_pairs(getattr(self, "pair_selector", None), Vc.shape[-1])
            return _ops.iss2_transform(Vc, pairs, floor, self._info_tensor())
        return _ops.ipa_sweep(Vc, self.lqpqm_normalization, self.newton_iter, floor,
                              self._info_tensor(), newton_ws=self._newton_words(Vc.device),
                              not_converged=self._newton_counter())

    def _implied_step(self, U, floor, normalize=None) -> None:
        """One ISS / ISS2 / IPA step on the route from the weighted covariances U (B, F, N, N, N) of
        the MIXTURE: statistics W U W^H (tracked), G, W <- G W into the spare, ``normalize(W)`` if
        given, ``output`` deferred (formed when somebody reads it, _state_defer)."""
        W = self._implied_filter()
        self._Vc = self._spare("_Vc", U)
        tracked = self._amp_tracked(self._C())
        _ops.covariance_congruence(U, W, self._Vc, tracked=tracked)
        self._amp_launched(tracked)
        G = self._spatial_transform(self._Vc, floor)
        spare = self._spare("_implied_spare", W)
        _ops.compose_filters(G, W, spare)
        if normalize is not None:
            normalize(spare)
        self._state_defer("output", self._fill_output_from_implied_filter)
        self._implied, self._implied_spare = (spare, self._state_rev("output")), W

    # -- scale restoration ------------------------------------------------------------------
    def restore_scale(self) -> None:
        """ref: ssspy/bss/ilrma.py:538-555, ssspy/bss/iva.py:238-257."""
        scale_restoration = self.scale_restoration
        assert scale_restoration, "Set self.scale_restoration=True."
        if type(scale_restoration) is bool:
            scale_restoration = _PROJECTION_BACK[0]
        if scale_restoration in _PROJECTION_BACK:
            self.apply_projection_back()
        elif scale_restoration in _MDP:
            self.apply_minimal_distortion_principle()
        else:
            raise ValueError("{} is not supported for scale restoration.".format(scale_restoration))

    def apply_projection_back(self) -> None:
        """ref: ssspy/bss/ilrma.py:557-565, :1969-1979; ssspy/bss/iva.py:259-267, :2194-2204;
        algorithm/projection_back.py:87-121."""
        assert self.scale_restoration, "Set self.scale_restoration=True."
        info = self._info_tensor()
        if self._uses_filter():
            W = self._state_dev("demix_filter")
            _ops.projection_back_filter(W, self.reference_id, info)
            self._state_touch("demix_filter")
            self._state_set_dev("output", _ops.separate(self._X, W))
        elif self._implied_filter() is not None and self.reference_id is not None:
            # the same scales from the filters the output state implies: one pass instead of four
            W = self._implied_filter().clone()
            _ops.projection_back_filter(W, self.reference_id, info)
            self._state_set_dev("output", _ops.separate(self._X, W))
            self._implied = (W, self._state_rev("output"))
        else:
            Y = self._state_dev("output")
            XY = _ops.cross_covariance(self._X, Y)
            YY = _ops.cross_covariance(Y, Y)
            G = _ops.projection_back_scale(XY, YY, self.reference_id, info)
            _ops.separate(Y, G, out=Y)
            self._state_touch("output")

    def apply_minimal_distortion_principle(self) -> None:
        """Per (bin, source) scale z = <y, x_ref> / <y, y>, output conj(z) y; with a filter state the
        filter is re-fitted as Y X^H (X X^H)^-1 like the reference.
        ref: ssspy/bss/ilrma.py:567-579, :1981-1989; ssspy/bss/iva.py:269-281, :2206-2214;
        algorithm/minimal_distortion_principle.py:6-43."""
        assert self.scale_restoration, "Set self.scale_restoration=True."
        filt = self._uses_filter()
        if self.reference_id is None:
            # reachable only by clearing the attribute after construction; as in the reference the
            # estimate gains a leading channel axis (minimal_distortion_principle.py:34-35) and a
            # filter state cannot take that shape
            if filt:
                raise ValueError("reference_id=None needs the output state (ISS / IPA), not filters.")
            from ..algorithm import minimal_distortion_principle as _mdp

            Y, X = dv.to_host(self._state_dev("output")), dv.to_host(self._X)
            out = np.stack([_mdp(y, reference=x, reference_id=None) for y, x in zip(Y, X)])
            self.output = out if self._batched else out[0]
            return
        if filt:
            Y = _ops.separate(self._X, self._state_dev("demix_filter"))
        else:
            Y = self._state_dev("output")
        G = _ops.mdp_scale(_ops.cross_covariance(Y, self._X), _ops.cross_covariance(Y, Y),
                           self.reference_id)
        _ops.separate(Y, G, out=Y)
        if filt:
            W = _ops.demix_from_covariance(_ops.cross_covariance(Y, self._X), self._C(),
                                           self._info_tensor())
            self._state_set_dev("demix_filter", W)
            self._state_set_dev("output", Y)
        else:
            self._state_touch("output")
