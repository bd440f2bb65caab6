"""ILRMA with joint dereverberation (ILRMA-T) on MI355X: 2..8 channels.

R. Ikeshita, N. Ito, T. Nakatani, K. Kinoshita, "Independent low-rank matrix analysis with
decorrelation learning", WASPAA 2019; T. Nakatani et al., Interspeech 2020 (the source-wise
factorisation).  The reference has no such class.  It is ``ConvGaussIVA`` with the low-rank source
model of ``GaussILRMA``: the state of ConvIVA (``convolutional_filter``) and the non-partitioned
``basis`` ``(N, F, n_basis)`` / ``activation`` ``(N, n_basis, T)`` under one objective.

One iteration, from ``Y = W xb`` (the notation of ``conviva``), ``p = domain``:

1. the MM updates of ``GaussILRMA`` on ``|Y|^2``, basis then activation (exponent ``p / (p + 2)``,
   floored; ``ssspy_ilrma_update_basis`` / ``_activation`` in their on-Y form);
2. per (bin, source) ``Sigma_n`` and ``G_n`` as in ConvIVA, with the weights
   ``phi_nft = (sum_k T_nfk V_nkt)^(-2/p)`` formed inside the statistics kernel
   (``ssspy_conviva_statistics_nmf``);
3. the IP1 sweep on ``Q = W[..., :M]``, 4. the composition of ``W``, 5. ``Y = W xb``;
6. power normalisation (``normalization`` ``True`` / ``"power"``): ``psi_n = floor(sqrt(mean_{f,t}
   |y_nft|^2))`` divides ``Y_n`` and all ``Lb`` entries of the rows ``W[f, n, :]``, ``psi_n^p`` divides
   ``basis_n``; ``G`` is untouched.

Loss: ``sum_{n,f} mean_t (|y|^2 / r + (2/p) log TV) - 2 sum_f log|det Q_f|``, ``r = TV^(2/p)``.  With
``diagonal_loading = 0`` and a floor that does not bind it does not increase, and the normalisation
leaves it unchanged.  ``taps = 0`` is ``GaussILRMA`` with IP1.  There is no host path.
"""

import functools
from typing import Callable, List, Optional, Union

import numpy as np

from .. import _device as dv
from .. import _lib, _ops
from ..special.flooring import max_flooring
from ._device_state import Synced
from .conviva import EPS, ConvIVABase

__all__ = ["ConvGaussILRMA"]

_POWER = ("power",)


class ConvGaussILRMA(ConvIVABase):
    """ILRMA with joint dereverberation, Gauss source model.

    Args:
        n_basis: number of NMF bases per source, 1..32.
        taps, delay, diagonal_loading, flooring_fn, scale_restoration, reference_id: as ``ConvIVABase``.
        domain: ``p`` in (0, 2]: the NMF models ``|y|^p``.
        normalization: ``True`` / ``"power"`` or ``False``.
        rng: draws the initial ``basis`` and ``activation`` (``flooring_fn(rng.random(...))``, basis
            first).

    Inputs, outputs, ``convolutional_filter``, ``demix_filter``, ``prediction_filter``, ``apply`` and
    the errors are those of ``ConvIVABase``.  ``convolutional_filter``, ``basis`` ``(n_sources, n_bins,
    n_basis)`` and ``activation`` ``(n_sources, n_basis, n_frames)`` (with the leading mixture axis of a
    batch) can each be given by keyword at the call; each is copied.
    """

    basis = Synced(dv.f64)
    activation = Synced(dv.f64)

    def __init__(
        self,
        n_basis: int,
        taps: int = 5,
        delay: int = 3,
        domain: float = 2,
        diagonal_loading: float = 0.0,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        normalization: Union[bool, str] = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
        rng: Optional[np.random.Generator] = None,
    ) -> None:
        super().__init__(taps=taps, delay=delay, diagonal_loading=diagonal_loading,
                         flooring_fn=flooring_fn, callbacks=callbacks,
                         scale_restoration=scale_restoration, record_loss=record_loss,
                         reference_id=reference_id)
        self.n_basis = self._checked_n_basis(n_basis)
        self.domain = self._checked_domain(domain)
        if type(normalization) is str and normalization == "projection_back":
            raise NotImplementedError(
                "ConvGaussILRMA normalises by power only: projection back per iteration would "
                "re-compose every convolutional filter")
        if type(normalization) is str and normalization not in _POWER:
            raise ValueError("{} is not supported for normalization.".format(normalization))
        self.normalization = normalization
        self.rng = np.random.default_rng() if rng is None else rng

    def __repr__(self) -> str:
        s = ("ConvGaussILRMA(n_basis={}, taps={}, delay={}, domain={}, diagonal_loading={}, "
             "normalization={}, scale_restoration={}, record_loss={}"
             .format(self.n_basis, self.taps, self.delay, self.domain, self.diagonal_loading,
                     self.normalization, self.scale_restoration, self.record_loss))
        if self.scale_restoration:
            s += ", reference_id={}".format(self.reference_id)
        return s + ")"

    @staticmethod
    def _checked_n_basis(n_basis):
        if isinstance(n_basis, bool) or int(n_basis) != n_basis or n_basis < 1:
            raise ValueError("n_basis must be an integer >= 1, got {!r}.".format(n_basis))
        if n_basis > _lib.CONVIVA_MAX_BASIS:
            raise NotImplementedError("ConvGaussILRMA takes up to {} bases, got {}.".format(
                _lib.CONVIVA_MAX_BASIS, n_basis))
        return int(n_basis)

    @staticmethod
    def _checked_domain(domain):
        if isinstance(domain, bool) or not 0 < float(domain) <= 2:
            raise ValueError("domain must be in (0, 2], got {!r}.".format(domain))
        return domain

    def __call__(self, input, n_iter: int = 100, initial_call: bool = True, **kwargs):
        self.n_basis = self._checked_n_basis(self.n_basis)
        self.domain = self._checked_domain(self.domain)
        self._check_shape(input.shape)
        self._check_factors(tuple(input.shape), kwargs)
        return super().__call__(input, n_iter=n_iter, initial_call=initial_call, **kwargs)

    def _check_factors(self, shape, kwargs) -> None:
        """The shapes of factors given by keyword, before anything is uploaded."""
        lead, (M, F, T) = shape[:-3], shape[-3:]
        for name, want in (("basis", lead + (M, F, self.n_basis)),
                           ("activation", lead + (M, self.n_basis, T))):
            if name in kwargs:
                if kwargs[name] is None:
                    raise ValueError("{}=None cannot be given at reset.".format(name))
                if tuple(np.shape(kwargs[name])) != want:
                    raise ValueError("{} must be {}, got {}.".format(
                        name, want, tuple(np.shape(kwargs[name]))))

    def _reset(self, **kwargs) -> None:
        given = {name: kwargs.pop(name) for name in ("basis", "activation") if name in kwargs}
        B, M, F, T = self._X.shape
        # (the draws come before the first launch and in the order of ILRMABase._init_nmf)
        for name, shape in (("basis", (M, F, self.n_basis)), ("activation", (M, self.n_basis, T))):
            if name in given:
                value = np.array(given[name], dtype=np.float64, copy=True)
            else:
                value = np.asarray(self.flooring_fn(self.rng.random(self._lead() + shape)))
            setattr(self, name, value)
        self._ws, self._ws_bytes = _ops.ilrma_workspace(B, M, F, T, self.n_basis, self._X.device)
        super()._reset(**kwargs)

    # -- iterations ------------------------------------------------------------------------------
    def _step(self, floor, data_out=None, logdet_out=None) -> None:
        M, K, p = self.n_channels, self.taps, float(self.domain)
        W = self._W()
        Y = self._current_output()
        basis, activation = self._state_dev("basis"), self._state_dev("activation")
        Q = W[..., :M].clone()  # (data movement only; a copy also with taps = 0)
        if data_out is not None:
            _ops.ilrma_loss_data(Y, None, basis, activation, p, out=data_out)
            _ops.sum_logdet(Q, out=logdet_out)
        _ops.ilrma_update_basis(Y, None, basis, activation, p, floor, self._ws, self._ws_bytes)
        _ops.ilrma_update_activation(Y, None, basis, activation, p, floor, self._ws, self._ws_bytes)
        _ops.conviva_statistics_nmf(self._X, basis, activation, p, K, self.delay,
                                    self.diagonal_loading, self._conv_info, Sigma=self._Sigma,
                                    G=self._G, failed=self._failed)
        _ops.update_by_ip1(Q, self._Sigma, floor, self._info_tensor())
        _ops.conviva_compose(Q, self._G, W, K, self._failed)
        self._state_touch("convolutional_filter")
        self._form_output()
        if self.normalization:
            # Y and the rows of W are divided by the same psi: Y stays W xb to one rounding
            _ops.convilrma_normalize(self._state_dev("output"), W, basis, K, p, floor)
            self._state_touch("convolutional_filter")
            self._state_touch("output")
            self._output_rev = (self._state_rev("convolutional_filter"), self._state_rev("output"))
        self._state_touch("basis")
        self._state_touch("activation")

    def _terms(self, data_out, logdet_out) -> None:
        _ops.ilrma_loss_data(self._current_output(), None, self._state_dev("basis"),
                             self._state_dev("activation"), float(self.domain), out=data_out)
        Q = self._W()[..., :self.n_channels].contiguous()
        _ops.sum_logdet(Q, out=logdet_out)
