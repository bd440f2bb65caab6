"""Independent positive semidefinite tensor analysis (IPSDTA) with block-decomposed bases on MI355X.

Drop-in classes for the reference's ``ssspy.bss.ipsdta`` (ssspy/bss/ipsdta.py:26-1870):
``IPSDTABase``, ``BlockDecompositionIPSDTABase``, ``GaussIPSDTA`` and ``TIPSDTA`` with the MM source
model and the VCD spatial model (``source_algorithm="EM"`` and ``spatial_algorithm="FPI"`` raise
``NotImplementedError`` where the reference does).

The F bins are cut into ``n_blocks`` blocks of ``F // n_blocks`` bins, the last ``F % n_blocks``
of them one bin larger; every (source, frame, block) owns an L x L Hermitian matrix
R = to_psd(sum_k v T).  An iteration rebuilds R three times, as the reference does -- for the basis
statistics, for the activation terms and for the weighted covariance of VCD -- each time inside one
pass over the frames (csrc/ipsdta.hip); the N K C small matrices of the basis step go through the
device operators ``to_psd``, ``gmeanmh``, ``sqrtmh`` and ``invsqrtmh``.  Device limits: 2-8 sources,
block sizes up to 8, 1-32 bases.  A flooring callable that is none of the reference's three is
evaluated on the host on the eigenvalues of those small matrices and once at 0 for the VCD
singularity test.
"""

import functools
from typing import Callable, List, Optional, Union

import numpy as np

from .. import _device as dv
from .. import _lib, _ops
from ..special.flooring import identity, max_flooring
from ..utils.flooring import choose_flooring_fn, device_flooring, host_floor
from ._device_state import Synced
from ._filter_base import DemixingFilterBase
from .base import IterativeMethodBase

__all__ = ["IPSDTABase", "BlockDecompositionIPSDTABase", "GaussIPSDTA", "TIPSDTA"]

spatial_algorithms = ["FPI", "VCD"]
source_algorithms = ["EM", "MM"]
EPS = 1e-10


class IPSDTABase(DemixingFilterBase):
    """Base class of IPSDTA (ref: ssspy/bss/ipsdta.py:26-382)."""

    activation = Synced(dv.f64)

    def __init__(
        self,
        n_basis: int,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[
            Union[Callable[["IPSDTABase"], None], List[Callable[["IPSDTABase"], None]]]
        ] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
        rng: Optional[np.random.Generator] = None,
    ) -> None:
        super().__init__(callbacks=callbacks, record_loss=record_loss)
        self.n_basis = n_basis
        self.flooring_fn = identity if flooring_fn is None else flooring_fn
        self.input = None
        self.scale_restoration = scale_restoration
        if reference_id is None and scale_restoration:
            raise ValueError("Specify 'reference_id' if scale_restoration=True.")
        self.reference_id = reference_id
        self.rng = np.random.default_rng() if rng is None else rng

    def __call__(self, input: np.ndarray, n_iter: int = 100, **kwargs) -> np.ndarray:
        """Separate a frequency-domain multichannel mixture (ref: ssspy/bss/ipsdta.py:96-122)."""
        self._bind_input(input)
        self._reset(**kwargs)
        IterativeMethodBase.__call__(self, n_iter=n_iter)
        return self._finish_call()

    def __repr__(self) -> str:
        s = "IPSDTA(n_basis={}, scale_restoration={}, record_loss={}".format(
            self.n_basis, self.scale_restoration, self.record_loss)
        if self.scale_restoration:
            s += ", reference_id={}".format(self.reference_id)
        return s + ")"

    def separate(self, input: np.ndarray, demix_filter: np.ndarray) -> np.ndarray:
        """y_ij = W_i x_ij (ref: ssspy/bss/ipsdta.py:235-258); NumPy in, NumPy out."""
        batched = input.ndim == 4
        X = dv.to_device(input if batched else input[None], dtype=np.complex128)
        W = dv.to_device(demix_filter if batched else demix_filter[None], dtype=np.complex128)
        Y = dv.to_host(_ops.separate(X, W))
        return Y if batched else Y[0]

    def _reconstruct(self, basis, activation, axis1: int, axis2: int) -> np.ndarray:
        """to_psd(sum_k v_k T_k) for a basis (..., K, C, L, L) -- (..., C, L, L, K) when the matrix
        axes are the second and third from the end -- and an activation (..., K, T): (..., T, C, L, L).
        The floor on the eigenvalues is the instance's.  Matrices up to 16 x 16 with up to
        ``IPSDTA_MAX_BASIS`` bases and a built-in floor go through one kernel, a lane per matrix;
        anything else is summed on the host and handed to ``ssspy_amd.special.to_psd``."""
        T, V = np.asarray(basis), np.asarray(activation)
        nd = T.ndim
        axis1 = nd + axis1 if axis1 < 0 else axis1
        axis2 = nd + axis2 if axis2 < 0 else axis2
        assert (axis1 == nd - 3 and axis2 == nd - 2) or (axis1 == nd - 2 and axis2 == nd - 1)
        basis_last = axis1 == nd - 3
        floor = device_flooring(self.flooring_fn, allow_host=True)
        L, K = T.shape[axis1], V.shape[-2]
        if (host_floor(floor) is None and L <= _lib.RT_MAX_SOURCES
                and 1 <= K <= _lib.IPSDTA_MAX_BASIS):
            R = _ops.ipsdta_reconstruct(dv.to_device(T, dtype=np.complex128),
                                        dv.to_device(V, dtype=np.float64), floor, basis_last)
            return dv.to_host(R)
        from ..special.psd import to_psd

        if basis_last:
            T = np.moveaxis(T, -1, -4)
        na = np.newaxis
        R = np.sum(T[..., :, na, :, :, :] * V[..., :, :, na, na, na], axis=-5)
        return to_psd(R, flooring_fn=self.flooring_fn)

    def reconstruct_psdtf(self, basis: np.ndarray, activation: np.ndarray, axis1: int = -2,
                          axis2: int = -1) -> np.ndarray:
        """R_nt = to_psd(sum_k v_nkt T_nk) (ref: ssspy/bss/ipsdta.py:260-300).

        Args:
            basis: (n_sources, n_basis, n_bins, n_bins), or (n_sources, n_bins, n_bins, n_basis)
                with ``axis1=-3, axis2=-2`` (``1, 2``).
            activation: (n_sources, n_basis, n_frames).

        Returns:
            (n_sources, n_frames, n_bins, n_bins), exactly Hermitian.  Up to 16 bins the block kernel
            of ``reconstruct_block_decomposition_psdtf`` runs with one block; above, the sum is formed
            on the host and ``ssspy_amd.special.to_psd`` floors it, with the sizes that function takes.
        """
        T = np.asarray(basis)
        nd = T.ndim
        a1 = nd + axis1 if axis1 < 0 else axis1
        a2 = nd + axis2 if axis2 < 0 else axis2
        assert (a1 == 1 and a2 == 2) or (a1 == 2 and a2 == 3)
        # one block that spans every bin: (n_sources, n_basis, 1, n_bins, n_bins)
        T = T[:, np.newaxis] if a1 == 1 else T[:, :, np.newaxis]
        return self._reconstruct(T, activation, a1 + 1, a2 + 1)[:, :, 0]

    def normalize_psdtf(self) -> None:
        """T / tr T, V tr T per (source, basis) (ref: ssspy/bss/ipsdta.py:306-317).  Host only: a
        pass over the n_sources x n_basis matrices, through the ``basis`` and ``activation``
        attributes."""
        assert self.source_normalization, "Set source_normalization."
        T, V = self.basis, self.activation
        trace = np.trace(T, axis1=-2, axis2=-1).real
        self.basis = T / trace[:, :, np.newaxis, np.newaxis]
        self.activation = V * trace[:, :, np.newaxis]

    def update_once(self) -> None:
        raise NotImplementedError("Implement 'update_once' method.")

    def compute_loss(self) -> float:
        raise NotImplementedError("Implement 'compute_loss' method.")

    def compute_logdet(self, demix_filter: np.ndarray) -> np.ndarray:
        """log|det W_i| per bin (ref: ssspy/bss/ipsdta.py:327-339)."""
        return np.linalg.slogdet(demix_filter)[1]


class BlockDecompositionIPSDTABase(IPSDTABase):
    """IPSDTA with block decomposition of the bases (ref: ssspy/bss/ipsdta.py:385-697)."""

    def __init__(
        self,
        n_basis: int,
        n_blocks: int,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[
            Union[
                Callable[["BlockDecompositionIPSDTABase"], None],
                List[Callable[["BlockDecompositionIPSDTABase"], None]],
            ]
        ] = None,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
        rng: Optional[np.random.Generator] = None,
    ) -> None:
        super().__init__(
            n_basis=n_basis,
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            scale_restoration=scale_restoration,
            record_loss=record_loss,
            reference_id=reference_id,
            rng=rng,
        )
        self.n_blocks = n_blocks

    def __repr__(self) -> str:
        return "IPSDTA(" + self._repr_fields()

    def _repr_fields(self, extra: str = "") -> str:
        s = "n_basis={}, n_blocks={}".format(self.n_basis, self.n_blocks) + extra
        s += ", scale_restoration={}, record_loss={}".format(self.scale_restoration, self.record_loss)
        if self.scale_restoration:
            s += ", reference_id={}".format(self.reference_id)
        return s + ")"

    @property
    def n_remains(self) -> int:
        if not hasattr(self, "n_bins"):
            raise AttributeError("Since n_bins is not defined, n_remains cannot be computed.")
        return self.n_bins % self.n_blocks

    # -- basis: (N, K, C, L, L), or the pair (low, high) when n_bins % n_blocks > 0; on the device a
    # list of (B, N, K, C, L, L) tensors, one per partition
    @property
    def basis(self):
        if "_basis_host" not in self.__dict__ and "_basis_dev" not in self.__dict__:
            raise AttributeError("'{}' object has no attribute 'basis'".format(type(self).__name__))
        if self.__dict__.get("_basis_host") is None:
            self._check_device_errors()
            mats = [dv.to_host(t) for t in self.__dict__["_basis_dev"]]
            if not self._batched:
                mats = [m[0] for m in mats]
            self.__dict__["_basis_host"] = tuple(mats) if len(mats) > 1 else mats[0]
        return self.__dict__["_basis_host"]

    @basis.setter
    def basis(self, value):
        self.__dict__["_basis_host"] = value
        self.__dict__.pop("_basis_dev", None)

    def _basis_parts(self):
        """[(basis tensor, first bin, first block)] of the partitions, uploading if needed."""
        if "_basis_dev" not in self.__dict__:
            host = self.__dict__["_basis_host"]
            mats = list(host) if type(host) is tuple else [host]
            mats = [np.asarray(m) if self._batched else np.asarray(m)[None] for m in mats]
            self.__dict__["_basis_dev"] = [dv.to_device(m, dtype=np.complex128) for m in mats]
        tensors = self.__dict__["_basis_dev"]
        L = self.n_bins // self.n_blocks
        n_low = self.n_blocks - self.n_remains
        parts = [(tensors[0], 0, 0)]
        if len(tensors) > 1:
            parts.append((tensors[1], n_low * L, n_low))
        return parts

    def _set_basis_dev(self, tensors) -> None:
        self.__dict__["_basis_dev"] = list(tensors)
        self.__dict__["_basis_host"] = None

    def _check_limits(self, n_sources: int, n_bins: int) -> None:
        name = type(self).__name__
        if not 2 <= n_sources <= _lib.IPSDTA_MAX_SOURCES:
            raise NotImplementedError("{} takes 2 to {} sources, got {}.".format(
                name, _lib.IPSDTA_MAX_SOURCES, n_sources))
        if not 1 <= self.n_blocks <= n_bins:
            raise ValueError("n_blocks must be in [1, n_bins], got {}.".format(self.n_blocks))
        largest = n_bins // self.n_blocks + (1 if n_bins % self.n_blocks else 0)
        if largest > _lib.IPSDTA_MAX_BLOCK:
            raise NotImplementedError("{} takes block sizes up to {}, got {}.".format(
                name, _lib.IPSDTA_MAX_BLOCK, largest))
        if not 1 <= self.n_basis <= _lib.IPSDTA_MAX_BASIS:
            raise NotImplementedError("{} takes n_basis 1 to {}, got {}.".format(
                name, _lib.IPSDTA_MAX_BASIS, self.n_basis))

    def _reset(self, flooring_fn="self", **kwargs) -> None:
        """ref: ssspy/bss/ipsdta.py:464-510."""
        assert self._has_input(), "Specify data!"
        flooring_fn = choose_flooring_fn(flooring_fn, method=self)
        for key, value in kwargs.items():
            setattr(self, key, value)
        B, N, F, T = self._X.shape
        self._check_limits(N, F)
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
        self._init_block_decomposition_psdtf(flooring_fn=flooring_fn, rng=self.rng)

    def _draw_psdtf(self, flooring_fn, rng, n_mixtures: int):
        """The random initialisation (host only): per mixture the reference's draws in its order and
        shapes -- low blocks, high blocks, activations (ref: ssspy/bss/ipsdta.py:545-567) -- for
        whichever of ``basis`` / ``activation`` is not set yet.  Returns (basis or None, activation or
        None) with a leading mixture axis."""
        N, K, T = self.n_sources, self.n_basis, self.n_frames
        n_blocks, n_remains = self.n_blocks, self.n_remains
        L = self.n_bins // n_blocks
        want_basis = not hasattr(self, "basis")
        want_activation = not self._state_has("activation")
        low, high, act = [], [], []
        for _ in range(n_mixtures):
            if want_basis:
                low.append(rng.random((N, K, n_blocks - n_remains, L))[..., np.newaxis]
                           * np.eye(L, dtype=np.complex128))
                if n_remains > 0:
                    high.append(rng.random((N, K, n_remains, L + 1))[..., np.newaxis]
                                * np.eye(L + 1, dtype=np.complex128))
            if want_activation:
                act.append(flooring_fn(rng.random((N, K, T))))
        basis = None
        if want_basis:
            basis = (np.stack(low), np.stack(high)) if n_remains > 0 else np.stack(low)
        return basis, (np.stack(act) if want_activation else None)

    def _init_block_decomposition_psdtf(self, flooring_fn="self", rng=None) -> None:
        """ref: ssspy/bss/ipsdta.py:512-575; one draw per mixture, in the reference's order."""
        n_remains = self.n_remains
        flooring_fn = choose_flooring_fn(flooring_fn, method=self)
        if rng is None:
            rng = np.random.default_rng()
        basis, activation = self._draw_psdtf(flooring_fn, rng, self._X.shape[0])
        if basis is not None:
            if n_remains > 0:
                self.basis = basis if self._batched else tuple(m[0] for m in basis)
            else:
                self.basis = basis if self._batched else basis[0]
        else:  # (to avoid overwriting what was given)
            given = self.basis
            if n_remains > 0:
                self.basis = tuple(np.array(t, dtype=np.complex128, copy=True) for t in given)
            else:
                self.basis = np.array(given, dtype=np.complex128, copy=True)
        if activation is not None:
            self.activation = activation if self._batched else activation[0]
        else:
            self.activation = np.array(self.activation, dtype=np.float64, copy=True)
        if self.source_normalization:
            self.normalize_block_decomposition_psdtf()

    def reconstruct_block_decomposition_psdtf(self, basis, activation, axis1: int = -2,
                                              axis2: int = -1):
        """R_ntc = to_psd(sum_k v_nkt T_nkc) per block (ref: ssspy/bss/ipsdta.py:584-664): the
        matrices the frame passes form and keep to themselves, handed out.

        Args:
            basis: (n_sources, n_basis, n_blocks, n_neighbors, n_neighbors), or (n_sources,
                n_blocks, n_neighbors, n_neighbors, n_basis) with ``axis1=-3, axis2=-2``; or the
                pair ``(basis_low, basis_high)`` when ``n_bins % n_blocks > 0``.
            activation: (n_sources, n_basis, n_frames).

        Returns:
            (n_sources, n_frames, n_blocks, n_neighbors, n_neighbors), exactly Hermitian; a pair for
            a pair.
        """
        if type(basis) is tuple:
            assert self.n_remains > 0, "n_remains is expected to be positive."
            T_low, T_high = basis
            return (self._reconstruct(T_low, activation, axis1, axis2),
                    self._reconstruct(T_high, activation, axis1, axis2))
        return self._reconstruct(basis, activation, axis1, axis2)

    def normalize_block_decomposition_psdtf(self, axis1: int = -2, axis2: int = -1) -> None:
        """T / tr, V tr with the traces summed over both partitions (ref: ipsdta.py:666-697)."""
        assert self.source_normalization, "Set source_normalization."
        parts = self._basis_parts()
        _ops.ipsdta_normalize(parts[0][0], parts[1][0] if len(parts) > 1 else None,
                              self._state_dev("activation"))
        self._set_basis_dev([p[0] for p in parts])
        self._state_touch("activation")

    # -- the stages of an iteration
    def _dof(self):
        return None

    def _weight(self, parts):
        """pi (B, N, T) of the t model from a pass of its own over the frames; None for Gauss."""
        if self._dof() is None:
            return None
        quad, logdet = _ops.ipsdta_quadratic(self._X, self._state_dev("demix_filter"), parts,
                                             self._state_dev("activation"), self.n_blocks)
        return _ops.ipsdta_weight_loss(quad, logdet, self.n_blocks - self.n_remains, self.n_bins,
                                       _lib.SOURCE_T, self._dof(), want_pi=True)

    def _on_host(self, tensor, fn):
        """``fn`` on the host copy of a device stack, one mixture at a time."""
        host = dv.to_host(tensor)
        out = np.stack([np.asarray(fn(h)) for h in host])
        return dv.to_device(out, dtype=np.complex128, dev=tensor.device)

    def _psd(self, A, floor):
        if host_floor(floor) is not None:
            from ..special.psd import to_psd

            return self._on_host(A, functools.partial(to_psd, flooring_fn=host_floor(floor)))
        return _ops.to_psd_dev(A, floor)

    def _invsqrt(self, A, floor):
        if host_floor(floor) is not None:
            from ..linalg import invsqrtmh

            return self._on_host(A, functools.partial(invsqrtmh, flooring_fn=host_floor(floor)))
        return _ops.sqrtmh_dev(A, inverse=True, flooring=floor)

    def update_source_model(self, flooring_fn="self") -> None:
        """ref: ssspy/bss/ipsdta.py:842-866, :1356-1380."""
        flooring_fn = choose_flooring_fn(flooring_fn, method=self)
        if self.source_algorithm == "MM":
            self.update_source_model_mm(flooring_fn=flooring_fn)
        else:
            raise NotImplementedError("Not support {}.".format(self.source_algorithm))
        if self.source_normalization:
            self.normalize_block_decomposition_psdtf()

    def update_source_model_mm(self, flooring_fn="self") -> None:
        flooring_fn = choose_flooring_fn(flooring_fn, method=self)
        self.update_basis_mm(flooring_fn=flooring_fn)
        self.update_activation_mm()

    def update_basis_mm(self, flooring_fn="self") -> None:
        """Gauss: T <- to_psd(to_psd(P)^-1 # to_psd(T Q T)) (ref: ipsdta.py:889-973);
        t: T <- to_psd(T Q' (Q' T P T Q')^-1/2 Q' T), Q' = to_psd(Q)^1/2 (ref: ipsdta.py:1404-1530)."""
        floor = self._resolve_floor(flooring_fn)
        parts = self._basis_parts()
        X, W, V = self._X, self._state_dev("demix_filter"), self._state_dev("activation")
        pi = self._weight(parts)
        new = []
        for part in parts:
            T = part[0]
            P, Q = _ops.ipsdta_basis_statistics(X, W, part, V, pi, self.n_blocks)
            if self._dof() is None:
                TQT = _ops.matmul3(T, Q, T)
                G = _ops.gmeanmh_dev(self._psd(P, floor), self._psd(TQT, floor), type=2)
            else:
                Qh = _ops.sqrtmh_dev(self._psd(Q, floor))
                mid = _ops.matmul3(_ops.matmul3(Qh, T, P), T, Qh)
                mid = self._invsqrt(self._psd(mid, floor), floor)
                G = _ops.matmul3(_ops.matmul3(T, Qh, mid), Qh, T)
            new.append(self._psd(G, floor))
        self._set_basis_dev(new)

    def update_activation_mm(self) -> None:
        """V <- V sqrt(num / den) (ref: ssspy/bss/ipsdta.py:975-1033, :1532-1632)."""
        parts = self._basis_parts()
        X, W, V = self._X, self._state_dev("demix_filter"), self._state_dev("activation")
        num, den = _ops.ipsdta_activation_terms(X, W, parts, V, self._weight(parts), self.n_blocks)
        _ops.ipsdta_activation(V, num, den)
        self._state_touch("activation")

    def update_spatial_model(self, flooring_fn="self") -> None:
        """ref: ssspy/bss/ipsdta.py:1035-1056, :1634-1655."""
        flooring_fn = choose_flooring_fn(flooring_fn, method=self)
        if self.spatial_algorithm == "VCD":
            self.update_spatial_model_vcd(flooring_fn=flooring_fn)
        else:
            raise NotImplementedError("Not support {}.".format(self.spatial_algorithm))

    def update_spatial_model_vcd(self, flooring_fn="self") -> None:
        """ref: ssspy/bss/ipsdta.py:1058-1147, :1657-1777."""
        floor = self._resolve_floor(flooring_fn)
        threshold = float(np.asarray(host_floor(floor)(0))) if host_floor(floor) is not None else floor[1]
        parts = self._basis_parts()
        X, W, V = self._X, self._state_dev("demix_filter"), self._state_dev("activation")
        pi = self._weight(parts)
        # (every partition's covariance is formed with the filters the sweep starts from)
        covs = [_ops.ipsdta_weighted_covariance(X, W, part, V, pi, self.n_blocks) for part in parts]
        for part, cov in zip(parts, covs):
            _ops.ipsdta_vcd(W, cov, part[1], threshold, self._info_tensor())
        self._state_touch("demix_filter")

    def update_once(self, flooring_fn="self") -> None:
        """ref: ssspy/bss/ipsdta.py:820-840, :1335-1354."""
        flooring_fn = choose_flooring_fn(flooring_fn, method=self)
        self.update_source_model(flooring_fn=flooring_fn)
        self.update_spatial_model(flooring_fn=flooring_fn)

    def compute_loss(self) -> float:
        """ref: ssspy/bss/ipsdta.py:1149-1227, :1779-1869."""
        parts = self._basis_parts()
        W = self._state_dev("demix_filter")
        quad, logdet = _ops.ipsdta_quadratic(self._X, W, parts, self._state_dev("activation"),
                                             self.n_blocks)
        data = dv.empty((self._X.shape[0],), dv.f64, self._X.device)
        dof = self._dof()
        _ops.ipsdta_weight_loss(quad, logdet, self.n_blocks - self.n_remains, self.n_bins,
                                _lib.SOURCE_GAUSS if dof is None else _lib.SOURCE_T,
                                0.0 if dof is None else dof, loss=data)
        return self._host_loss(data, _ops.sum_logdet(W))


class GaussIPSDTA(BlockDecompositionIPSDTABase):
    """IPSDTA on the Gaussian distribution (ref: ssspy/bss/ipsdta.py:700-1227)."""

    def __init__(
        self,
        n_basis: int,
        n_blocks: int,
        source_algorithm: str = "MM",
        spatial_algorithm: str = "VCD",
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[
            Union[Callable[["GaussIPSDTA"], None], List[Callable[["GaussIPSDTA"], None]]]
        ] = None,
        source_normalization: Optional[Union[bool, str]] = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
        rng: Optional[np.random.Generator] = None,
    ) -> None:
        super().__init__(n_basis, n_blocks, flooring_fn, callbacks, scale_restoration, record_loss,
                         reference_id, rng)
        assert source_algorithm in source_algorithms, "Not support {}.".format(source_algorithms)
        assert spatial_algorithm in spatial_algorithms, "Not support {}.".format(spatial_algorithms)
        self.source_algorithm = source_algorithm
        self.spatial_algorithm = spatial_algorithm
        self.source_normalization = source_normalization

    def __repr__(self) -> str:
        return "GaussIPSDTA(" + self._repr_fields(
            ", source_algorithm={}, spatial_algorithm={}, source_normalization={}".format(
                self.source_algorithm, self.spatial_algorithm, self.source_normalization))

    def _reset(self, **kwargs) -> None:
        """ref: ssspy/bss/ipsdta.py:800-818."""
        super()._reset(**kwargs)
        if self.spatial_algorithm == "FPI":
            if not hasattr(self, "fixed_point"):
                self.fixed_point = np.ones((self.n_sources, self.n_bins), dtype=np.complex128)
            else:
                self.fixed_point = self.fixed_point.copy()
            raise NotImplementedError("IPSDTA with fixed-point iteration is not supported.")


class TIPSDTA(BlockDecompositionIPSDTABase):
    """IPSDTA on Student's t distribution (ref: ssspy/bss/ipsdta.py:1230-1869)."""

    def __init__(
        self,
        n_basis: int,
        n_blocks: int,
        dof: float,
        source_algorithm: str = "MM",
        spatial_algorithm: str = "VCD",
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[
            Union[Callable[["GaussIPSDTA"], None], List[Callable[["GaussIPSDTA"], None]]]
        ] = None,
        source_normalization: Optional[Union[bool, str]] = True,
        scale_restoration: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
        rng: Optional[np.random.Generator] = None,
    ) -> None:
        super().__init__(n_basis, n_blocks, flooring_fn, callbacks, scale_restoration, record_loss,
                         reference_id, rng)
        assert source_algorithm in source_algorithms, "Not support {}.".format(source_algorithm)
        assert spatial_algorithm in spatial_algorithms, "Not support {}.".format(spatial_algorithm)
        self.dof = dof
        self.source_algorithm = source_algorithm
        self.source_normalization = source_normalization
        self.spatial_algorithm = spatial_algorithm

    def __repr__(self) -> str:
        return "TIPSDTA(" + self._repr_fields(
            ", dof={}, source_algorithm={}, spatial_algorithm={}, source_normalization={}".format(
                self.dof, self.source_algorithm, self.spatial_algorithm, self.source_normalization))

    def _dof(self):
        return float(self.dof)
