"""Complex angular central Gaussian mixture model (cACGMM) on the HIP device.

Counterpart of ``ssspy.bss.cacgmm`` (CACGMMBase, CACGMM): mask-based separation by an EM algorithm
on the direction vectors z = x / ||x||.  The E and the M step evaluate the quadratic forms
z^H B^-1 z with the same B, so one iteration is one pass over the unit mixture
(``_ops.cacgmm_frame_pass``: the sums of the posteriors, the weighted outer products and the loss of
the parameters it was given) and one per-(source, bin) step (``_ops.cacgmm_parameter_step``).  The
posterior is formed only when somebody reads it; permutation alignment runs once per call, on the
device for 2..8 sources (csrc/permutation.hip, route ``device_alignment``) and on the host for 1 or
9..16 (``ssspy_amd.algorithm.permutation_alignment``).

On the device: 2..8 channels, 1..16 sources, ``flooring_fn`` None / ``max_flooring`` /
``add_flooring`` (possibly a ``functools.partial`` with ``eps``); anything else raises
``NotImplementedError``.
"""

import functools
from typing import Callable, List, Optional, Union

import numpy as np

from .. import _device as dv
from .. import _lib, _ops, _routes
from ..algorithm.permutation_alignment import (
    correlation_based_permutation_solver,
    device_correlation_permutation,
    device_score_permutation,
    score_based_permutation_solver,
)
from ..special.flooring import identity, max_flooring
from ..utils.flooring import choose_flooring_fn, device_flooring
from ._device_state import DeviceStateMixin, Synced
from .base import IterativeMethodBase

__all__ = ["CACGMMBase", "CACGMM"]

EPS = 1e-10
MIN_CHANNELS, MAX_CHANNELS, MAX_SOURCES = 2, 8, 16


class CACGMMBase(DeviceStateMixin, IterativeMethodBase):
    """Base class of cACGMM: arguments, attributes and initialisation of the reference's
    ``CACGMMBase`` (ssspy/bss/cacgmm.py:21-420).

    Args:
        n_sources: number of components; the number of channels when ``None``.
        flooring_fn: ``None``, ``max_flooring`` or ``add_flooring`` (a ``functools.partial`` with
            ``eps`` is recognised).
        callbacks: callable or list of callables ``f(method)``.
        record_loss: record the loss before the first and after every iteration.
        rng: ``numpy.random.Generator`` the initial parameters are drawn from.
    """

    unit_input = Synced(dv.c128)
    mixing = Synced(dv.f64)
    covariance = Synced(dv.c128)
    posterior = Synced(dv.f64)
    output = Synced(dv.c128)

    def __init__(
        self,
        n_sources: Optional[int] = None,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        record_loss: bool = True,
        rng: Optional[np.random.Generator] = None,
    ) -> None:
        self.normalization: bool
        self.permutation_alignment: Union[bool, str]

        super().__init__(callbacks=callbacks, record_loss=record_loss)

        self.n_sources = n_sources
        self.flooring_fn = identity if flooring_fn is None else flooring_fn
        self.rng = np.random.default_rng() if rng is None else rng

    def __call__(self, input, n_iter: int = 100, initial_call: bool = True, **kwargs):
        self._bind_input(input)
        self._reset(**kwargs)

        raise NotImplementedError("Implement '__call__' method.")

    def __repr__(self) -> str:
        s = "CACGMM("
        if self.n_sources is not None:
            s += "n_sources={n_sources}, "
        s += "record_loss={record_loss}"
        s += ")"
        return s.format(**self.__dict__)

    # -- device plumbing -------------------------------------------------------------------
    def _floor(self, flooring_fn="self"):
        """``(kind, eps)`` of the flooring function a method was given."""
        return device_flooring(choose_flooring_fn(flooring_fn, method=self), what="CACGMM")

    def _reset(self, flooring_fn="self", **kwargs) -> None:
        """Unit input and initial parameters (ssspy/bss/cacgmm.py:116-191)."""
        assert self._has_input(), "Specify data!"

        floor = self._floor(flooring_fn)

        for key in kwargs.keys():
            setattr(self, key, kwargs[key])

        n_channels, n_bins, n_frames = self._X.shape[1:]
        n_sources = n_channels if self.n_sources is None else self.n_sources
        if n_channels < MIN_CHANNELS or n_channels > MAX_CHANNELS:
            raise NotImplementedError(
                "CACGMM runs on the device for {}..{} channels, got n_channels={}".format(
                    MIN_CHANNELS, MAX_CHANNELS, n_channels))
        if n_sources < 1 or n_sources > MAX_SOURCES:
            raise NotImplementedError(
                "CACGMM runs on the device for 1..{} sources, got n_sources={}".format(
                    MAX_SOURCES, n_sources))

        self._state_set_host("unit_input", None, dv.c128)
        self._state_set_dev("unit_input", _ops.cacgmm_unit_input(self._X, floor))

        self.n_sources, self.n_channels = n_sources, n_channels
        self.n_bins, self.n_frames = n_bins, n_frames
        self.__dict__["_staged"] = None
        self.__dict__["_posterior_from"] = None
        self._applied_permutation = None

        self._init_parameters(rng=self.rng)

    def _init_parameters(self, rng: Optional[np.random.Generator] = None) -> None:
        """Random mixing weights and diagonal covariances: ``alpha`` from ``rng``, then the
        diagonals from ``self.rng``, one mixture after the other (mixture 0 first)."""
        n_sources, n_channels, n_bins = self.n_sources, self.n_channels, self.n_bins

        if rng is None:
            rng = np.random.default_rng()

        eye = np.eye(n_channels, dtype=np.complex128)
        alphas, covariances = [], []
        for _ in range(self._X.shape[0]):
            alpha = rng.random((n_sources, n_bins))
            alpha = alpha / alpha.sum(axis=0)
            B_diag = self.rng.random((n_sources, n_bins, n_channels))
            B_diag = B_diag / B_diag.sum(axis=-1, keepdims=True)
            alphas.append(alpha)
            covariances.append(B_diag[:, :, :, np.newaxis] * eye)

        if self._batched:
            self.mixing, self.covariance = np.stack(alphas), np.stack(covariances)
        else:
            self.mixing, self.covariance = alphas[0], covariances[0]

        # (n_sources, n_bins, n_frames), summing to 1 over the sources, once an E step has run
        self.posterior = None

    def _stage(self):
        """(binv, logp) of the current parameters: the packed inverse covariances and
        log alpha - log det B the frame pass reads; recomputed when either parameter changed."""
        key = (self._state_rev("mixing"), self._state_rev("covariance"))
        staged = self.__dict__.get("_staged")
        if staged is None or staged[0] != key:
            binv, logp = _ops.cacgmm_prepare(self._state_dev("covariance"), self._state_dev("mixing"),
                                             self._info_tensor())
            staged = self.__dict__["_staged"] = (key, binv, logp)
        return staged

    def _posterior_dev(self, staged, floor):
        """gamma (B, N, F, T) of the staged parameters."""
        B, _, F, T = self._X.shape
        gamma = dv.empty((B, self.n_sources, F, T), dv.f64, self._X.device)
        _ops.cacgmm_frame_pass(self._state_dev("unit_input"), staged[1], staged[2], floor,
                               posterior=gamma)
        return gamma

    def _defer_posterior(self, staged, floor) -> None:
        """``posterior`` is now the E step of the ``staged`` parameters; it is formed when read."""
        ent = {"host": None, "dev": None, "none": False, "dtype": dv.f64, "rev": self._next_rev()}

        def fill():
            ent["dev"] = self._posterior_dev(staged, floor)

        ent["lazy"] = fill
        self._state()["posterior"] = ent
        self.__dict__["_posterior_from"] = (ent["rev"], staged[0])

    def separate(self, input: np.ndarray) -> np.ndarray:
        raise NotImplementedError("Implement 'separate' method.")

    def normalize_covariance(self) -> None:
        """B <- B / tr(B)."""
        assert self.normalization, "Set normalization."

        _ops.cacgmm_normalize(self._state_dev("covariance"))
        self._state_touch("covariance")

    def compute_loss(self) -> float:
        raise NotImplementedError("Implement 'compute_loss' method.")

    def compute_logdet(self, covariance: np.ndarray) -> np.ndarray:
        """Log-determinant of ``covariance`` (..., n_channels, n_channels), on the host."""
        _, logdet = np.linalg.slogdet(np.asarray(covariance))

        return logdet

    # -- permutation alignment (once per call) ---------------------------------------------
    def solve_permutation(self, flooring_fn="self") -> None:
        """Align the components over the bins by ``permutation_alignment``."""
        permutation_alignment = self.permutation_alignment
        flooring_fn = choose_flooring_fn(flooring_fn, method=self)

        assert permutation_alignment, "Set permutation_alignment=True."

        if type(permutation_alignment) is bool:
            permutation_alignment = "posterior_score"

        if permutation_alignment in ["posterior_score", "posterior_correlation"]:
            target = "posterior"
        elif permutation_alignment in ["amplitude_score", "amplitude_correlation"]:
            target = "amplitude"
        else:
            raise NotImplementedError(
                "permutation_alignment {} is not implemented.".format(permutation_alignment)
            )

        if permutation_alignment in ["posterior_score", "amplitude_score"]:
            self.solve_permutation_by_score(target=target, flooring_fn=flooring_fn)
        else:
            self.solve_permutation_by_correlation(target=target, flooring_fn=flooring_fn)

    def _host_parameters(self):
        """Writable host copies (B, F, N, ...) of mixing, covariance and posterior, and |Y|."""
        def lead(a):
            a = np.array(a)
            return a if self._batched else a[None]

        alpha = lead(self.mixing).transpose(0, 2, 1).copy()
        cov = lead(self.covariance).transpose(0, 2, 1, 3, 4).copy()
        gamma = lead(self.posterior).transpose(0, 2, 1, 3).copy()
        return alpha, cov, gamma

    def _reference_channel(self):
        X = dv.to_host(self._X[:, self.reference_id])  # (B, F, T)
        return X

    def _store_aligned(self, alpha, cov, gamma, perm) -> None:
        def unlead(a):
            return a if self._batched else a[0]

        self.mixing = unlead(np.ascontiguousarray(alpha.transpose(0, 2, 1)))
        self.covariance = unlead(np.ascontiguousarray(cov.transpose(0, 2, 1, 3, 4)))
        self.posterior = unlead(np.ascontiguousarray(gamma.transpose(0, 2, 1, 3)))
        self.__dict__["_posterior_from"] = None
        # (for the tests) the permutation applied per bin: component perm[i, n] of the E step
        # became component n; None after a call without alignment
        self._applied_permutation = unlead(perm)
        self._state_set_dev("output", _ops.cacgmm_separate(self._state_dev("posterior"), self._X,
                                                           self.reference_id))

    def _align_on_device(self, solver, target, flooring_fn, **iters) -> bool:
        """The alignment on the device where route ``device_alignment`` and
        ``ssspy_permutation_route`` allow (2..8 sources, a built-in floor): the amplitudes
        ``|gamma x_ref|`` are formed there, mixing, covariance and posterior are gathered there, and
        only the permutations -- for the correlation solver also the per-bin overlaps -- cross to
        the host.  False: nothing was done, the host solvers take over."""
        floor = device_flooring(flooring_fn, allow_host=True)
        if not _routes.get("device_alignment") or not _ops.permutation_route(
                self.n_sources, self.n_frames, solver, floor):
            return False
        gamma = self._state_dev("posterior")
        sequence = gamma
        if target == "amplitude":
            sequence = _ops.permutation_amplitude(gamma, self._X, self.reference_id)
        if solver == _lib.PERM_SOLVER_SCORE:
            perm = device_score_permutation(sequence, floor, **iters)
        else:
            perm = device_correlation_permutation(sequence, floor)
        layout = _lib.PERM_LAYOUT_SOURCE_BIN
        mixing = _ops.permute_sources(self._state_dev("mixing"), perm, layout)
        covariance = _ops.permute_sources(self._state_dev("covariance"), perm, layout)
        gamma = _ops.permute_sources(gamma, perm, layout)
        self._state_set_dev("mixing", mixing)
        self._state_set_dev("covariance", covariance)
        self._state_set_dev("posterior", gamma)
        self.__dict__["_posterior_from"] = None
        applied = dv.to_host(perm).astype(np.intp)
        self._applied_permutation = applied if self._batched else applied[0]
        self._state_set_dev("output", _ops.cacgmm_separate(gamma, self._X, self.reference_id))
        return True

    def solve_permutation_by_score(self, target: str = "posterior", flooring_fn="self") -> None:
        """Align by the score of Sawada et al. on the posteriors or on the amplitudes."""
        assert target in ["posterior", "amplitude"], "Invalid target {} is specified.".format(
            target
        )

        flooring_fn = choose_flooring_fn(flooring_fn, method=self)
        global_iter = getattr(self, "global_iter", 1)
        local_iter = getattr(self, "local_iter", 1)

        if self._align_on_device(_lib.PERM_SOLVER_SCORE, target, flooring_fn,
                                 global_iter=global_iter, local_iter=local_iter):
            return

        alpha, cov, gamma = self._host_parameters()
        ref = self._reference_channel() if target == "amplitude" else None
        perms = []
        for b in range(alpha.shape[0]):
            index = np.tile(np.arange(self.n_sources), (self.n_bins, 1))
            if target == "posterior":
                # (the solver returns the permuted sequence; only the further arguments are
                #  permuted in place)
                gamma[b], _ = score_based_permutation_solver(
                    gamma[b], alpha[b], cov[b], index,
                    global_iter=global_iter, local_iter=local_iter, flooring_fn=flooring_fn)
            else:
                amplitude = np.abs(gamma[b] * ref[b][:, np.newaxis, :])
                score_based_permutation_solver(
                    amplitude, alpha[b], cov[b], gamma[b], index,
                    global_iter=global_iter, local_iter=local_iter, flooring_fn=flooring_fn)
            perms.append(index)
        self._store_aligned(alpha, cov, gamma, np.stack(perms))

    def solve_permutation_by_correlation(self, target: str = "amplitude",
                                         flooring_fn="self") -> None:
        """Align by the inter-bin correlation of the amplitudes (Murata et al.)."""
        assert target == "amplitude", "Only amplitude is supported as target."

        flooring_fn = choose_flooring_fn(flooring_fn, method=self)

        if self._align_on_device(_lib.PERM_SOLVER_CORRELATION, target, flooring_fn):
            return

        alpha, cov, gamma = self._host_parameters()
        ref = self._reference_channel()
        perms = []
        for b in range(alpha.shape[0]):
            index = np.tile(np.arange(self.n_sources), (self.n_bins, 1))
            Y = gamma[b] * ref[b][:, np.newaxis, :]
            correlation_based_permutation_solver(Y, alpha[b], cov[b], gamma[b], index,
                                                 flooring_fn=flooring_fn)
            perms.append(index)
        self._store_aligned(alpha, cov, gamma, np.stack(perms))


class CACGMM(CACGMMBase):
    """cACGMM of Ito, Araki and Nakatani (EUSIPCO 2016) with the reference's interface
    (ssspy/bss/cacgmm.py:423-738).

    Args (beyond ``CACGMMBase``):
        normalization: divide every covariance by its trace after the M step.
        permutation_alignment: ``True`` (``"posterior_score"``), ``False``, ``"posterior_score"``,
            ``"amplitude_score"``, ``"posterior_correlation"`` or ``"amplitude_correlation"``.
        reference_id: channel the masks are applied to.
        global_iter, local_iter: iterations of the score solver (score alignments only).
    """

    def __init__(
        self,
        n_sources: Optional[int] = None,
        flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
            max_flooring, eps=EPS
        ),
        callbacks: Optional[Union[Callable, List[Callable]]] = None,
        normalization: bool = True,
        permutation_alignment: Union[bool, str] = True,
        record_loss: bool = True,
        reference_id: int = 0,
        rng: Optional[np.random.Generator] = None,
        **kwargs,
    ) -> None:
        super().__init__(
            n_sources=n_sources,
            flooring_fn=flooring_fn,
            callbacks=callbacks,
            record_loss=record_loss,
            rng=rng,
        )

        self.normalization = normalization
        self.permutation_alignment = permutation_alignment
        self.reference_id = reference_id

        if type(permutation_alignment) is bool and permutation_alignment:
            valid_keys = {"global_iter", "local_iter"}
        elif type(permutation_alignment) is str and permutation_alignment in [
            "posterior_score",
            "amplitude_score",
        ]:
            valid_keys = {"global_iter", "local_iter"}
        else:
            valid_keys = set()

        invalid_keys = set(kwargs) - valid_keys

        assert invalid_keys == set(), "Invalid keywords {} are given.".format(invalid_keys)

        for key, value in kwargs.items():
            setattr(self, key, value)

    def __call__(self, input, n_iter: int = 100, initial_call: bool = True, **kwargs):
        """Separate ``input`` (n_channels, n_bins, n_frames) or a batch
        (n_mixtures, n_channels, n_bins, n_frames); returns (n_sources, n_bins, n_frames) or the
        batch of them."""
        self._bind_input(input)
        self._reset(flooring_fn=self.flooring_fn, **kwargs)

        n_iter = int(n_iter)
        plain = (type(self).update_once is CACGMM.update_once
                 and type(self).compute_loss is CACGMM.compute_loss)
        if plain and self._unobserved_loss(n_iter):
            self._iterate_with_resident_loss(n_iter, initial_call)
        else:
            IterativeMethodBase.__call__(self, n_iter=n_iter, initial_call=initial_call)
            # posterior should be updated
            self.update_posterior(flooring_fn=self.flooring_fn)

        if self.permutation_alignment:
            self.solve_permutation(flooring_fn=self.flooring_fn)
        else:
            self._state_set_dev("output", _ops.cacgmm_separate(self._state_dev("posterior"),
                                                               self._X, self.reference_id))

        return self._final_output()

    def _iterate_with_resident_loss(self, n_iter, initial_call) -> None:
        """The loop when nothing can look at the loss in between: the pass of iteration k leaves the
        loss of the parameters it starts from -- the loss after iteration k - 1 -- as a by-product,
        the final E step that of the last iteration; the per-bin terms stay in HBM and are folded
        and downloaded once.  n_iter + 1 passes in all."""
        B, _, F, _ = self._X.shape
        terms = dv.zeros((n_iter + 1, B, F), dv.f64, self._X.device)
        for k in range(n_iter):
            self._em_step(self._floor(self.flooring_fn), terms[k])
        self.update_posterior(flooring_fn=self.flooring_fn, _loss=terms[n_iter])
        self._check_device_errors()
        values = dv.to_host(_ops.cacgmm_fold_loss(terms))
        self.loss.extend(self._loss_entry(v) for v in (values if initial_call else values[1:]))

    def __repr__(self) -> str:
        s = "CACGMM("
        if self.n_sources is not None:
            s += "n_sources={n_sources}, "
        s += "record_loss={record_loss}"
        s += ", normalization={normalization}"
        s += ", permutation_alignment={permutation_alignment}"
        s += ", reference_id={reference_id}"
        s += ")"
        return s.format(**self.__dict__)

    def separate(self, input: np.ndarray, posterior: Optional[np.ndarray] = None) -> np.ndarray:
        """``posterior * input[reference_id]``; without ``posterior`` the E step of the current
        parameters is used (and not stored)."""
        arr = np.asarray(input)
        X = dv.to_device(arr if arr.ndim == 4 else arr[None], dtype=np.complex128)
        if posterior is None:
            gamma = self._posterior_dev(self._stage(), self._floor(self.flooring_fn))
        else:
            post = np.asarray(posterior)
            gamma = dv.to_device(post if post.ndim == 4 else post[None], dtype=np.float64)
        out = dv.to_host(_ops.cacgmm_separate(gamma, X, self.reference_id))
        return out if arr.ndim == 4 else out[0]

    def _em_step(self, floor, loss=None) -> None:
        """E and M step in one pass over the unit mixture, then the parameter step."""
        staged = self._stage()
        B, M, F, T = self._X.shape
        N, dev = self.n_sources, self._X.device
        sum_gamma = dv.empty((B, N, F), dv.f64, dev)
        num = dv.empty((B, N, F, M, M), dv.c128, dev)
        _ops.cacgmm_frame_pass(self._state_dev("unit_input"), staged[1], staged[2], floor,
                               sum_gamma=sum_gamma, num=num, loss=loss)
        mixing, covariance = _ops.cacgmm_parameter_step(sum_gamma, num, T, floor, self.normalization)
        self._defer_posterior(staged, floor)
        self._state_set_dev("mixing", mixing)
        self._state_set_dev("covariance", covariance)

    def update_once(self, flooring_fn="self") -> None:
        """E step, M step and, with ``normalization``, the trace normalisation."""
        self._em_step(self._floor(flooring_fn))

    def update_posterior(self, flooring_fn="self", _loss=None) -> None:
        """E step: the posteriors of the current parameters."""
        floor = self._floor(flooring_fn)
        staged = self._stage()
        B, _, F, T = self._X.shape
        gamma = dv.empty((B, self.n_sources, F, T), dv.f64, self._X.device)
        _ops.cacgmm_frame_pass(self._state_dev("unit_input"), staged[1], staged[2], floor,
                               loss=_loss, posterior=gamma)
        self._state_set_dev("posterior", gamma)
        self.__dict__["_posterior_from"] = (self._state_rev("posterior"), staged[0])

    def update_parameters(self, flooring_fn="self") -> None:
        """M step from ``posterior`` and the current covariances (no trace normalisation)."""
        floor = self._floor(flooring_fn)
        staged = self._stage()
        B, M, F, T = self._X.shape
        N, dev = self.n_sources, self._X.device
        # the posterior of exactly these parameters is what the pass forms itself; any other
        # (assigned by hand, or parameters changed since the E step) is read from HBM
        own = self.__dict__.get("_posterior_from") == (self._state_rev("posterior"), staged[0])
        given = None if own else self._state_dev("posterior")
        sum_gamma = dv.empty((B, N, F), dv.f64, dev)
        num = dv.empty((B, N, F, M, M), dv.c128, dev)
        _ops.cacgmm_frame_pass(self._state_dev("unit_input"), staged[1], staged[2], floor,
                               sum_gamma=sum_gamma, num=num, posterior_in=given)
        mixing, covariance = _ops.cacgmm_parameter_step(sum_gamma, num, T, floor, False)
        self._state_set_dev("mixing", mixing)
        self._state_set_dev("covariance", covariance)

    def compute_loss(self):
        """-(1/T) sum_ij log sum_n alpha_in / det B_in / (z_ij^H B_in^-1 z_ij)^M."""
        staged = self._stage()
        B, _, F, _ = self._X.shape
        terms = dv.empty((B, F), dv.f64, self._X.device)
        _ops.cacgmm_frame_pass(self._state_dev("unit_input"), staged[1], staged[2],
                               self._floor(self.flooring_fn), loss=terms)
        self._check_device_errors()
        return self._loss_entry(dv.to_host(_ops.cacgmm_fold_loss(terms)))
