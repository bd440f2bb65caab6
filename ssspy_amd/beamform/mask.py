"""Mask-based beamformers on MI355X: MVDR, GEV and the speech-distortion-weighted MWF.

Time-frequency masks (``CACGMM.posterior``, a network's output) weight the spatial covariances and the
covariances steer a filter per bin: Higuchi et al., ICASSP 2016; Heymann et al., ICASSP 2016.  Per
(mixture, bin), with ``x_t`` the ``M`` channels of frame ``t``, ``m_nt >= 0`` the mask of source ``n``
and ``u_nt`` its noise weight (``noise_mask``, or ``1 - m_nt`` formed inside the kernel):

* ``S_n = sum_t m_nt x_t x_t^H``, ``a_n = sum_t m_nt``, ``N_n = sum_t u_nt x_t x_t^H``,
  ``b_n = sum_t u_nt``;
* ``Phi_s = S_n / max(a_n, eps)`` and
  ``Phi_v = N_n / max(b_n, eps) + diagonal_loading (tr(N_n / max(b_n, eps)) / M) I``, ``eps = 1e-10``;
* MVDR (Souden, Benesty, Affes 2010): ``A = Phi_v^-1 Phi_s``, ``w = A e_ref / max(Re tr A, eps)``;
* MWF (speech-distortion-weighted; Doclo et al.): ``w = (Phi_s + mu Phi_v)^-1 Phi_s e_ref``;
* GEV (Warsitz, Haeb-Umbach 2007): ``Phi_v = L L^H``, ``v`` the principal unit eigenvector of
  ``L^-1 Phi_s L^-H``, ``w0 = L^-H v``, ``a = L v``; ``w = w0 conj(a_ref)`` (``"reference"``) or
  ``w = w0 p ||a|| / sqrt(M)`` with ``p = conj(a_ref) / |a_ref|`` (``"ban"``);
* ``y_nt = w_n^H x_t`` and ``demix_filter[f, n, :] = w_n^H``.

The bins never talk to each other, so a workgroup owns one (mixture, bin) and one launch goes from the
spectrogram and the masks to the output (csrc/beamform.hip).  There is no host path: a shape the
kernel does not take raises ``NotImplementedError``.
"""

import numpy as np
import torch

from .. import _device as dv
from .. import _lib, _ops
from ..bss._device_state import DeviceStateMixin, Synced

__all__ = ["MaskBeamformerBase", "MVDR", "GEV", "MWF", "masked_covariance"]

EPS = 1e-10


def _is_device_tensor(value) -> bool:
    return isinstance(value, torch.Tensor)


def _check_containers(input, mask, noise_mask) -> bool:
    """True for device tensors, False for NumPy; a mixture of the two is a ValueError."""
    given = [v for v in (input, mask, noise_mask) if v is not None]
    tensors = [_is_device_tensor(v) for v in given]
    if any(tensors) and not all(tensors):
        raise ValueError(
            "input, mask and noise_mask must all be NumPy arrays or all be tensors on the HIP device.")
    return bool(tensors[0])


def _check_shapes(input_shape, mask_shape, noise_shape) -> None:
    """Ranks, matching axes and the limits of the kernel; nothing is uploaded before this passes."""
    input_shape, mask_shape = tuple(input_shape), tuple(mask_shape)
    if len(input_shape) not in (3, 4):
        raise ValueError(
            "input must be (n_channels, n_bins, n_frames) or (n_mixtures, n_channels, n_bins, "
            "n_frames), got shape {}".format(input_shape))
    if len(mask_shape) != len(input_shape):
        raise ValueError(
            "mask must be (n_sources, n_bins, n_frames), with the leading mixture axis of input if it "
            "has one: input {} and mask {}".format(input_shape, mask_shape))
    if min(input_shape) < 1 or min(mask_shape) < 1:
        raise ValueError("input {} or mask {} has an empty axis".format(input_shape, mask_shape))
    lead = input_shape[:-3]
    if mask_shape[:-3] != lead or mask_shape[-2:] != input_shape[-2:]:
        raise ValueError("input {} and mask {} do not match".format(input_shape, mask_shape))
    if noise_shape is not None:
        noise_shape = tuple(noise_shape)
        allowed = (mask_shape, lead + input_shape[-2:])
        if noise_shape not in allowed:
            raise ValueError("noise_mask must be {} or {}, got {}".format(*allowed, noise_shape))
    M, N = input_shape[-3], mask_shape[-3]
    if M > _lib.BEAMFORM_MAX_CHANNELS:
        raise NotImplementedError(
            "The beamformers take 1..{} channels, got {}.".format(_lib.BEAMFORM_MAX_CHANNELS, M))
    if N > _lib.BEAMFORM_MAX_SOURCES:
        raise NotImplementedError(
            "The beamformers take 1..{} masks, got {}.".format(_lib.BEAMFORM_MAX_SOURCES, N))


def _host_mask(mask, name):
    arr = np.asarray(mask)
    if arr.dtype.kind not in "fiub":
        raise ValueError("{} must be real, got dtype {}".format(name, arr.dtype))
    arr = arr.astype(np.float64, copy=False)
    if not np.all(np.isfinite(arr)) or np.any(arr < 0):
        raise ValueError("{} must be finite and >= 0".format(name))
    return arr


def _device_mask(mask, name, batched, is_tensor):
    """A mask as a contiguous float64 tensor with the leading mixture axis."""
    if mask is None:
        return None
    if is_tensor:
        if not mask.is_cuda or mask.dtype != torch.float64:
            raise ValueError("a tensor {} must be float64 on the HIP device".format(name))
        return (mask if batched else mask[None]).contiguous()
    return dv.to_device(mask if batched else mask[None], dtype=np.float64)


def _device_input(input, batched):
    if _is_device_tensor(input):
        if not input.is_cuda or input.dtype != torch.complex128:
            raise ValueError("a tensor input must be complex128 on the HIP device")
        return (input if batched else input[None]).contiguous()
    arr = np.asarray(input)
    return dv.to_device(arr if batched else arr[None], dtype=np.complex128)


def _raise_if_failed(info, what) -> None:
    failed = int(info[0].item())  # synchronises
    if failed:
        info.zero_()
        raise np.linalg.LinAlgError(
            "{}: the noise covariance of {} (mixture, bin, source) triple(s) has a Cholesky pivot that "
            "is not positive and finite; their filters are zero".format(what, failed))


def masked_covariance(input, mask, normalize: bool = True):
    """``S_n / max(a_n, eps)`` per bin and mask, ``(n_bins, n_sources, n_channels, n_channels)`` (with
    a leading mixture axis for a batch), or ``S_n = sum_t m_nt x_t x_t^H`` itself with
    ``normalize=False``.  ``input`` and ``mask`` as for the beamformers, and the answer comes in the
    same container.  A NumPy mask is checked to be finite and ``>= 0``; a device mask is not."""
    is_tensor = _check_containers(input, mask, None)
    _check_shapes(input.shape, mask.shape, None)
    batched = len(input.shape) == 4
    if not is_tensor:
        mask = _host_mask(mask, "mask")
    X = _device_input(input, batched)
    S = _ops.beamform_covariances(X, _device_mask(mask, "mask", batched, is_tensor),
                                  normalize=normalize)[0]
    S = S if batched else S[0]
    return S if is_tensor else dv.to_host(S)


class MaskBeamformerBase(DeviceStateMixin):
    """What MVDR, GEV and MWF share: the argument checks, the single launch and the attributes.

    ``__call__(input, mask, noise_mask=None)`` takes ``input`` ``(n_channels, n_bins, n_frames)`` or a
    batch ``(n_mixtures, n_channels, n_bins, n_frames)`` and ``mask`` ``(n_sources, n_bins, n_frames)``
    (with the same leading axis for a batch); ``noise_mask`` has the shape of ``mask`` or is
    ``(n_bins, n_frames)``, shared by the sources, and defaults to ``1 - mask``.  All are NumPy arrays
    (any real dtype of a mask is converted to float64) or all are tensors on the HIP device
    (complex128 / float64), and the output ``(n_sources, n_bins, n_frames)`` comes in the same
    container.  NumPy masks are checked to be finite and ``>= 0``; device masks are NOT checked.
    1..8 channels and 1..16 masks, else ``NotImplementedError``.

    After a call: ``input``, ``n_channels``, ``n_sources``, ``n_bins``, ``n_frames``, ``demix_filter``
    ``(n_bins, n_sources, n_channels)``, ``output`` and -- formed by a second launch when first read,
    for which the masks stay referenced -- ``signal_covariance`` and ``noise_covariance``
    ``(n_bins, n_sources, n_channels, n_channels)``: ``Phi_s`` and ``Phi_v`` (loading included) as full
    Hermitian matrices.  A noise covariance with a Cholesky pivot that is not positive and finite
    (too few frames without loading, a mask of ones) raises ``numpy.linalg.LinAlgError`` after the
    launch; the filters of those (bin, source) pairs are zero and ``output`` stays finite.  An
    all-zero mask gives a zero filter and a zero output, and no error.
    """

    demix_filter = Synced(dv.c128)
    output = Synced(dv.c128)
    signal_covariance = Synced(dv.c128)
    noise_covariance = Synced(dv.c128)

    _kind = None
    _mu = 1.0

    def __init__(self, reference_id: int = 0, diagonal_loading: float = 0.0) -> None:
        if isinstance(reference_id, bool) or int(reference_id) != reference_id:
            raise ValueError("reference_id must be an integer, got {!r}.".format(reference_id))
        loading = float(diagonal_loading)
        if not (0.0 <= loading < float("inf")):
            raise ValueError(
                "diagonal_loading must be finite and >= 0, got {!r}.".format(diagonal_loading))
        self.reference_id, self.diagonal_loading = int(reference_id), loading
        self.input = None

    def _reference(self, n_channels: int) -> int:
        ref = self.reference_id
        if not -n_channels <= ref < n_channels:
            raise ValueError(
                "reference_id {} is out of range for {} channels.".format(ref, n_channels))
        return ref % n_channels

    def __call__(self, input, mask, noise_mask=None):
        is_tensor = _check_containers(input, mask, noise_mask)
        _check_shapes(input.shape, mask.shape, None if noise_mask is None else noise_mask.shape)
        ref = self._reference(input.shape[-3])
        if not is_tensor:
            mask = _host_mask(mask, "mask")
            noise_mask = None if noise_mask is None else _host_mask(noise_mask, "noise_mask")
        self._bind_input(input)
        batched = self._batched
        mask_dev = _device_mask(mask, "mask", batched, is_tensor)
        noise_dev = _device_mask(noise_mask, "noise_mask", batched, is_tensor)
        B, M, F, T = self._X.shape
        self.n_channels, self.n_bins, self.n_frames = M, F, T
        self.n_sources = mask_dev.shape[1]
        W, Y, _, _ = _ops.beamform_run(self._X, mask_dev, noise_dev, self._kind, ref,
                                       self.diagonal_loading, self._mu, info=self._info_tensor())
        self._state_set_dev("demix_filter", W)
        self._state_set_dev("output", Y)
        # Phi_s, Phi_v: the same sums again, only if somebody reads them
        shape = (B, F, self.n_sources, M, M)
        for name in ("signal_covariance", "noise_covariance"):
            self._state_set_dev(name, None)
            self._state_defer(name, lambda: self._fill_covariances(mask_dev, noise_dev, ref, shape))
        self._check_device_errors()
        if is_tensor:
            return Y if batched else Y[0]
        return self._final_output()

    def _fill_covariances(self, mask_dev, noise_dev, ref, shape) -> None:
        _, _, Ps, Pv = _ops.beamform_run(self._X, mask_dev, noise_dev, self._kind, ref,
                                         self.diagonal_loading, self._mu, want_output=False,
                                         want_covariances=True)
        assert tuple(Ps.shape) == shape
        state = self._state()
        for name, value in (("signal_covariance", Ps), ("noise_covariance", Pv)):
            state[name]["dev"] = value
            state[name].pop("lazy", None)

    def _check_device_errors(self):
        _ops.check_workspace_canaries()  # no-op unless SSSPY_AMD_WS_CANARY is set
        info = self.__dict__.get("_info")
        if info is not None:
            _raise_if_failed(info, type(self).__name__)

    def apply(self, input):
        """The stored ``demix_filter`` on another spectrogram of the same ``(n_channels, n_bins)``
        (the one before dereverberation, say): ``(n_sources, n_bins, n_frames')`` in the container of
        ``input``.  It runs the apply walk of the beamformer kernel for every shape."""
        if not self._state_has("demix_filter"):
            raise ValueError("apply() needs the filters of a call.")
        shape = tuple(input.shape)
        lead = (self._X.shape[0],) if self._batched else ()
        if len(shape) != len(lead) + 3 or shape[:-1] != lead + (self.n_channels, self.n_bins) \
                or shape[-1] < 1:
            raise ValueError("input must be {}, got {}.".format(
                lead + (self.n_channels, self.n_bins, "n_frames"), shape))
        X = _device_input(input, self._batched)
        Y = _ops.beamform_apply(X, self._state_dev("demix_filter"))
        Y = Y if self._batched else Y[0]
        return Y if _is_device_tensor(input) else dv.to_host(Y)


class MVDR(MaskBeamformerBase):
    """Minimum-variance distortionless-response beamformer in Souden's form,
    ``w = Phi_v^-1 Phi_s e_ref / max(Re tr(Phi_v^-1 Phi_s), eps)``.

    Args:
        reference_id: the channel the output is referred to; negative values count from the end.
        diagonal_loading: ``Phi_v += diagonal_loading (tr Phi_v / n_channels) I``.
    """

    _kind = _lib.BEAMFORM_MVDR

    def __init__(self, reference_id: int = 0, diagonal_loading: float = 1e-6) -> None:
        super().__init__(reference_id=reference_id, diagonal_loading=diagonal_loading)

    def __repr__(self) -> str:
        s = "MVDR(reference_id={reference_id}, diagonal_loading={diagonal_loading})"
        return s.format(**self.__dict__)


class GEV(MaskBeamformerBase):
    """Generalised-eigenvalue (maximum-SNR) beamformer.

    Args:
        reference_id: the channel whose steering-vector entry fixes scale and phase.
        diagonal_loading: ``Phi_v += diagonal_loading (tr Phi_v / n_channels) I``.
        normalization: ``"reference"``: ``w = w0 conj(a_ref)``, distortionless towards the reference
            channel for the steering vector ``a = Phi_v w0`` GEV itself estimates; ``"ban"``: blind
            analytic normalisation with the phase pinned, ``w = w0 p ||a|| / sqrt(n_channels)``,
            ``p = conj(a_ref) / |a_ref|``.
    """

    def __init__(self, reference_id: int = 0, diagonal_loading: float = 1e-6,
                 normalization: str = "reference") -> None:
        super().__init__(reference_id=reference_id, diagonal_loading=diagonal_loading)
        if normalization not in ("reference", "ban"):
            raise ValueError(
                "normalization must be 'reference' or 'ban', got {!r}.".format(normalization))
        self.normalization = normalization

    @property
    def _kind(self):
        if self.normalization not in ("reference", "ban"):
            raise ValueError(
                "normalization must be 'reference' or 'ban', got {!r}.".format(self.normalization))
        return (_lib.BEAMFORM_GEV_BAN if self.normalization == "ban"
                else _lib.BEAMFORM_GEV_REFERENCE)

    def __repr__(self) -> str:
        s = ("GEV(reference_id={reference_id}, diagonal_loading={diagonal_loading}, "
             "normalization={normalization})")
        return s.format(**self.__dict__)


class MWF(MaskBeamformerBase):
    """Speech-distortion-weighted multichannel Wiener filter,
    ``w = (Phi_s + mu Phi_v)^-1 Phi_s e_ref``.

    Args:
        reference_id: the channel the output estimates the source image at.
        diagonal_loading: ``Phi_v += diagonal_loading (tr Phi_v / n_channels) I``.
        mu: trade-off ``> 0`` between noise reduction (large) and speech distortion (small);
            1 is the Wiener filter.
    """

    _kind = _lib.BEAMFORM_MWF

    def __init__(self, reference_id: int = 0, diagonal_loading: float = 0.0,
                 mu: float = 1.0) -> None:
        super().__init__(reference_id=reference_id, diagonal_loading=diagonal_loading)
        if not (0.0 < float(mu) < float("inf")):
            raise ValueError("mu must be finite and > 0, got {!r}.".format(mu))
        self.mu = float(mu)

    @property
    def _mu(self):
        if not (0.0 < self.mu < float("inf")):
            raise ValueError("mu must be finite and > 0, got {!r}.".format(self.mu))
        return self.mu

    def __repr__(self) -> str:
        s = "MWF(reference_id={reference_id}, diagonal_loading={diagonal_loading}, mu={mu})"
        return s.format(**self.__dict__)
