"""Permutation alignment between frequency bins: NumPy arrays on the host, torch device tensors on
the device (csrc/permutation.hip; ``device_correlation_permutation`` / ``device_score_permutation``
are what the separators call), with the same permutations.

Counterparts of ``ssspy.algorithm.permutation_alignment``: the correlation-based solver of Murata,
Ikeda and Ziehe (Neurocomputing 41, 2001) and the score-based solver of Sawada, Araki and Makino
(IEEE Trans. ASLP 19(3), 2010), with the reference's signatures, layouts -- ``(n_bins, n_sources,
...)`` -- and results.  Both score every permutation of a bin from that bin's
``n_sources x n_sources`` table of inner products, formed once, instead of reducing over the
frames again for each of the ``n_sources!`` permutations.
"""

import functools
import itertools
from typing import Callable, Optional

import numpy as np

from ..special.flooring import identity, max_flooring

__all__ = ["correlation_based_permutation_solver", "score_based_permutation_solver"]

EPS = 1e-10
_CORRELATION, _SCORE = 0, 1  # _lib.PERM_SOLVER_* (this module loads no library for NumPy input)


def _prepare(sequence, args, overwrite):
    assert sequence.ndim == 3, "Dimension of sequence is expected to be 3."

    for pos_idx, arg in enumerate(args):
        if arg.shape[:2] != sequence.shape[:2]:
            raise ValueError("The shape of {}th argument is invalid.".format(pos_idx + 1))

    if overwrite:
        return sequence, tuple(args)
    return sequence.copy(), tuple(arg.copy() for arg in args)


def _result(sequence, permutable):
    if len(permutable) == 0:
        return sequence
    if len(permutable) == 1:
        return sequence, permutable[0]
    return sequence, permutable


def _all_permutations(n_sources):
    return np.array(list(itertools.permutations(range(n_sources))), dtype=np.intp)


def _best_permutation(gain, permutations):
    """Index of the first permutation p maximising sum_i gain[..., p[i], i]; gain (..., N, N)."""
    n_sources = permutations.shape[1]
    columns = np.arange(n_sources)
    flat = gain.reshape(-1, n_sources, n_sources)
    best = np.empty(flat.shape[0], dtype=np.intp)
    # bins in chunks: the scores of a chunk are (chunk, N!, N) doubles
    chunk = max(1, (1 << 22) // max(1, permutations.size))
    for start in range(0, flat.shape[0], chunk):
        part = flat[start:start + chunk]
        scores = part[:, permutations, columns].sum(axis=-1)
        best[start:start + chunk] = np.argmax(scores, axis=1)
    return best.reshape(gain.shape[:-2])


def _take_sources(array, order):
    """array[f, order[f]] for every bin f; array (n_bins, n_sources, ...), order (n_bins, n_sources)."""
    index = order.reshape(order.shape + (1,) * (array.ndim - 2))
    return np.take_along_axis(array, index, axis=1)


# -- the device solvers (csrc/permutation.hip) ----------------------------------------------------
def _is_device_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def device_correlation_permutation(sequence, floor):
    """perm int32 (B, F, N) of the correlation solver for a device sequence indexed (b, n, f, t),
    real or complex; ``floor`` a resolved ``device_flooring``.  Only the (B, F) overlaps come to
    the host, where ``numpy.argsort`` -- the call of the host solver -- orders the bins."""
    from .. import _device as dv
    from .. import _ops

    envelope, overlap = _ops.permutation_envelope_overlap(sequence, floor)
    order = np.stack([np.argsort(row) for row in dv.to_host(overlap)])
    order = dv.to_device(order, dtype=np.int32, dev=sequence.device)
    return _ops.permutation_correlation_sweep(envelope, order)


def device_score_permutation(sequence, floor, global_iter=1, local_iter=1):
    """perm int32 (B, F, N) of the score solver for a real device sequence indexed (b, n, f, t)."""
    from .. import _ops

    B, N, F, _ = sequence.shape
    normalized = _ops.permutation_score_normalize(sequence)
    perm = _ops.permutation_identity(B, F, N, sequence.device)
    centroid_std = _ops.permutation_score_global(normalized, perm, global_iter, floor)
    return _ops.permutation_score_local(normalized, centroid_std, perm, local_iter, floor)


def _solve_on_device(solver, sequence, args, flooring_fn, overwrite, **iters):
    """The public solvers on torch device tensors (n_bins, n_sources, n_frames) or batched
    (n_mixtures, n_bins, n_sources, n_frames): wholly on the device, or ``NotImplementedError``."""
    from .. import _lib, _ops
    from ..utils.flooring import device_flooring

    assert sequence.ndim in (3, 4), "Dimension of sequence is expected to be 3 (4 with a batch)."
    lead = sequence.ndim - 1
    for pos_idx, arg in enumerate(args):
        if not _is_device_tensor(arg) or tuple(arg.shape[:lead]) != tuple(sequence.shape[:lead]):
            raise ValueError("The shape of {}th argument is invalid.".format(pos_idx + 1))
    if not sequence.is_cuda:
        raise NotImplementedError("permutation alignment of a tensor runs on a HIP device only")

    batched = sequence.ndim == 4
    seq = sequence if batched else sequence[None]
    others = [arg if batched else arg[None] for arg in args]
    B, F, N, T = seq.shape
    floor = device_flooring(flooring_fn, allow_host=True)
    if not _ops.permutation_route(N, T, solver, floor):
        raise NotImplementedError(
            "permutation alignment on the device is limited to {} (convert to NumPy for the host "
            "solver)".format(_ops.permutation_limit(N, T, solver, floor)))

    view = seq.permute(0, 2, 1, 3)  # (b, n, f, t) through strides
    if T > 1 and view.stride(3) != 1:
        view = seq.contiguous().permute(0, 2, 1, 3)
    if solver == _CORRELATION:
        perm = device_correlation_permutation(view, floor)
    else:
        perm = device_score_permutation(view, floor, **iters)

    results = [_ops.permute_sources(a, perm, _lib.PERM_LAYOUT_BIN_SOURCE) for a in [seq] + others]
    if overwrite:
        for given, result in zip([seq] + others, results):
            given.copy_(result)
        results = [seq] + others
    if not batched:
        results = [r[0] for r in results]
    return _result(results[0], tuple(results[1:]))


def correlation_based_permutation_solver(
    sequence: np.ndarray,
    *args,
    flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
        max_flooring, eps=EPS
    ),
    overwrite: bool = True,
):
    """Group the components of every bin by the correlation of their amplitude envelopes.

    The bins are visited from the one whose normalised envelopes overlap least to the one where
    they overlap most; each is permuted to correlate best with the sum of the envelopes aligned so
    far (the first bin keeps its order).

    NumPy arrays are aligned on the host.  Torch device tensors -- (n_bins, n_sources, n_frames)
    or a batch (n_mixtures, n_bins, n_sources, n_frames), ``args`` likewise -- are aligned on the
    device and tensors come back; beyond the device limits (2..8 sources, the built-in floors,
    n_sources * n_frames <= 16384) that raises ``NotImplementedError``.

    Args:
        sequence: (n_bins, n_sources, n_frames), real or complex.
        args: further arrays (n_bins, n_sources, ...) that receive the same permutations.
        flooring_fn: floor of the per-(bin, frame) norm; ``None`` for the identity.
        overwrite: permute ``sequence`` and ``args`` in place.

    Returns:
        The permuted sequence; with one extra argument ``(sequence, arg)``, with more
        ``(sequence, (arg, ...))``.
    """
    if _is_device_tensor(sequence):
        return _solve_on_device(_CORRELATION, sequence, args, flooring_fn, overwrite)

    Y, permutable = _prepare(sequence, args, overwrite)
    if flooring_fn is None:
        flooring_fn = identity

    n_bins, n_sources, _ = Y.shape
    permutations = _all_permutations(n_sources)

    P = np.abs(Y)
    norm = flooring_fn(np.sqrt(np.sum(P**2, axis=1, keepdims=True)))
    P = P / norm
    overlap = np.sum(P @ P.transpose(0, 2, 1), axis=(1, 2))
    order = np.argsort(overlap)

    criterion = P[order[0]].copy()

    for bin_idx in order[1:]:
        # table[a, i] = <envelope a of this bin, criterion i>
        table = P[bin_idx] @ criterion.T
        perm = permutations[_best_permutation(table, permutations)]
        criterion = criterion + P[bin_idx, perm]
        Y[bin_idx] = Y[bin_idx, perm]
        for item in permutable:
            item[bin_idx] = item[bin_idx, perm]

    return _result(Y, permutable)


def _score_gain(table, denom):
    """gain[..., a, i] such that the score of a permutation p -- the sum over i of the correlation of
    component p[i] with centroid i minus its correlations with the other centroids, each divided by
    ``denom[i]`` -- is sum_i gain[..., p[i], i].  table[..., a, j] = mean_t s_a(t) c_j(t)."""
    total = table.sum(axis=-1, keepdims=True)
    return (2 * table - total) / denom.reshape(-1)


def score_based_permutation_solver(
    sequence: np.ndarray,
    *args,
    global_iter: int = 1,
    local_iter: int = 1,
    flooring_fn: Optional[Callable[[np.ndarray], np.ndarray]] = functools.partial(
        max_flooring, eps=EPS
    ),
    multi_centroids: bool = False,
    overwrite: bool = True,
):
    """Align the components of every bin by the score of Sawada et al.

    The sequences are normalised per (bin, component) to zero mean and unit (population) standard
    deviation.  A global stage permutes every bin towards the centroid over all bins,
    ``global_iter`` times; a local stage then visits the bins in order, ``local_iter`` times, and
    permutes each towards its neighbours f-3..f+3 and its (sub)harmonics f/2-1..f/2+1 and
    2f-1..2f+1.  As in the reference, the correlations of both stages are divided by the floored
    standard deviation of the last global centroid, taken at the position the component moves to
    (with ``global_iter=0`` that of the centroid of the unpermuted sequences).

    Args:
        sequence: (n_bins, n_sources, n_frames), real.
        args: further arrays (n_bins, n_sources, ...) that receive the same permutations.
        global_iter, local_iter: iterations of the two stages.
        flooring_fn: floor of the centroid's standard deviation; ``None`` for the identity.
        multi_centroids: not supported.
        overwrite: permute ``args`` in place (and ``sequence`` where the reference does).

    NumPy arrays are aligned on the host.  Torch device tensors -- (n_bins, n_sources, n_frames)
    or a batch (n_mixtures, n_bins, n_sources, n_frames), ``args`` likewise -- are aligned on the
    device and tensors come back (with ``overwrite`` the given tensors, the sequence included);
    beyond the device limits (2..8 sources, the built-in floors) that raises
    ``NotImplementedError``.

    Returns:
        The permuted sequence; with one extra argument ``(sequence, arg)``, with more
        ``(sequence, (arg, ...))``.
    """
    if _is_device_tensor(sequence):
        assert not multi_centroids, "multi_centroids version is not supported."
        return _solve_on_device(_SCORE, sequence, args, flooring_fn, overwrite,
                                global_iter=global_iter, local_iter=local_iter)

    assert sequence.ndim == 3, "Dimension of sequence is expected to be 3."
    assert not multi_centroids, "multi_centroids version is not supported."

    sequence, permutable = _prepare(sequence, args, overwrite)
    if flooring_fn is None:
        flooring_fn = identity

    n_bins, n_sources, n_frames = sequence.shape
    permutations = _all_permutations(n_sources)

    mean = sequence.mean(axis=-1, keepdims=True)
    std = sequence.std(axis=-1, keepdims=True)
    normalized = (sequence - mean) / std

    centroid_std = normalized.mean(axis=0).std(axis=-1, keepdims=True)

    for _ in range(global_iter):
        centroid = normalized.mean(axis=0)
        centroid_std = centroid.std(axis=-1, keepdims=True)
        table = (normalized @ centroid.T) / n_frames
        gain = _score_gain(table, flooring_fn(centroid_std))
        chosen = permutations[_best_permutation(gain, permutations)]
        normalized = _take_sources(normalized, chosen)
        sequence = _take_sources(sequence, chosen)
        for item in permutable:
            item[:] = _take_sources(item, chosen)

    denom = flooring_fn(centroid_std)

    for _ in range(local_iter):
        for bin_idx in range(n_bins):
            near = set(range(max(0, bin_idx - 3), min(n_bins - 1, bin_idx + 3) + 1)) - {bin_idx}
            half = set(range(max(0, bin_idx // 2 - 1), min(n_bins - 1, bin_idx // 2 + 1) + 1))
            double = set(range(max(0, 2 * bin_idx - 1), min(n_bins - 1, 2 * bin_idx + 1) + 1))
            neighbours = sorted(near | half | double)

            # the score adds over the neighbours, so their sum stands in for each of them
            anchor = normalized[neighbours].sum(axis=0)
            table = (normalized[bin_idx] @ anchor.T) / n_frames
            gain = _score_gain(table, denom)
            perm = permutations[_best_permutation(gain, permutations)]
            normalized[bin_idx] = normalized[bin_idx, perm]
            sequence[bin_idx] = sequence[bin_idx, perm]
            for item in permutable:
                item[bin_idx] = item[bin_idx, perm]

    return _result(sequence, permutable)
