"""Permutation alignment on the device (csrc/permutation.hip) against the host solvers of
ssspy_amd/algorithm/permutation_alignment.py: the same permutation in every bin, the same tie rule,
gathered arrays bit for bit.

The sums of the device run in another order than NumPy's, so a parity test is only meaningful where
no decision of the host solver is a near-tie.  Every parity test therefore computes that
precondition on the host and asserts it as such: at every decision the best score exceeds the
second-best distinct score by at least 1e-9 of sum |gain| (the rounding of a table entry is about
T eps <= 1e-13 of it), and neighbouring sorted overlaps of the correlation solver differ by at
least 1e-9 relative.  A seed that breaks it fails loudly instead of hiding a flipped decision.
"""

import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 1e-10
MARGIN = 1e-9
# (n_sources, n_bins, n_frames): 300 and 257 frames are no multiple of a workgroup
SHAPES = [(2, 2, 2), (2, 9, 7), (3, 17, 64), (4, 33, 300), (8, 9, 40), (5, 12, 257)]
# the score solver: T = 2 is an exact tie after normalisation; 2 and 3 bins clip every neighbour set
SCORE_SHAPES = [s for s in SHAPES if s[2] >= 7] + [(3, 2, 64), (3, 3, 64)]


# ---------------------------------------------------------------- the host solvers as they were
# Verbatim copies of the NumPy solvers before the device route existed (test_numpy_calls_unchanged
# compares the public functions with them); _best_permutation additionally reports every decision
# to `_decisions` for the precondition.
def identity(x):
    return x


def max_flooring(x, eps=EPS):
    return np.maximum(x, eps)


def add_flooring(x, eps=EPS):
    return x + eps


_decisions = []


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
    n_sources = permutations.shape[1]
    columns = np.arange(n_sources)
    flat = gain.reshape(-1, n_sources, n_sources)
    best = np.empty(flat.shape[0], dtype=np.intp)
    chunk = max(1, (1 << 22) // max(1, permutations.size))
    for start in range(0, flat.shape[0], chunk):
        part = flat[start:start + chunk]
        scores = part[:, permutations, columns].sum(axis=-1)
        best[start:start + chunk] = np.argmax(scores, axis=1)
        for table, row in zip(part, scores):
            distinct = np.unique(row)
            gap = distinct[-1] - distinct[-2] if distinct.size > 1 else 0.0
            _decisions.append(gap / max(np.abs(table).sum(), np.finfo(float).tiny))
    return best.reshape(gain.shape[:-2])


def _take_sources(array, order):
    index = order.reshape(order.shape + (1,) * (array.ndim - 2))
    return np.take_along_axis(array, index, axis=1)


def host_correlation(sequence, *args, flooring_fn=functools.partial(max_flooring, eps=EPS),
                     overwrite=True):
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
        table = P[bin_idx] @ criterion.T
        perm = permutations[_best_permutation(table, permutations)]
        criterion = criterion + P[bin_idx, perm]
        Y[bin_idx] = Y[bin_idx, perm]
        for item in permutable:
            item[bin_idx] = item[bin_idx, perm]

    return _result(Y, permutable)


def _score_gain(table, denom):
    total = table.sum(axis=-1, keepdims=True)
    return (2 * table - total) / denom.reshape(-1)


def host_score(sequence, *args, global_iter=1, local_iter=1,
               flooring_fn=functools.partial(max_flooring, eps=EPS), multi_centroids=False,
               overwrite=True):
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

            anchor = normalized[neighbours].sum(axis=0)
            table = (normalized[bin_idx] @ anchor.T) / n_frames
            gain = _score_gain(table, denom)
            perm = permutations[_best_permutation(gain, permutations)]
            normalized[bin_idx] = normalized[bin_idx, perm]
            sequence[bin_idx] = sequence[bin_idx, perm]
            for item in permutable:
                item[bin_idx] = item[bin_idx, perm]

    return _result(sequence, permutable)


FLOORS = {
    "none": None,
    "max": functools.partial(max_flooring, eps=EPS),
    "add": functools.partial(add_flooring, eps=EPS),
}


def package_floor(name):
    from ssspy_amd.special import flooring

    if name == "none":
        return None
    return functools.partial(getattr(flooring, name + "_flooring"), eps=EPS)


# ---------------------------------------------------------------- inputs
def make_sources(seed, B, N, F, T):
    """(B, F, N, T) complex: sources with distinct frame envelopes (each is active in its own
    stretch of the frames, over a smooth random floor), shuffled at random in every bin."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    out = np.empty((B, F, N, T), dtype=np.complex128)
    for b in range(B):
        centre = (rng.permutation(N) + 0.5) * T / N
        width = max(T / N, 1.0)
        env = 0.2 + rng.random((N, T)) * 0.3 + 2.0 * np.exp(
            -0.5 * ((t[None, :] - centre[:, None]) / (0.4 * width)) ** 2)
        for f in range(F):
            gain = 0.5 + rng.random((N, 1))
            noise = rng.standard_normal((N, T)) + 1j * rng.standard_normal((N, T))
            jitter = 1.0 + 0.2 * rng.random((N, T))
            out[b, f] = (gain * env * jitter * noise / np.abs(noise))[rng.permutation(N)]
    return out


def index_like(B, F, N):
    return np.tile(np.arange(N), (B, F, 1))


def dev(a, dtype=None):
    from ssspy_amd import _device as dv

    return dv.to_device(a, dtype=dtype)


def host(t):
    return t.cpu().numpy()


_cache = {}


def correlation_reference(N, F, T, B, floor):
    """Host solver per mixture, once per case: (Y, aligned Y, permutations, margins, overlap gap)."""
    key = ("corr", N, F, T, B, floor)
    if key not in _cache:
        Y = make_sources(100 + N * F + T, B, N, F, T)
        aligned, index = Y.copy(), index_like(B, F, N)
        del _decisions[:]
        gaps = [np.inf]
        for b in range(B):
            host_correlation(aligned[b], index[b], flooring_fn=FLOORS[floor])
            P = np.abs(Y[b])
            norm = np.sqrt(np.sum(P ** 2, axis=1, keepdims=True))
            P = P / (norm if FLOORS[floor] is None else FLOORS[floor](norm))
            overlap = np.sort(np.sum(P @ P.transpose(0, 2, 1), axis=(1, 2)))
            if F > 1:
                gaps.append(np.min(np.diff(overlap) / overlap[1:]))
        margin = min(_decisions) if _decisions else np.inf
        for a in (Y, aligned, index):
            a.flags.writeable = False
        _cache[key] = (Y, aligned, index, margin, min(gaps))
    return _cache[key]


def score_reference(N, F, T, B, floor, iters):
    key = ("score", N, F, T, B, floor, iters)
    if key not in _cache:
        S = np.abs(make_sources(200 + N * F + T, B, N, F, T)) ** 2
        index = index_like(B, F, N)
        aligned = np.empty_like(S)
        del _decisions[:]
        for b in range(B):
            aligned[b], _ = host_score(S[b].copy(), index[b], global_iter=iters[0],
                                       local_iter=iters[1], flooring_fn=FLOORS[floor])
        margin = min(_decisions) if _decisions else np.inf
        for a in (S, aligned, index):
            a.flags.writeable = False
        _cache[key] = (S, aligned, index, margin)
    return _cache[key]


# ---------------------------------------------------------------- 1. best permutation alone
@pytest.mark.parametrize("N", [2, 3, 4, 5, 8])
def test_best_permutation(N):
    from ssspy_amd import _ops

    rng = np.random.default_rng(N)
    tables = rng.standard_normal((24, N, N))
    tables[8:12, 1] = tables[8:12, 0]           # two identical rows: an exact tie by construction
    tables[12:14, N - 1] = tables[12:14, 0]
    tables[14] = 0.75                           # all equal: index 0
    tables[15] = 0.0
    expect = _best_permutation(tables, _all_permutations(N))
    got = host(_ops.best_permutation(dev(tables)))
    assert np.array_equal(got, expect)
    assert got[14] == 0 and got[15] == 0
    # the tie really is one: the winner's mirror image scores the same and comes later
    perms = _all_permutations(N)
    for m in range(8, 12):
        mirror = perms[got[m]].copy()
        i0, i1 = np.where(mirror == 0)[0][0], np.where(mirror == 1)[0][0]
        mirror[i0], mirror[i1] = 1, 0
        later = np.where((perms == mirror).all(axis=1))[0][0]
        assert later > got[m]


# ---------------------------------------------------------------- 2. envelope and overlap
@pytest.mark.parametrize("floor", ["none", "max", "add"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_envelope_and_overlap(shape, floor):
    from ssspy_amd import _ops
    from ssspy_amd.utils.flooring import device_flooring

    N, F, T = shape
    Y = make_sources(7, 2, N, F, T)
    if floor == "max":
        Y[0, F // 2, :, T // 2] = 0.0  # an all-zero frame: 0 / eps
    P = np.abs(Y)
    norm = np.sqrt(np.sum(P ** 2, axis=2, keepdims=True))
    P = P / (norm if FLOORS[floor] is None else FLOORS[floor](norm))
    overlap = np.sum(P @ P.transpose(0, 1, 3, 2), axis=(2, 3))
    native = dev(np.ascontiguousarray(Y.transpose(0, 2, 1, 3)))  # (B, N, F, T)
    strided = dev(Y).permute(0, 2, 1, 3)                         # the same through strides
    for sequence in (native, strided):
        envelope, got = _ops.permutation_envelope_overlap(
            sequence, device_flooring(package_floor(floor)))
        envelope, got = host(envelope), host(got)
        print(shape, floor, np.abs(envelope / np.where(P > 0, P, 1) - (P > 0)).max(),
              np.abs(got / overlap - 1).max())
        np.testing.assert_allclose(envelope, P, rtol=1e-12, atol=0)
        np.testing.assert_allclose(got, overlap, rtol=1e-12, atol=0)
    if floor == "max":
        assert (envelope[0, F // 2, :, T // 2] == 0).all()


# ---------------------------------------------------------------- 3. correlation solver
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_correlation_solver(shape, B):
    from ssspy_amd import _lib, _ops
    from ssspy_amd.algorithm.permutation_alignment import (
        correlation_based_permutation_solver,
        device_correlation_permutation,
    )
    from ssspy_amd.utils.flooring import device_flooring

    N, F, T = shape
    for floor in ("max", "none"):
        Y, aligned, index, margin, gap = correlation_reference(N, F, T, B, floor)
        print(shape, B, floor, "margin", margin, "overlap gap", gap)
        assert margin >= MARGIN and gap >= MARGIN, "precondition: a near-tie on the host"
        rng = np.random.default_rng(5)
        filt = rng.standard_normal((B, F, N, N)) + 1j * rng.standard_normal((B, F, N, N))
        spec = rng.standard_normal((B, F, N, T + 3))
        take = index[..., None]
        # the library's layout through the operators
        native = dev(np.ascontiguousarray(Y.transpose(0, 2, 1, 3)))
        perm = device_correlation_permutation(native, device_flooring(package_floor(floor)))
        assert np.array_equal(host(perm), index)
        moved = _ops.permute_sources(native, perm, _lib.PERM_LAYOUT_SOURCE_BIN)
        assert np.array_equal(host(moved), aligned.transpose(0, 2, 1, 3))
        # the public function on (B, F, N, T), and on (F, N, T)
        lead = (slice(None),) if B > 1 else (0,)
        for overwrite in (False, True):
            given = [dev(a[lead]) for a in (Y, filt, spec, index_like(B, F, N))]
            out, (out_filt, out_spec, out_index) = correlation_based_permutation_solver(
                *given, flooring_fn=package_floor(floor), overwrite=overwrite)
            assert np.array_equal(host(out_index), index[lead])
            assert np.array_equal(host(out), aligned[lead])
            assert np.array_equal(host(out_filt), np.take_along_axis(filt, take, axis=2)[lead])
            assert np.array_equal(host(out_spec), np.take_along_axis(spec, take, axis=2)[lead])
            assert np.array_equal(host(given[0]), (aligned if overwrite else Y)[lead])


def test_correlation_solver_single_bin():
    from ssspy_amd.algorithm.permutation_alignment import correlation_based_permutation_solver

    Y = make_sources(3, 1, 3, 1, 40)[0]
    out, index = correlation_based_permutation_solver(dev(Y), dev(index_like(1, 1, 3)[0]))
    assert np.array_equal(host(out), Y) and np.array_equal(host(index), [[0, 1, 2]])


# ---------------------------------------------------------------- 4. score solver
@pytest.mark.parametrize("iters", [(1, 1), (2, 2), (0, 1), (1, 0)], ids=str)
@pytest.mark.parametrize("shape", SCORE_SHAPES, ids=str)
def test_score_solver(shape, iters):
    from ssspy_amd.algorithm.permutation_alignment import (
        device_score_permutation,
        score_based_permutation_solver,
    )
    from ssspy_amd.utils.flooring import device_flooring

    N, F, T = shape
    for B, floor in ((3, "max"), (1, "none")):
        S, aligned, index, margin = score_reference(N, F, T, B, floor, iters)
        print(shape, iters, B, floor, "margin", margin)
        assert margin >= MARGIN, "precondition: a near-tie on the host"
        native = dev(np.ascontiguousarray(S.transpose(0, 2, 1, 3)))
        perm = device_score_permutation(native, device_flooring(package_floor(floor)), *iters)
        assert np.array_equal(host(perm), index)
        rng = np.random.default_rng(6)
        cov = rng.standard_normal((B, F, N, 2, 2)) + 1j * rng.standard_normal((B, F, N, 2, 2))
        weight = rng.random((B, F, N))
        lead = (slice(None),) if B > 1 else (0,)
        given = [dev(a[lead]) for a in (S, cov, weight, index_like(B, F, N))]
        out, (out_cov, out_weight, out_index) = score_based_permutation_solver(
            *given, global_iter=iters[0], local_iter=iters[1], flooring_fn=package_floor(floor))
        assert np.array_equal(host(out_index), index[lead])
        assert np.array_equal(host(out), aligned[lead])
        assert np.array_equal(host(out_cov),
                              np.take_along_axis(cov, index[..., None, None], axis=2)[lead])
        assert np.array_equal(host(out_weight), np.take_along_axis(weight, index, axis=2)[lead])


# ---------------------------------------------------------------- 5. an exact tie through a solver
def test_exact_tie_through_the_solvers():
    from ssspy_amd.algorithm.permutation_alignment import (
        correlation_based_permutation_solver,
        score_based_permutation_solver,
    )

    N, F, T = 3, 9, 64
    Y = make_sources(11, 1, N, F, T)[0]
    Y[4, 2] = Y[4, 0]  # two identical components in bin 4: every table of that bin has equal rows
    index = index_like(1, F, N)[0]
    host_correlation(Y.copy(), index)
    _, got = correlation_based_permutation_solver(dev(Y), dev(index_like(1, F, N)[0]))
    assert np.array_equal(host(got), index)
    S = np.abs(Y) ** 2
    index = index_like(1, F, N)[0]
    host_score(S.copy(), index, global_iter=2, local_iter=2)
    _, got = score_based_permutation_solver(dev(S), dev(index_like(1, F, N)[0]), global_iter=2,
                                            local_iter=2)
    assert np.array_equal(host(got), index)


# ---------------------------------------------------------------- 6. determinism
def test_two_runs_give_the_same_bits():
    from ssspy_amd.algorithm.permutation_alignment import (
        device_correlation_permutation,
        device_score_permutation,
    )
    from ssspy_amd.utils.flooring import device_flooring

    floor = device_flooring(package_floor("max"))
    Y = dev(np.ascontiguousarray(make_sources(13, 3, 4, 33, 300).transpose(0, 2, 1, 3)))
    S = (Y.real ** 2 + Y.imag ** 2).contiguous()
    runs = [(host(device_correlation_permutation(Y, floor)),
             host(device_score_permutation(S, floor, 2, 2))) for _ in range(2)]
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert not np.array_equal(runs[0][0], index_like(3, 33, 4))  # (something was aligned)


# ---------------------------------------------------------------- 7. the classes
def fdica_mixture(B, N, F, T):
    from ssspy_amd.utils.dataset import nmf_mixture

    X = np.stack([nmf_mixture(40 + b, N, F, T) for b in range(B)])
    return X if B > 1 else X[0]


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", ["NaturalGradLaplaceFDICA", "AuxLaplaceFDICA"])
def test_fdica_routes_agree(name, B):
    from ssspy_amd import _routes, bss

    X = fdica_mixture(B, 3, 17, 64)
    runs = []
    for device in (True, False):
        with _routes.override(device_alignment=device):
            kwargs = dict(spatial_algorithm="IP1") if name == "AuxLaplaceFDICA" else {}
            m = getattr(bss, name)(**kwargs)
            Y = m(X, n_iter=10)
            runs.append((Y, np.array(m.demix_filter)))
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][0], runs[1][0])
    # (the alignment did something: without it the filters differ)
    m = getattr(bss, name)(permutation_alignment=False, **kwargs)
    m(X, n_iter=10)
    assert not np.array_equal(np.array(m.demix_filter), runs[0][1])


CACGMM_MODES = [True, "posterior_score", "amplitude_score", "amplitude_correlation"]


def run_cacgmm(X, how, device, n_sources=None, **kwargs):
    from ssspy_amd import _routes
    from ssspy_amd.bss import CACGMM

    with _routes.override(device_alignment=device):
        m = CACGMM(n_sources=n_sources, permutation_alignment=how, rng=np.random.default_rng(0),
                   **kwargs)
        Y = m(X, n_iter=10)
    return dict(output=Y, permutation=np.array(m._applied_permutation), mixing=np.array(m.mixing),
                covariance=np.array(m.covariance), posterior=np.array(m.posterior))


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("how", CACGMM_MODES, ids=str)
def test_cacgmm_routes_agree(how, B):
    import cacgmm_numpy as cn

    X = np.stack([cn.make_mixture(3, 3, 17, 64, seed=70 + b) for b in range(B)])
    X = X if B > 1 else X[0]
    kwargs = dict(global_iter=2, local_iter=2) if how == "posterior_score" else {}
    on, off = run_cacgmm(X, how, True, **kwargs), run_cacgmm(X, how, False, **kwargs)
    for key in on:
        assert np.array_equal(on[key], off[key]), key
    assert on["permutation"].shape == ((B,) if B > 1 else ()) + (17, 3)


# ---------------------------------------------------------------- 8. limits
def test_nine_sources_take_the_host_route():
    import cacgmm_numpy as cn
    from ssspy_amd import _lib, _ops
    from ssspy_amd.utils.flooring import device_flooring

    floor = device_flooring(package_floor("max"))
    assert not _ops.permutation_route(9, 64, _lib.PERM_SOLVER_SCORE, floor)
    assert not _ops.permutation_route(1, 64, _lib.PERM_SOLVER_SCORE, floor)
    assert _ops.permutation_route(8, 2048, _lib.PERM_SOLVER_CORRELATION, floor)
    assert not _ops.permutation_route(8, 2049, _lib.PERM_SOLVER_CORRELATION, floor)
    assert _ops.permutation_route(8, 2049, _lib.PERM_SOLVER_SCORE, floor)
    X = cn.make_mixture(4, 9, 9, 48)
    # (the factorial search of the host solver: a correlation alignment keeps this to seconds)
    on = run_cacgmm(X, "amplitude_correlation", True, n_sources=9)
    off = run_cacgmm(X, "amplitude_correlation", False, n_sources=9)
    for key in on:
        assert np.array_equal(on[key], off[key]), key


def test_callable_floor_takes_the_host_route():
    from ssspy_amd import _routes, bss

    def floor(x):
        return np.maximum(x, 1e-9)

    X = fdica_mixture(1, 3, 17, 64)
    runs = []
    for device in (True, False):
        with _routes.override(device_alignment=device):
            m = bss.NaturalGradLaplaceFDICA(flooring_fn=floor)
            Y = m(X, n_iter=5)
            runs.append((Y, np.array(m.demix_filter)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_public_functions_refuse_beyond_the_limits():
    from ssspy_amd.algorithm.permutation_alignment import (
        correlation_based_permutation_solver,
        score_based_permutation_solver,
    )

    nine = dev(np.abs(make_sources(1, 1, 9, 3, 16)[0]))
    small = dev(np.abs(make_sources(1, 1, 3, 3, 16)[0]))
    for solver in (correlation_based_permutation_solver, score_based_permutation_solver):
        with pytest.raises(NotImplementedError, match="2..8 sources"):
            solver(nine)
        with pytest.raises(NotImplementedError, match="flooring_fn"):
            solver(small, flooring_fn=lambda x: x + 1e-3)
    with pytest.raises(NotImplementedError, match="16384"):
        correlation_based_permutation_solver(dev(np.ones((2, 8, 2049))))
    with pytest.raises(AssertionError):
        score_based_permutation_solver(small, multi_centroids=True)
    with pytest.raises(ValueError, match="1th argument"):
        score_based_permutation_solver(small, dev(np.ones((3, 2, 5))))


def test_numpy_calls_unchanged():
    from ssspy_amd.algorithm.permutation_alignment import (
        correlation_based_permutation_solver,
        score_based_permutation_solver,
    )

    N, F, T = 4, 33, 300
    Y = make_sources(17, 1, N, F, T)[0]
    extra = np.random.default_rng(1).standard_normal((F, N, N))
    for floor in ("max", "none", "add"):
        a = correlation_based_permutation_solver(Y.copy(), extra.copy(),
                                                 flooring_fn=package_floor(floor))
        b = host_correlation(Y.copy(), extra.copy(), flooring_fn=FLOORS[floor])
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        S = np.abs(Y) ** 2
        a = score_based_permutation_solver(S.copy(), extra.copy(), global_iter=2, local_iter=2,
                                           flooring_fn=package_floor(floor), overwrite=False)
        b = host_score(S.copy(), extra.copy(), global_iter=2, local_iter=2,
                       flooring_fn=FLOORS[floor], overwrite=False)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
