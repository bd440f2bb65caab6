"""The GaussMNMF launch plan (csrc/gmnmf_plan.hpp) through its host-only query, restated here in plain
Python on the boundary shapes tests/test_gpu_gmnmf_pass_elementwise.py names: route drift shows
without a GPU.  No compute."""

import itertools

import pytest

LITERAL, PACKED, ROWS8 = range(3)
REGISTERS, LDS_TILE, MEMORY = range(3)
LDS_MAX = 160 * 1024


@pytest.fixture(scope="module")
def ops():
    from ssspy_amd import _build, _lib, _ops

    _build.build()
    _lib.load()
    return _ops


def _al(x):
    return (x + 255) & ~255


def _cdiv(a, b):
    return -(-a // b)


def _chunks(B, N, F, T):
    """Bin chunks of the activation sums: about 1024 blocks, at most 16, at least 8 bins each."""
    blocks0 = _cdiv(T, 64) * N * B
    return max(1, min(_cdiv(1024, blocks0), 16, _cdiv(F, 8)))


def _fold_scratch(total, nslabs):
    """Slabs are folded in groups of 32; more than one group parks its sums and a counter per 256."""
    ng = _cdiv(nslabs, 32)
    return 0 if ng <= 1 else ng * total * 8 + _cdiv(total, 256) * 4


def _bin_lds(N, M, K):
    return N * M * M * 16 + ((N * K + 1) & ~1) * 8


def _acc_lds(N, M, K):
    s = 16 if (N > 8 and M < 4) else 8
    return _bin_lds(N, M, K) + 64 * (2 * M * M + s) * 8


def _expected(B, N, M, F, T, K, part):
    chunks = _chunks(B, N, F, T)
    tb = _cdiv(T, 128)
    nx = 16 if N > 8 else 8
    # workspace of ssspy_gmnmf_update: A, Bt, PQ, activation sums, the expanded pair and the raw basis
    # sums of partitioning, the chunk slabs (one fold group up to 32 slabs: no fold scratch)
    sizes = [B * N * F * T * 8] * 2 + [B * N * F * M * M * 16, B * N * 2 * K * T * 8, B * N * F * K * 8,
                                       B * N * K * T * 8, B * N * F * K * 16]
    off = sum(_al(s) for s in sizes)
    off += _al(chunks * 2 * B * N * K * T * 8) if chunks > 1 else 0
    flags = off
    total = flags + _al(tb * F * B * 4) + _al(B * F * nx * M * M * 8)
    plan = {
        "packed": int(M >= 4), "trace_sources": 0 if M < 4 else (4 if N <= 4 else 8),
        "wide": int(N > 8), "spatial_form": LITERAL if M < 4 else (PACKED if M <= 6 else ROWS8),
        "basis_form": REGISTERS if T <= 512 else (LDS_TILE if T <= 4096 else MEMORY),
        "basis_kc": 4096 // T if T <= 4096 else 0,
        "basis_bpw": max(1, min(16, B * N * F // 8192)),
        "act_chunks": chunks, "act_bins_per_chunk": _cdiv(F, chunks), "act_kslabs": _cdiv(K, 8),
        "bin_lds_bytes": _bin_lds(N, M, K), "latent_lds_bytes": N * K * 8 if part else 0,
        "flags_offset": flags, "point_blocks": tb * F * B, "matrix_blocks": _cdiv(B * N * F, 64),
        # the loss slots [slot][B] and the scratch of their fold, then the flag words
        "loss_flags_offset": _al(tb * F * B * 8) + _al(_fold_scratch(B, tb * F)),
    }
    # (a byte count that does not fit an int reads -1)
    return {k: (v if v < 2 ** 31 else -1) for k, v in plan.items()}, total


NAMED = [
    # forms
    *[(2, N, M, 9, T, 3, 0) for M in range(2, 9) for N in (1, 4, 5, 8, 9, 16) for T in (40, 129)],
    # basis forms, bins per wave
    *[(1, 2, 2, 5, T, 9, p) for T in (512, 513, 4096, 4097) for p in (0, 1)],
    (4, 8, 2, 513, 4, 2, 0),
    # activation chunks
    *[(1, 1, 2, F, 40, 9, 0) for F in (8, 9, 17, 130)],
    # repair
    *[(1, 3, M, 9, 200, 3, 0) for M in (4, 6, 8)], (1, 3, 4, 70, 40, 3, 0), (1, 3, 7, 70, 40, 3, 0),
    # partitioning
    *[(2, N, M, F, T, K, 1) for M in (2, 4, 7) for N in (3, 9) for K in (3, 9)
      for F, T in ((9, 40), (40, 9))],
    (1, 16, 2, 2, 3, 1024, 1),
    # LDS
    (1, 8, 2, 2, 3, 800, 0), (1, 8, 2, 2, 3, 1100, 0), (1, 16, 8, 2, 3, 600, 0),
]


def test_named_shapes_restated(ops):
    from ssspy_amd import _lib

    L = _lib.load()
    for B, N, M, F, T, K, part in NAMED:
        want, total = _expected(B, N, M, F, T, K, part)
        got = ops.gmnmf_route(B, N, M, F, T, K, partitioning=bool(part))
        assert got == want, ((B, N, M, F, T, K, part), {k: (got[k], want[k]) for k in want
                                                         if got[k] != want[k]})
        assert L.ssspy_gmnmf_workspace_bytes(B, N, M, F, T, K) == total
        assert L.ssspy_gmnmf_loss_workspace_bytes(B, F, T) == \
            want["loss_flags_offset"] + _al(want["point_blocks"] * 4)


def test_grid_restated(ops):
    grid = itertools.product([1, 3, 40], [1, 4, 8, 9, 16], [2, 3, 4, 6, 7, 8], [1, 9, 130, 513],
                             [1, 64, 65, 600, 5000], [1, 8, 9, 40])
    for B, N, M, F, T, K in grid:
        want, _ = _expected(B, N, M, F, T, K, 0)
        assert ops.gmnmf_route(B, N, M, F, T, K) == want, (B, N, M, F, T, K)


def test_boundaries_the_gpu_cases_rely_on(ops):
    r = ops.gmnmf_route
    # k_gmnmf_basis: registers, a tile of 7 basis indices (9 = 7 + 2), of 1, memory
    assert [(p["basis_form"], p["basis_kc"]) for p in (r(1, 2, 2, 5, T, 9) for T in
                                                        (512, 513, 4096, 4097))] == \
        [(REGISTERS, 8), (LDS_TILE, 7), (LDS_TILE, 1), (MEMORY, 0)]
    assert r(4, 8, 2, 513, 4, 2)["basis_bpw"] == 2  # 65 workgroups of 8 bins: the last holds one
    # activation chunks: one, two, ragged waves, and 16 chunks of 9 bins of which 15 is empty and 14
    # holds 4
    assert [(p["act_chunks"], p["act_bins_per_chunk"]) for p in (r(1, 1, 2, F, 40, 9) for F in
                                                                  (8, 9, 17, 130))] == \
        [(1, 8), (2, 5), (3, 6), (16, 9)]
    assert 130 - 14 * 9 == 4 and 15 * 9 > 130
    assert r(1, 1, 2, 8, 40, 9)["act_kslabs"] == 2
    assert [r(1, 3, M, 9, 40, 3)["spatial_form"] for M in range(2, 9)] == \
        [LITERAL, LITERAL, PACKED, PACKED, PACKED, ROWS8, ROWS8]
    assert [r(1, N, 4, 9, 40, 3)["trace_sources"] for N in (1, 4, 5, 8, 9, 16)] == [4, 4, 8, 8, 8, 8]
    assert r(1, 3, 4, 9, 200, 3)["point_blocks"] == 18 and r(1, 3, 4, 70, 40, 3)["matrix_blocks"] == 4
    p = r(1, 16, 2, 2, 3, 1024, partitioning=True)
    assert p["latent_lds_bytes"] == 128 * 1024 and p["bin_lds_bytes"] == 129 * 1024


def test_lds_bound(ops):
    """Every source count: n_basis is admitted exactly while the spatial sums' LDS (the bin's spatial
    matrices and basis rows, and a row per frame of the chunk) fits 160 KB."""
    for N, M in ((8, 2), (8, 8), (16, 8), (16, 2), (1, 2), (9, 3)):
        kmax = max(K for K in range(1, 20000) if _acc_lds(N, M, K) <= LDS_MAX)
        assert ops.gmnmf_route(1, N, M, 2, 3, kmax)["bin_lds_bytes"] == _bin_lds(N, M, kmax)
        with pytest.raises(ValueError):
            ops.gmnmf_route(1, N, M, 2, 3, kmax + 1)
    assert ops.gmnmf_route(1, 8, 2, 2, 3, 800)["bin_lds_bytes"] > 48 * 1024
    assert ops.gmnmf_route(1, 8, 2, 2, 3, 1100)["bin_lds_bytes"] > 64 * 1024
    assert _bin_lds(8, 2, 2600) > LDS_MAX
    with pytest.raises(ValueError):
        ops.gmnmf_route(1, 8, 2, 2, 3, 2600)


def test_rejected_arguments(ops):
    for shape in ((0, 2, 2, 9, 40, 4), (1, 0, 2, 9, 40, 4), (1, 2, 1, 9, 40, 4), (1, 17, 2, 9, 40, 4),
                  (1, 2, 9, 9, 40, 4), (1, 2, 2, 0, 40, 4), (1, 2, 2, 9, 0, 4), (1, 2, 2, 9, 40, 0),
                  (1, 2, 2, 9, 40, 65537)):
        with pytest.raises(ValueError):
            ops.gmnmf_route(*shape)
    ops.gmnmf_route(1, 2, 2, 9, 40, 1025)
    with pytest.raises(ValueError):  # the latent step keeps N x n_basis in LDS: up to 1024
        ops.gmnmf_route(1, 2, 2, 9, 40, 1025, partitioning=True)
