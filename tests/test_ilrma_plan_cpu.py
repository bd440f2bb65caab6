"""The ILRMA launch plan (csrc/ilrma_plan.hpp) through its host-only queries, on the boundary shapes
tests/test_gpu_pass_elementwise.py names: route drift shows without a GPU.  No compute."""

import ctypes

import pytest

LAT, THR, GRP, GEN, WIDE, RTN = range(6)
ROUTE_NAMES = ["latency", "throughput", "grouped", "generic", "wide_basis", "runtime_n"]
GAUSS, TMODEL = 0, 1
GROUPED_SHAPES = [(2, 8), (2, 6), (1, 5), (2, 5), (3, 5), (3, 7), (2, 7), (1, 7)]
K_TILE_SHAPES = [(16, 16), (16, 64), (17, 16), (32, 40), (12, 40), (16, 40)]


@pytest.fixture(scope="module")
def lib():
    from ssspy_amd import _build, _lib

    _build.build()
    return _lib.load()


def _route(lib, B, N, F, T, K, domain=2.0, model=GAUSS):
    chunks = ctypes.c_int(0)
    plan = (ctypes.c_int * 3)()
    route = lib.ssspy_ilrma_route(B, N, F, T, K, domain, model, ctypes.byref(chunks), plan)
    return route, chunks.value, tuple(plan)


def _check(lib, shape, route, chunks=None, split=None):
    got, got_chunks, plan = _route(lib, *shape)
    assert got == route, "{} reaches {} instead of {}".format(shape, ROUTE_NAMES[got],
                                                              ROUTE_NAMES[route])
    if chunks == "one":
        assert got_chunks == 1, (shape, got_chunks)
    elif chunks == "many":
        assert got_chunks > 1, (shape, got_chunks)
    # frame splits of the basis pass: (unsplit items, split items, chunks per split item)
    if split == "none":
        assert plan[0] > 0 and plan[1] == 0 and plan[2] == 1, (shape, plan)
    elif split == "all":
        assert plan[0] == 0 and plan[1] > 0 and plan[2] > 1, (shape, plan)
    elif split == "mixed":
        assert plan[0] > 0 and plan[1] > 0 and plan[2] > 1, (shape, plan)
    # the workspaces are sized without knowing the model: they exist for every shape with a route
    assert lib.ssspy_ilrma_workspace_bytes(*shape) > 0
    assert lib.ssspy_ilrma_loss_workspace_bytes(*shape, 1) >= \
        lib.ssspy_ilrma_loss_workspace_bytes(*shape, 0) > 0


@pytest.mark.parametrize("N", [2, 3, 4])
def test_latency_throughput_boundary(lib, N):
    """F = 17 is two bin tiles: 175 mixtures are 350 tiles (latency kernels), 176 leave them.  The
    log-determinant shares come per 16-bin tile from the latency IP1 kernel, finished past it."""
    _check(lib, (175, N, 17, 17, 7), LAT)
    _check(lib, (176, N, 17, 17, 7), THR)
    assert lib.ssspy_ilrma_deferred_logdet_slots(175, N, 17, 17, 7, 2.0, GAUSS) == (17 + 15) // 16
    assert lib.ssspy_ilrma_deferred_logdet_slots(176, N, 17, 17, 7, 2.0, GAUSS) == 1


@pytest.mark.parametrize("B,N", GROUPED_SHAPES)
def test_grouped_sources(lib, B, N):
    _check(lib, (B, N, 17, 17, 7), GRP)


@pytest.mark.parametrize("K", [33, 40])
def test_wide_basis(lib, K):
    _check(lib, (2, 3, 17, 17, K), WIDE)


@pytest.mark.parametrize("N", [9, 16])
def test_runtime_source_count(lib, N):
    _check(lib, (1, N, 17, 17, 7), RTN)


@pytest.mark.parametrize("K,T", K_TILE_SHAPES)
def test_throughput_k_tiles_and_full_tiles(lib, K, T):
    _check(lib, (176, 4, 17, T, K), THR, chunks="many" if K <= 16 else "one",
           split="all" if (T > 16 and K <= 16) else "none")


def test_throughput_one_chunk_and_edge_groups(lib):
    _check(lib, (2048, 2, 17, 16, 16), THR, chunks="one")
    _check(lib, (272, 2, 65, 32, 16), THR, split="mixed")
    _check(lib, (272, 2, 64, 32, 16), THR, split="none")


def test_deferred_loss_by_product(lib):
    """The Student-t data term is not linear in the basis pass's accumulators: no by-product."""
    N, F, T, K = 4, 17, 17, 16
    assert lib.ssspy_ilrma_deferred_loss_supported(N, F, T, K, 2.0, GAUSS)
    assert not lib.ssspy_ilrma_deferred_loss_supported(N, F, T, K, 2.0, TMODEL)
    assert lib.ssspy_ilrma_deferred_loss_slots(2, N, F, T, K, 2.0, GAUSS) > 0
    assert lib.ssspy_ilrma_deferred_loss_slots(2, N, F, T, K, 2.0, TMODEL) == 0
    assert lib.ssspy_ilrma_deferred_logdet_slots(2, N, F, T, K, 2.0, TMODEL) == 0
