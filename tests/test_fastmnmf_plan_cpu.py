"""The FastGaussMNMF launch plan (csrc/mnmf_plan.hpp) through its host-only queries, on the boundary
shapes tests/test_gpu_mnmf_pass_elementwise.py names: route drift shows without a GPU.  No compute."""

import itertools
import os
import subprocess
import sys

import pytest

from conftest import ROOT

TILED, GENERIC, RUNTIME = range(3)


@pytest.fixture(scope="module")
def ops():
    from ssspy_amd import _build, _lib, _ops

    _build.build()
    _lib.load()
    return _ops


def _al(x):
    return (x + 255) & ~255


def _tiled_workspace_bytes(B, N, M, F, T, K, chunks):
    """The scratch layout of the tiled family, restated: activation partial sums of `chunks` bin
    chunks, the basis copy above 16 bases, U, the row powers, Q^-1, 512 tail records."""
    part = _al(B * chunks * N * 2 * K * T * 8)
    btmp = _al(B * N * F * K * 8) if K > 16 else 0
    tail = _al(512 * max(N * 64 * 16 * 2, 64 * M ** 3 * 2, 64 * N * M * 2) * 8)
    return (part + btmp + _al(B * F * M ** 3 * 16) + _al(B * F * M * 8) + _al(B * F * M * M * 16)
            + tail)


GRID = list(itertools.product([1, 2, 171, 257], [(2, 2), (3, 2), (2, 3), (4, 3), (4, 4)],
                              [17, 65, 129], [32, 33, 34], [3, 8, 9, 16, 17, 40]))


@pytest.mark.parametrize("M,N", [(2, 2), (3, 2), (2, 3), (4, 3), (4, 4), (5, 5), (6, 2), (8, 8),
                                 (3, 1), (2, 6), (9, 9), (16, 3), (4, 12), (16, 16)])
def test_family(ops, M, N):
    route, plan = ops.fastmnmf_route(2, N, M, 9, 40, 4)
    tiled = 2 <= N <= 4 and 2 <= M <= 4
    want = TILED if tiled else (RUNTIME if max(M, N) > 8 else GENERIC)
    assert route == want
    if not tiled:
        assert not any(plan[k] for k in ("fast", "ksmall", "handover", "glds_cov", "kq", "loss_slots"))
        assert plan["logdet_slots"] == 1
        with pytest.raises(ValueError):
            ops.fastmnmf_route(2, N, M, 9, 40, 4, handover=True)


def test_rejected_arguments(ops):
    for shape in ((0, 2, 2, 9, 40, 4), (1, 0, 2, 9, 40, 4), (1, 2, 1, 9, 40, 4), (1, 17, 2, 9, 40, 4),
                  (1, 2, 17, 9, 40, 4), (1, 2, 2, 0, 40, 4), (1, 2, 2, 9, 0, 4), (1, 2, 2, 9, 40, 0)):
        with pytest.raises(ValueError):
            ops.fastmnmf_route(*shape)


def test_query_agrees_with_the_sizers(ops):
    """handover_doubles, deferred_logdet_slots, loss_handover_slots and workspace_bytes are projections
    of the same plan: the query may not drift from them on any shape of the grid."""
    from ssspy_amd import _lib

    L = _lib.load()
    for B, (M, N), F, T, K in GRID:
        route, p = ops.fastmnmf_route(B, N, M, F, T, K)
        assert route == TILED
        hd = L.ssspy_fastmnmf_handover_doubles(B, N, M, F, T, K)
        assert (hd > 0) == bool(p["handover"]) == (K <= 16 and T % 2 == 0)
        assert hd == (B * M * F * T + B * M if p["handover"] else 0)
        assert L.ssspy_fastmnmf_deferred_logdet_slots(B, N, M, F, T, K) == p["logdet_slots"]
        assert L.ssspy_fastmnmf_loss_handover_slots(B, N, M, F, T, K) == p["loss_slots"]
        # the predicates, restated
        assert p["fast"] == p["ksmall"] == int(K <= 16) and p["basis_copy"] == int(K > 16)
        assert p["glds_cov"] == int(K <= 16 and T % 16 == 0)
        assert p["kq"] == (2 if K <= 8 else 4 if K <= 16 else 0)
        for pre, slots, on in (("tail", 256, p["fast"]), ("htail", 512, p["handover"])):
            full, tail, split, groups = (p[pre + s] for s in ("_full", "_tail", "_split", "_groups"))
            if not on:
                assert (full, tail, split, groups) == (0, 0, 1, 0)
                continue
            # make_tail_plan's invariants: every item is there, whole rounds of `slots` run unsplit,
            # the split items fit one round and no chunk is empty
            g, ntiles, items = (F + 63) // 64, (T + 15) // 16, B * ((F + 63) // 64)
            assert groups == g and full + tail == items
            assert (tail == 0 and split == 1) or (1 < split <= min(16, ntiles) and full % slots == 0
                                                  and tail * split <= slots)
        th = (p["htail_groups"], p["htail_split"])
        assert p["loss_slots"] == (th[0] * max(th[1], 1) * 4 if p["handover"] else 0)
        all_split = p["fast"] and p["tail_full"] == 0 and p["tail_tail"] > 0
        assert p["spatial_fold_in_norm"] == int(all_split)
        small = B * F <= 16384  # IP1's latency form (ip1_small_shape, 2..4 channels)
        assert p["ip1_records"] == int(all_split and small)
        assert p["logdet_slots"] == ((F + 15) // 16 if small else 1)
        # the workspace is sized by exactly act_chunks chunks of partial sums (and the basis copy)
        ws = L.ssspy_fastmnmf_workspace_bytes(B, N, M, F, T, K)
        assert ws == _tiled_workspace_bytes(B, N, M, F, T, K, p["act_chunks"])
        assert bool(p["basis_copy"]) == (K > 16)
        hroute, hp = (ops.fastmnmf_route(B, N, M, F, T, K, handover=True) if p["handover"]
                      else (route, None))
        if hp:
            assert hp["glds_spatial"] == hp["glds_cov"] and not p["glds_spatial"]
            assert {k: v for k, v in hp.items() if k != "glds_spatial"} == \
                {k: v for k, v in p.items() if k != "glds_spatial"}


def test_named_shapes(ops):
    """The tail plans the GPU cases rely on."""
    _, p = ops.fastmnmf_route(1, 2, 2, 17, 32, 4)  # one mixture: every item split
    assert p["tail_full"] == 0 and p["tail_tail"] == 1 and p["tail_split"] == 2
    assert p["ip1_records"] and p["spatial_fold_in_norm"] and p["logdet_slots"] == 2
    _, p = ops.fastmnmf_route(257, 2, 2, 17, 32, 4)  # 256 whole items and one split item
    assert (p["tail_full"], p["tail_tail"], p["tail_split"]) == (256, 1, 2)
    assert not p["ip1_records"] and not p["spatial_fold_in_norm"]
    _, p = ops.fastmnmf_route(171, 2, 2, 129, 32, 4, handover=True)  # 513 items of the 512-slot plan
    assert (p["htail_full"], p["htail_tail"], p["htail_split"], p["htail_groups"]) == (512, 1, 2, 3)
    _, p = ops.fastmnmf_route(2, 3, 3, 17, 34, 8, handover=True)  # register-fed with a hand-over
    assert p["handover"] and not p["glds_cov"] and not p["glds_spatial"]
    _, p = ops.fastmnmf_route(2, 3, 3, 17, 33, 8)  # odd T: no hand-over
    assert p["fast"] and not p["handover"]


_CHILD = """
import sys
sys.path.insert(0, {root!r})
from ssspy_amd import _ops
for K in (3, 8, 9, 16):
    route, p = _ops.fastmnmf_route(2, 3, 4, 17, 32, K)
    assert route == 0 and p["ksmall"] == 1, p
    assert not any(p[k] for k in ("fast", "glds_cov", "handover", "loss_slots", "ip1_records",
                                  "spatial_fold_in_norm", "tail_full", "tail_tail")), p
    assert p["kq"] == (2 if K <= 8 else 4)
print("slow forms")
"""


def test_fast_path_disabled_in_a_child(ops):
    """SSSPY_AMD_NO_FAST is read once per process: a fresh child reports the KSMALL forms."""
    env = dict(os.environ, SSSPY_AMD_NO_FAST="1")
    res = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "slow forms" in res.stdout, res.stderr
