"""GPU parity at the sizes BASELINE.json names (configs[1]..[4]), through the C ABI, against the
CPU oracle (which is pinned to the reference by tests/test_oracle_golden.py and was checked
against the reference itself at the full configs[1] size).

Tolerances: north_star asks for 1e-4 relative fp64 on filters and spectrograms.  Iterative
projection amplifies rounding by up to ~1e5 over 100 iterations, so the
100-iteration run is held to 1e-6; short runs to 1e-8; loss lists to 1e-9.
The inputs are regenerated from their seeds on the box; their SHA-256 is checked against
tests/golden/input_sha256.json first, so "the same synthetic mixture" is literal.
"""

import json
import os

import numpy as np
import pytest

from conftest import rel_err

from ssspy_amd import _routes

pytestmark = pytest.mark.gpu

TOL = 1e-8
LOSS_RTOL = 1e-9
HERE = os.path.dirname(os.path.abspath(__file__))


def _pinned_mixture(name):
    from ssspy_amd.utils.dataset import nmf_mixture, sha256_of

    pin = json.load(open(os.path.join(HERE, "golden", "input_sha256.json")))[name]
    X = nmf_mixture(pin["seed"], *pin["shape"])
    assert sha256_of(X) == pin["sha256"], "regenerated input differs from the committed bytes"
    return X


def test_configs1_full_size_100_iterations_against_oracle():
    """BASELINE configs[1] literally: GaussILRMA-IP1, N=4, F=1025, T=512, n_basis=16, 100
    iterations, against the oracle's 100 iterations on the host (the reference's update order,
    ssspy/bss/ilrma.py:900-922)."""
    from oracle.ilrma import GaussILRMAOracle
    from ssspy_amd.bss.ilrma import GaussILRMA

    N, F, T, K = 4, 1025, 512, 16
    X = _pinned_mixture("configs1_seed1000_N4_F1025_T512")
    basis = np.random.default_rng(1001).random((N, F, K))
    act = np.random.default_rng(1002).random((N, K, T))
    m = GaussILRMA(n_basis=K)
    Y = m(X, n_iter=100, basis=basis, activation=act)
    ref = GaussILRMAOracle(n_basis=K)
    Yr = ref.run(X, n_iter=100, basis=basis, activation=act)
    np.testing.assert_allclose(m.loss, ref.loss, rtol=LOSS_RTOL)
    assert rel_err(m.demix_filter, ref.demix_filter) < 1e-6
    assert rel_err(Y, Yr) < 1e-6
    assert rel_err(m.basis, ref.basis) < 1e-6 and rel_err(m.activation, ref.activation) < 1e-6


def test_configs4_shard_of_128_mixtures():
    """BASELINE configs[4], one GPU's shard: 128 independent full-size mixtures (seeds 1000..1127)
    resident in HBM, 20 iterations of the batched update_once() bench.py times (round 5: two before).
    Mixtures 0, 63 and 127 must equal their single-mixture runs (same kernels, other schedule: the
    batched launch runs whole rounds of work items plus a split tail, the single launch only split
    items), and each of the three must match 20 iterations of the oracle."""
    import torch

    from oracle.ilrma import GaussILRMAOracle
    from ssspy_amd.bss.ilrma import GaussILRMA
    from ssspy_amd.utils.dataset import nmf_mixture_batch, sha256_of

    B, N, F, T, K = 128, 4, 1025, 512, 16
    pins = json.load(open(os.path.join(HERE, "golden", "input_sha256.json")))
    Xh = nmf_mixture_batch(1000, B, N, F, T)
    for b in (0, 63, 127):
        assert sha256_of(Xh[b]) == pins["configs1_seed{}_N4_F1025_T512".format(1000 + b)]["sha256"]
    rng = np.random.default_rng(2000)
    basis, act = rng.random((B, N, F, K)), rng.random((B, N, K, T))
    X = torch.from_numpy(Xh).to("cuda")
    mb = GaussILRMA(n_basis=K, scale_restoration=False)
    n_iter = 20
    mb(X, n_iter=n_iter, basis=basis, activation=act)
    Wb, Tb, Vb = mb.demix_filter, mb.basis, mb.activation
    lossb = np.asarray(mb.loss)
    assert Wb.shape == (B, F, N, N) and lossb.shape == (n_iter + 1, B)
    for b in (0, 63, 127):
        m1 = GaussILRMA(n_basis=K, scale_restoration=False)
        m1(Xh[b], n_iter=n_iter, basis=basis[b], activation=act[b])
        # (20 iterations of IP amplify the reduction-order difference of the two schedules)
        assert rel_err(Wb[b], m1.demix_filter) < 1e-9
        assert rel_err(Tb[b], m1.basis) < 1e-9 and rel_err(Vb[b], m1.activation) < 1e-9
        np.testing.assert_allclose(lossb[:, b], m1.loss, rtol=1e-10)
        ref = GaussILRMAOracle(n_basis=K, scale_restoration=False)
        ref.run(Xh[b], n_iter=n_iter, basis=basis[b], activation=act[b])
        assert rel_err(Wb[b], ref.demix_filter) < 1e-7
        assert rel_err(Tb[b], ref.basis) < 1e-7 and rel_err(Vb[b], ref.activation) < 1e-7
        np.testing.assert_allclose(lossb[:, b], ref.loss, rtol=LOSS_RTOL)


def test_configs2_full_size_against_oracle():
    """BASELINE configs[2]: AuxLaplaceIVA-ISS, N=8, F=2049, T=1024; two iterations against the
    oracle (ssspy/bss/iva.py:1917-1966, _update_spatial_model.py:146-194), before and after
    projection back."""
    from oracle.iva import AuxIVAOracle
    from ssspy_amd.bss.iva import AuxLaplaceIVA

    X = _pinned_mixture("configs2_seed3000_N8_F2049_T1024")
    m = AuxLaplaceIVA(spatial_algorithm="ISS")
    Y = m(X, n_iter=2)
    ref = AuxIVAOracle(spatial_algorithm="ISS", contrast="laplace")
    Yr = ref.run(X, n_iter=2)
    np.testing.assert_allclose(m.loss, ref.loss, rtol=LOSS_RTOL)
    assert rel_err(Y, Yr) < TOL


def test_configs3_full_size_against_oracle():
    """BASELINE configs[3]: FastGaussMNMF, N=M=4, F=1025, T=512, n_basis=8; every parameter after
    one and two iterations against the oracle (ssspy/bss/mnmf.py:1278-1303), then the Wiener-filter
    output (:1174-1217)."""
    from oracle.mnmf import FastGaussMNMFOracle
    from ssspy_amd.bss.mnmf import FastGaussMNMF

    M, F, T, K = 4, 1025, 512, 8
    X = _pinned_mixture("configs3_seed4000_N4_F1025_T512")
    kw = dict(basis=np.random.default_rng(1).random((M, F, K)),
              activation=np.random.default_rng(2).random((M, K, T)),
              spatial=np.random.default_rng(4).random((F, M, M)))
    snaps = []

    def grab(method):
        snaps.append({k: np.array(getattr(method, k)) for k in
                      ("diagonalizer", "spatial", "basis", "activation")})

    m = FastGaussMNMF(n_basis=K, callbacks=grab)
    Y = m(X, n_iter=2, **kw)
    ref = FastGaussMNMFOracle(n_basis=K, record_loss=True)
    ref.reset(X, **{k: v.copy() for k, v in kw.items()})
    ref_loss = [ref.compute_loss()]
    for it in (1, 2):
        ref.update_once()
        ref_loss.append(ref.compute_loss())
        for name in ("diagonalizer", "spatial", "basis", "activation"):
            assert rel_err(snaps[it][name], getattr(ref, name)) < TOL, (it, name)
    np.testing.assert_allclose(m.loss, ref_loss, rtol=LOSS_RTOL)
    assert rel_err(Y, ref.separate(ref.input)) < 1e-7


def test_configs2_full_size_100_iterations_against_oracle():
    """BASELINE configs[2] literally: AuxLaplaceIVA-ISS, N=8, F=2049, T=1024, 100 iterations,
    against 100 oracle iterations on the host (ssspy/bss/iva.py:1917-1966,
    _update_spatial_model.py:146-194).  Loss list 1e-9; spectrograms 1e-6 (100 sweeps of 8
    sources amplify rounding), as for configs[1]."""
    from oracle.iva import AuxIVAOracle
    from ssspy_amd.bss.iva import AuxLaplaceIVA

    X = _pinned_mixture("configs2_seed3000_N8_F2049_T1024")
    m = AuxLaplaceIVA(spatial_algorithm="ISS")
    Y = m(X, n_iter=100)
    ref = AuxIVAOracle(spatial_algorithm="ISS", contrast="laplace")
    Yr = ref.run(X, n_iter=100)
    assert len(m.loss) == 101
    np.testing.assert_allclose(m.loss, ref.loss, rtol=LOSS_RTOL)
    assert rel_err(Y, Yr) < 1e-6


def test_configs3_full_size_100_iterations_against_oracle():
    """BASELINE configs[3] literally: FastGaussMNMF (IP1), N=M=4, F=1025, T=512, n_basis=8, 100
    iterations against 100 oracle iterations (ssspy/bss/mnmf.py:1278-1303): loss list 1e-9, every
    parameter and the Wiener-filter output 1e-6."""
    from oracle.mnmf import FastGaussMNMFOracle
    from ssspy_amd.bss.mnmf import FastGaussMNMF

    M, F, T, K = 4, 1025, 512, 8
    X = _pinned_mixture("configs3_seed4000_N4_F1025_T512")
    kw = dict(basis=np.random.default_rng(1).random((M, F, K)),
              activation=np.random.default_rng(2).random((M, K, T)),
              spatial=np.random.default_rng(4).random((F, M, M)))
    m = FastGaussMNMF(n_basis=K)
    Y = m(X, n_iter=100, **kw)
    ref = FastGaussMNMFOracle(n_basis=K, record_loss=True)
    ref.reset(X, **{k: v.copy() for k, v in kw.items()})
    ref_loss = [ref.compute_loss()]
    for _ in range(100):
        ref.update_once()
        ref_loss.append(ref.compute_loss())
    np.testing.assert_allclose(m.loss, ref_loss, rtol=LOSS_RTOL)
    for name in ("diagonalizer", "spatial", "basis", "activation"):
        assert rel_err(getattr(m, name), getattr(ref, name)) < 1e-6, name
    assert rel_err(Y, ref.separate(ref.input)) < 1e-6


# -- the implied-filter route at the shapes bench.py's `pairwise_ipa` legs quote (round 6) ---------
# Since round 5 the ISS1 / ISS2 / IPA iterations of GaussILRMA (batches; ISS2 / IPA also on one
# mixture) and the ISS2 / IPA iterations of AuxIVA at up to 4 sources carry the filters the updates
# imply instead of Y (W <- G W, statistics W U W^H, Y formed on read).  These are the oracle
# comparisons of exactly that route at N = 4, F = 1025, T = 512: one mixture for 100 iterations and
# the 32-mixture batch of the bench legs for 20.
IMPLIED_LEGS = [("ilrma", "ISS1"), ("ilrma", "ISS2"), ("ilrma", "IPA"), ("iva", "ISS2"), ("iva", "IPA")]
BATCH_PICKS = (0, 17, 31)


@pytest.fixture(scope="module")
def oracle_runs():
    """Every oracle run of the implied-filter tests, started at once in spawned processes (the 100
    iteration runs take 1-3 minutes each on the host; the device tests overlap with them)."""
    import concurrent.futures
    import multiprocessing

    import _oracle_jobs

    jobs = [(fam, algo, 1000, 100) for fam, algo in IMPLIED_LEGS]
    jobs += [(fam, algo, 1000 + b, 20) for fam, algo in IMPLIED_LEGS for b in BATCH_PICKS]
    workers = max(1, min(len(jobs), (os.cpu_count() or 2) // 2))
    pool = concurrent.futures.ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn"))
    futures = {job: pool.submit(_oracle_jobs.run, *job) for job in jobs}
    yield futures
    pool.shutdown(wait=False, cancel_futures=True)


def _separator(family, algo, **kw):
    from ssspy_amd.bss.ilrma import GaussILRMA
    from ssspy_amd.bss.iva import AuxLaplaceIVA

    if family == "ilrma":
        return GaussILRMA(n_basis=16, spatial_algorithm=algo, **kw)
    return AuxLaplaceIVA(spatial_algorithm=algo, **kw)


@pytest.mark.parametrize("family,algo", IMPLIED_LEGS)
def test_implied_filter_route_100_iterations_against_oracle(family, algo, oracle_runs):
    """The pinned configs[1] mixture, 100 iterations of GaussILRMA-ISS1 / ISS2 / IPA and
    AuxLaplaceIVA-ISS2 / IPA against 100 oracle iterations (ssspy/bss/ilrma.py:1635-1908,
    ssspy/bss/iva.py:1968-2175): loss list 1e-9, spectrograms after projection back 1e-6.
    ISS1 on ONE mixture takes the fused sweep on Y by default; it is forced onto the statistics
    (the batch route) here, and checked on its default below."""
    import warnings

    import _oracle_jobs

    X = _pinned_mixture("configs1_seed1000_N4_F1025_T512")
    m = _separator(family, algo)
    kw = {}
    if family == "ilrma":
        kw["basis"], kw["activation"] = _oracle_jobs.initial(1000)
    with _routes.override(iss1_statistics=True if (family, algo) == ("ilrma", "ISS1") else None):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            Y = m(X, n_iter=100, **kw)
    # (the NMF variances of silent sources reach their floor after 60-70 iterations of this mixture
    #  and the route's rounding bound with them: ILRMA then goes on on Y, see _amp_exceeded)
    assert m._implied_iterations() >= 50, "the run left the implied-filter route early"
    if family == "iva":
        assert m._implied is not None
    loss_ref, Y_ref = oracle_runs[(family, algo, 1000, 100)].result()
    assert len(m.loss) == 101
    np.testing.assert_allclose(m.loss, loss_ref, rtol=LOSS_RTOL)
    assert rel_err(Y, Y_ref) < 1e-6


def test_implied_filter_route_batch_of_32_against_oracle(oracle_runs):
    """The workload of bench.py's `pairwise_ipa.*.b32` legs: the first 32 mixtures of the headline
    batch (seeds 1000..1031), 20 iterations of the five implied-filter iterations as ONE batch each;
    mixtures 0, 17 and 31 against 20 oracle iterations (loss 1e-9, spectrograms 1e-7)."""
    import warnings

    import torch

    import _oracle_jobs
    from ssspy_amd.utils.dataset import nmf_mixture_batch, sha256_of

    B, N, F, T = 32, 4, 1025, 512
    pins = json.load(open(os.path.join(HERE, "golden", "input_sha256.json")))
    Xh = nmf_mixture_batch(1000, B, N, F, T)
    assert sha256_of(Xh[0]) == pins["configs1_seed1000_N4_F1025_T512"]["sha256"]
    init = [_oracle_jobs.initial(1000 + b) for b in range(B)]
    basis, act = np.stack([i[0] for i in init]), np.stack([i[1] for i in init])
    X = torch.from_numpy(Xh).to("cuda")
    for family, algo in IMPLIED_LEGS:
        m = _separator(family, algo)
        kw = dict(basis=basis, activation=act) if family == "ilrma" else {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            Y = m(X, n_iter=20, **kw)
        assert m._implied is not None, (family, algo)
        loss = np.asarray(m.loss)
        assert loss.shape == (21, B)
        for b in BATCH_PICKS:
            loss_ref, Y_ref = oracle_runs[(family, algo, 1000 + b, 20)].result()
            np.testing.assert_allclose(loss[:, b], loss_ref, rtol=LOSS_RTOL, err_msg=str((family, algo, b)))
            assert rel_err(Y[b], Y_ref) < 1e-7, (family, algo, b)
        del m, Y
        torch.cuda.empty_cache()


def test_configs3_batch_of_32_equals_single_mixture_runs():
    """configs[3] at the batch bench.py and the profiles quote (32 full-size mixtures, seeds
    4000..4031): three iterations of the batched update_once() -- whole rounds plus a split tail of
    work items, the |Qx|^2 hand-over read by the two-waves-per-SIMD basis / activation passes from
    the second iteration on -- against the single-mixture runs of mixtures 0, 17 and 31 (all-split
    schedule), and the batch without the hand-over."""
    import torch

    from ssspy_amd.bss.mnmf import FastGaussMNMF
    from ssspy_amd.utils.dataset import nmf_mixture_batch, sha256_of

    B, M, F, T, K = 32, 4, 1025, 512, 8
    pins = json.load(open(os.path.join(HERE, "golden", "input_sha256.json")))
    Xh = nmf_mixture_batch(4000, B, M, F, T)
    assert sha256_of(Xh[0]) == pins["configs3_seed4000_N4_F1025_T512"]["sha256"]
    rng = np.random.default_rng(4100)
    kw = dict(basis=rng.random((B, M, F, K)), activation=rng.random((B, M, K, T)),
              spatial=rng.random((B, F, M, M)))
    names = ("diagonalizer", "spatial", "basis", "activation")

    def run(X, sel=None):
        m = FastGaussMNMF(n_basis=K)
        init = {k: (v if sel is None else v[sel]).copy() for k, v in kw.items()}
        Y = m(X, n_iter=3, **init)
        return m, [np.array(getattr(m, k)) for k in names] + [np.array(Y)], np.asarray(m.loss)

    mb, batch, lossb = run(torch.from_numpy(Xh).to("cuda"))
    assert mb._handover is not None and lossb.shape == (4, B)
    for b in (0, 17, 31):
        _, single, loss1 = run(Xh[b], b)
        for name, a, ref in zip(names + ("output",), batch, single):
            assert rel_err(a[b], ref) < 1e-10, (b, name)
        np.testing.assert_allclose(lossb[:, b], loss1, rtol=1e-10)
    with _routes.override(handover=False):
        mp, plain, lossp = run(torch.from_numpy(Xh).to("cuda"))
    assert mp._handover is None
    for name, a, ref in zip(names + ("output",), batch, plain):
        assert rel_err(a, ref) < 1e-10, name
    np.testing.assert_allclose(lossb, lossp, rtol=1e-10)


def test_bench_two_rank_control_flow_on_one_device():
    """bench.py's N > 1 path (rank/world from the environment, barrier, max over ranks, rank 0
    prints) dry-run with two gloo ranks sharing the one GPU of this box, so the multi-rank control
    flow stays runnable while no 8-GPU node is at hand.  Not a scaling measurement."""
    import subprocess
    import sys

    root = os.path.dirname(HERE)
    env = dict(os.environ, SSSPY_BENCH_ONE_DEVICE="1", SSSPY_BENCH_BACKEND="gloo",
               MASTER_ADDR="127.0.0.1", MASTER_PORT="29531")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29531", os.path.join(root, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "4", "--full"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["value"] > 0
    assert out["config"]["global_batch"] == 8 and out["scaling"] == "weak"
    # round 5: per-rank rates and the power of every card while all ranks iterate
    pr = out["per_rank"]
    assert len(pr["mixture_iterations_per_s"]) == 2 and pr["min"] <= pr["median"] <= pr["max"]
    assert pr["slowest_rank"] in (0, 1) and pr["sum"] >= out["value"] * 0.5
    pa = out["roofline"]["power_all_ranks"]
    assert "cards" in pa or "error" in pa


def test_bench_gpus_flag_starts_the_ranks_itself():
    """The driver's command form is plain ``python bench.py --gpus N ...`` (no launcher): bench.py
    must start the N ranks itself and report ``n_gpus == N``.  Dry run on this one-GPU box: both
    ranks on device 0, gloo for the barrier and the timing max (RCCL refuses two ranks on one
    device); on a node the same command runs one RCCL rank per GPU."""
    import subprocess
    import sys

    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(SSSPY_BENCH_ONE_DEVICE="1", SSSPY_BENCH_BACKEND="gloo")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--batch", "4"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 8 and out["value"] > 0


def test_bench_rejects_world_size_mismatch():
    """``--gpus`` is read: a launcher world size that disagrees with it is an error, not a silent
    one-rank run."""
    import subprocess
    import sys

    root = os.path.dirname(HERE)
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1",
                          "--warmup", "0", "--batch", "2", "--no-extra", "--no-cpu-baseline"],
                         env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert res.returncode != 0 and "WORLD_SIZE" in (res.stderr + res.stdout)


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps in one region and prints the headline
    line without the side legs; --dump-outputs holds the state the last timed step left, equal to
    the same warm-up + steps run here through bench.make_separator."""
    import subprocess
    import sys

    import torch

    import bench
    root = os.path.dirname(HERE)
    from ssspy_amd.utils.dataset import nmf_mixture_batch

    B, N, F, T, K, warmup, steps = 4, 4, 33, 64, 16, 1, 2
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", str(warmup), "--batch", str(B), "--sources", str(N), "--bins", str(F),
           "--frames", str(T), "--basis", str(K), "--dump-outputs", str(tmp_path)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["timed_regions"]["count"] == 1
    assert out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"] == "f64"
    assert not {"roofline", "cpu_baseline", "configs", "pairwise_ipa", "call_end_to_end"} & set(out)

    sep = bench.make_separator(torch.from_numpy(nmf_mixture_batch(1000, B, N, F, T)).cuda(), K,
                               seed=2000)
    for _ in range(warmup + steps):
        sep.update_once()
    files = sorted(os.listdir(str(tmp_path)))
    assert files == ["activation.npy", "basis.npy", "demix_filter.npy"]
    for name in ("demix_filter", "basis", "activation"):
        a = np.load(os.path.join(str(tmp_path), name + ".npy"))
        ref = np.asarray(getattr(sep, name))
        if np.iscomplexobj(ref):
            ref = np.stack([ref.real, ref.imag], axis=-1)
        assert a.dtype == np.float64 and a.shape == ref.shape, name
        assert rel_err(a, ref) < 1e-12, name
