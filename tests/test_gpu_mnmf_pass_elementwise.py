"""Every FastGaussMNMF entry point alone -- each ``steps`` bit of ssspy_fastmnmf_update from a fresh
copy of the same state -- element by element against the extended-precision restatement of
tests/mnmf_reference.py (its module docstring spells out the bars: ``m u companion`` per element,
nothing fitted to a measurement, no element left out).  Arrays a step must not touch come back
bitwise.  Inputs carry a NaN band, outputs sit between sentinel bands, workspaces have canaries
(up / Out / check of tests/test_gpu_pass_elementwise.py).

Routes.  Every case asserts the kernel family and the plan ssspy_fastmnmf_route reports for its shape
(csrc/mnmf_plan.hpp: the struct the launchers read), so a case that names a route runs it.

Solves.  The diagonaliser step (IP1) and the Wiener filter get normwise bars:
||q - q_ref|| <= c kappa u ||q_ref|| per bin and row, kappa = max_m kappa_2(Q U_m) of the extended
sweep; ||y - y_ref|| <= c kappa_2(R_ij) u ||x_ij|| per (bin, frame).  c = 8 x the kappa-normalised
error float64 NumPy makes on the same inputs -- np.linalg.solve fed the reference's own U for IP1, the
reference's composition (eigh, floor, solve) for the filter; both numbers are printed and go to the
profile.  The Wiener cases come in two families: to_psd's eigenvalue floor inactive (asserted on the
reference; ADD is R + eps I, exact in the restatement), and MAX with eps = 0.3 on a state scaled so
that the floor moves about half of the eigenvalues (share asserted on the reference, which rebuilds
R from a long-double Jacobi eigendecomposition).

Run as a script on the GPU to rewrite profiles/mnmf_pass_elementwise.txt.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mnmf_reference as mr  # noqa: E402
import pass_reference as pr  # noqa: E402
from test_gpu_pass_elementwise import Out, _mods, check, up  # noqa: E402

pytestmark = pytest.mark.gpu

LD, U = pr.LD, pr.U
MAXF, ADDF, NOF = (pr.FLOOR_MAX, pr.EPS), (pr.FLOOR_ADD, pr.EPS), (pr.FLOOR_NONE, 0.0)
TILED, GENERIC, RUNTIME = range(3)
FAMILY = ["tiled", "generic", "runtime"]
BASIS, ACT, DIAG, SPATIAL, NORM = mr.BASIS, mr.ACTIVATION, mr.DIAGONALIZER, mr.SPATIAL, mr.NORMALIZE
NAMES = ("Q", "D", "basis", "act")


def _line(line):
    print(line)
    path = os.environ.get("SSSPY_PASS_PROFILE_RAW")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _normwise(entry, tag, e, c, c_np, kappa):
    _line("{}\t{}\t{:.2f}\t{:.2f}\t{:.4f}\t(c_np {:.3f}, kappa max {:.1f})".format(
        entry, tag, e, c, e / c, c_np, float(np.max(kappa))))
    assert e <= c, "{} [{}]: error / bar = {:.3f}".format(entry, tag, e / c)


class Case:
    """One shape: host state, its route, and fresh device copies on demand."""

    def __init__(self, B, N, M, F, T, K, family=TILED, expect=None, flooring=MAXF, state=None,
                 seed=None):
        _, self.dv, _, self.ops = _mods()
        self.shape = (B, N, M, F, T, K)
        self.flooring = flooring
        route, self.plan = self.ops.fastmnmf_route(B, N, M, F, T, K)
        assert route == family, "shape reaches {} instead of {}".format(FAMILY[route], FAMILY[family])
        for key, val in (expect or {}).items():
            assert self.plan[key] == val, "{}: plan[{}] = {} instead of {} ({})".format(
                self.shape, key, self.plan[key], val, self.plan)
        seed = seed if seed is not None else B * 7 + N * 5 + M * 11 + F * 3 + T * 2 + K
        self.X, self.C, Q, D, basis, act = state or mr.gen_state(seed, B, N, M, F, T, K)
        self.h = dict(Q=Q, D=D, basis=basis, act=act)
        self.Xd, self.Cd = up(self.X), up(self.C)
        self.ws, self.wsb = self.ops.fastmnmf_workspace(B, N, M, F, T, K, self.dv.device())
        p = self.plan
        form = "fast" if p["fast"] else ("ksmall" if p["ksmall"] else "kwide")
        if family != TILED:
            form = FAMILY[family]
        self.tag = "{}{}{} B{} N{} M{} F{} T{} K{} f{}".format(
            form, "+glds" if p["glds_cov"] else "", "+split" if p["tail_tail"] else "", B, N, M, F,
            T, K, flooring[0])

    def fresh(self, **over):
        h = dict(self.h, **over)
        return {k: Out(h[k].shape, k == "Q", fill=h[k]) for k in NAMES}, h

    def update(self, o, steps, handover=None, valid=False, logdet=None):
        info = self.dv.zeros((1,), self.dv.i32)
        args = (self.Xd, self.Cd, o["Q"].t, o["D"].t, o["basis"].t, o["act"].t, steps, self.flooring,
                self.ws, self.wsb, info)
        if logdet is not None:
            valid = self.ops.fastmnmf_update_logdet(*args, None if handover is None else handover.t,
                                                    valid, logdet.t, self.shape[0])
        elif handover is not None:
            valid = self.ops.fastmnmf_update_handover(*args, handover.t, valid)
        else:
            self.ops.fastmnmf_update(*args)
        assert int(info.item()) == 0
        return valid

    def untouched(self, o, h, *names):
        for k in names:
            assert np.array_equal(o[k].get().view(np.float64), h[k].view(np.float64)), \
                "{}: the step changed {}".format(self.tag, k)

    # ---- one step each, from the same state
    def basis(self, handover=None, valid=False, extra=mr.NO_EXTRA, tag="", **over):
        o, h = self.fresh(**over)
        valid = self.update(o, BASIS, handover, valid)
        ref, bar = mr.update_basis(self.X, h["Q"], h["D"], h["basis"], h["act"], self.flooring,
                                   extra=extra)
        check("fastmnmf_basis" + tag, self.tag, o["basis"].get(), ref, bar)
        self.untouched(o, h, "Q", "D", "act")
        return valid, ref

    def activation(self, handover=None, valid=False, extra=mr.NO_EXTRA, tag="", **over):
        o, h = self.fresh(**over)
        valid = self.update(o, ACT, handover, valid)
        ref, bar = mr.update_activation(self.X, h["Q"], h["D"], h["basis"], h["act"], self.flooring,
                                        extra=extra)
        check("fastmnmf_activation" + tag, self.tag, o["act"].get(), ref, bar)
        self.untouched(o, h, "Q", "D", "basis")
        return valid, ref

    def diagonalizer(self, with_logdet=True):
        B = self.shape[0]
        o, h = self.fresh()
        ref, kappa = mr.update_diagonalizer(self.X, h["Q"], h["D"], h["basis"], h["act"], self.flooring)
        f64 = mr.ip1_yardstick(self.X, h["Q"], h["D"], h["basis"], h["act"], self.flooring)
        c_np = pr.ip1_row_error(f64, ref, kappa)
        shares = None
        if with_logdet:
            ns = self.plan["logdet_slots"]
            shares = Out((ns, B), fill=np.zeros((ns, B)))
        self.update(o, DIAG, logdet=shares)
        e = pr.ip1_row_error(o["Q"].get(), ref, kappa)
        _normwise("fastmnmf_diagonalizer" + ("_logdet" if with_logdet else ""), self.tag, e, 8 * c_np,
                  c_np, kappa)
        self.untouched(o, h, "D", "basis", "act")
        if with_logdet:
            shares.get()
            ld = Out((B,))
            self.ops.fold_scalar_slots(shares.t, B, ns, ld.t)
            lref, lbar = pr.sum_logdet(h["Q"])
            check("fastmnmf_update_logdet", self.tag, ld.get(), lref, lbar + ns * U * np.abs(lref))

    def spatial(self, handover=None, tag=""):
        """handover: the pass also writes the buffer (the LDS-DMA spatial kernel, or P_WRITE)."""
        o, h = self.fresh()
        valid = self.update(o, SPATIAL, handover, False)
        ref, bar = mr.update_spatial(self.X, h["Q"], h["D"], h["basis"], h["act"])
        check("fastmnmf_spatial" + tag, self.tag, o["D"].get(), ref, bar)
        self.untouched(o, h, "Q", "basis", "act")
        return o, valid

    def normalize(self, tag="", **over):
        o, h = self.fresh(**over)
        self.update(o, NORM)
        Qn, barQ, Dn, barD, psi = mr.normalize(h["Q"], self.C, h["D"], self.flooring)
        check("fastmnmf_normalize_Q" + tag, self.tag, o["Q"].get(), Qn, barQ)
        check("fastmnmf_normalize_D" + tag, self.tag, o["D"].get(), Dn, barD)
        self.untouched(o, h, "basis", "act")
        return psi

    def spatial_normalize(self, handover=None, tag=""):
        """SPATIAL | NORMALIZE in one call against the composed reference."""
        o, h = self.fresh()
        valid = self.update(o, SPATIAL | NORM, handover, False)
        D1, bar1 = mr.update_spatial(self.X, h["Q"], h["D"], h["basis"], h["act"])
        Qn, barQ, Dn, barD, _ = mr.normalize(h["Q"], self.C, D1, self.flooring,
                                             D_rel_u=bar1 / (U * D1))
        check("fastmnmf_spatial_normalize_Q" + tag, self.tag, o["Q"].get(), Qn, barQ)
        check("fastmnmf_spatial_normalize_D" + tag, self.tag, o["D"].get(), Dn, barD)
        self.untouched(o, h, "basis", "act")
        return o, valid

    def operators(self, cov="tiled"):
        """weights, loss_data, diagonalizer_covariance (`cov`: tiled -- with and without the workspace
        --, fused, or unsupported)."""
        B, N, M, F, T, K = self.shape
        h = self.h
        d = {k: up(h[k]) for k in NAMES}
        ref, bar = mr.fastmnmf_weights(h["D"], h["basis"], h["act"])
        o = Out((B, M, F, T))
        self.ops.fastmnmf_weights(self.Xd, d["Q"], d["D"], d["basis"], d["act"], out=o.t)
        check("fastmnmf_weights", self.tag, o.get(), ref, bar)
        ref, bar = mr.loss_data(self.X, h["Q"], h["D"], h["basis"], h["act"])
        o = Out((B,))
        self.ops.fastmnmf_loss_data(self.Xd, d["Q"], d["D"], d["basis"], d["act"], out=o.t)
        check("fastmnmf_loss_data", self.tag, o.get(), ref, bar)
        if cov == "unsupported":
            o = Out((B, F, M, M, M), True)
            with pytest.raises(NotImplementedError):
                self.ops.fastmnmf_diagonalizer_covariance(self.Xd, d["D"], d["basis"], d["act"], out=o.t)
            return
        ref, bar = mr.fastmnmf_diagonalizer_covariance(self.X, h["D"], h["basis"], h["act"])
        for name, kw in (("", {"ws": self.ws, "ws_bytes": self.wsb}), ("_no_ws", {})):
            o = Out((B, F, M, M, M), True)
            self.ops.fastmnmf_diagonalizer_covariance(self.Xd, d["D"], d["basis"], d["act"], out=o.t,
                                                      **kw)
            check("fastmnmf_diagonalizer_covariance" + name, self.tag, o.get(), ref, bar)

    def separate(self, flooring=None, tag="", active=False):
        """active: the MAX floor moves a share of the eigenvalues of R_ij (asserted on the reference)."""
        B, N, M, F, T, K = self.shape
        flooring = flooring or self.flooring
        h = self.h
        ref_id = M - 1
        Y, kappa, lam = mr.separate(self.X, h["Q"], h["D"], h["basis"], h["act"], ref_id, flooring,
                                    eig=active)
        if active:
            share = float(np.mean(lam < flooring[1]))
            assert 0.3 < share < 0.7, "floored share of the eigenvalues {}".format(share)
            assert np.all(np.any(lam < flooring[1], axis=-1).reshape(B, -1).mean(axis=1) > 0.5)
        elif flooring[0] != pr.FLOOR_ADD:
            assert float(lam.min()) > 1e3 * flooring[1]  # the eigenvalue floor is inactive
        Yf = mr.separate_float64(self.X, h["Q"], h["D"], h["basis"], h["act"], ref_id, flooring)
        c_np = mr.separate_error(Yf, Y, self.X, kappa)
        info = self.dv.zeros((1,), self.dv.i32)
        o = Out((B, N, F, T), True)
        self.ops.fastmnmf_separate(self.Xd, up(h["Q"]), up(h["D"]), up(h["basis"]), up(h["act"]),
                                   ref_id, flooring, self.ws, self.wsb, info, out=o.t)
        got = o.get()
        assert np.all(np.isfinite(got.view(np.float64))) and int(info.item()) == 0
        e = mr.separate_error(got, Y, self.X, kappa)
        _normwise("fastmnmf_separate" + tag, self.tag + " floor{}".format(flooring[0]), e, 8 * c_np,
                  c_np, kappa)

    def all_steps(self, cov="tiled", separate=True):
        self.basis()
        self.activation()
        self.diagonalizer()
        self.spatial()
        self.normalize()
        self.spatial_normalize()
        self.operators(cov)
        if separate:
            self.separate()

    # ---- the |Q x|^2 hand-over
    def handover_out(self):
        _, lib, _ = _mods()[1:]
        n = int(lib.load().ssspy_fastmnmf_handover_doubles(*self.shape))
        assert n == self.shape[0] * self.shape[2] * (self.shape[3] * self.shape[4] + 1)
        return Out((n,), fill=np.full(n, np.nan))  # (a pass that reads it before it is built shows)

    def handover_product(self, ho):
        B, N, M, F, T, K = self.shape
        buf = ho.get()
        return buf[:B * M * F * T].reshape(B, M, F, T) * buf[B * M * F * T:].reshape(B, M, 1, 1)


# ------------------------------------------------------------------------------- tiled: the forms
TILED_MN = [(2, 2), (3, 3), (4, 4), (3, 2), (4, 3), (2, 4)]


def _tiled_expect(T, K):
    fast = K <= 16
    return {"fast": int(fast), "ksmall": int(fast), "basis_copy": int(K > 16),
            "glds_cov": int(fast and T % 16 == 0), "handover": int(fast and T % 2 == 0),
            "kq": 2 if K <= 8 else 4 if K <= 16 else 0}


@pytest.mark.parametrize("K", [3, 8, 9, 16, 17, 40])
@pytest.mark.parametrize("T", [32, 33, 34])
@pytest.mark.parametrize("M,N", TILED_MN)
def test_tiled_forms(M, N, T, K):
    """T = 32: throughput form with LDS-DMA; 34: register-fed, hand-over available; 33: odd, no
    hand-over.  K = 3, 8 / 9, 16: both KQ variants; 17 and 40: the KSMALL = false kernels, the basis
    copy and several k tiles.  Two mixtures of one bin group: every item split (IP1 from the
    records, the spatial fold inside the normalisation) up to 16 bases."""
    exp = _tiled_expect(T, K)
    exp.update(ip1_records=int(K <= 16), spatial_fold_in_norm=int(K <= 16))
    Case(2, N, M, 17, T, K, expect=exp).all_steps()


@pytest.mark.parametrize("F", [65, 129])
@pytest.mark.parametrize("T,K", [(32, 8), (34, 16), (33, 17)])
def test_tiled_bin_edges(F, T, K):
    """A bin group that ends inside a wave's 16 bins (F = 65: the second group holds one bin) and
    waves without a bin (129: the third group)."""
    c = Case(1, 3, 3, F, T, K, expect=_tiled_expect(T, K))
    assert c.plan["tail_groups"] == (F + 63) // 64 or K > 16
    c.all_steps()


_NOFAST_ARG = "--nofast-child"


def _nofast_child():
    for (M, N), K in zip(TILED_MN[:4], (3, 8, 9, 16)):
        exp = {"fast": 0, "ksmall": 1, "handover": 0, "glds_cov": 0, "tail_tail": 0, "ip1_records": 0}
        Case(2, N, M, 17, 32, K, expect=exp).all_steps()
    print("nofast child OK")


def test_tiled_fast_path_disabled_in_a_child():
    """SSSPY_AMD_NO_FAST is read once per process: the KSMALL = true kernels at K <= 16 run in a
    fresh child (this file as a script)."""
    env = dict(os.environ, SSSPY_AMD_NO_FAST="1", SSSPY_AMD_WS_CANARY="1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), _NOFAST_ARG], env=env,
                         capture_output=True, text=True, timeout=600)
    sys.stdout.write(res.stdout)
    assert res.returncode == 0 and "nofast child OK" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


# ------------------------------------------------------------------------------- tail plans
def test_one_mixture_every_item_split():
    """One mixture: the covariance records are folded by IP1 itself, the spatial fold runs inside the
    normalisation (SPATIAL alone folds in its own kernel: both against the composed reference)."""
    c = Case(1, 2, 2, 17, 32, 4, expect={"tail_full": 0, "tail_tail": 1, "tail_split": 2,
                                         "ip1_records": 1, "spatial_fold_in_norm": 1,
                                         "logdet_slots": 2})
    c.all_steps()
    c.diagonalizer(with_logdet=False)


def test_whole_and_split_items_in_one_launch():
    """B = 257, F = 17, T = 32: 256 whole items and one split item."""
    c = Case(257, 2, 2, 17, 32, 3, expect={"tail_full": 256, "tail_tail": 1, "tail_split": 2,
                                           "ip1_records": 0, "spatial_fold_in_norm": 0})
    c.basis()
    c.activation()
    c.diagonalizer()
    c.spatial()
    c.normalize()
    c.spatial_normalize()
    c.operators()


def test_handover_basis_plan_whole_and_split_items():
    """B = 171, F = 129, T = 32 with a valid hand-over: 513 items on the 512-slot plan of the
    hand-over basis and loss passes, 512 whole and one split."""
    c = Case(171, 2, 2, 129, 32, 3, expect={"htail_full": 512, "htail_tail": 1, "htail_split": 2,
                                            "htail_groups": 3, "handover": 1})
    ho = c.handover_out()
    valid, _ = c.basis(ho, False, mr.HANDOVER_P, "_handover_rebuilt")
    assert valid
    _loss_from_handover(c, ho)
    # the same pass from a buffer left by a preceding SPATIAL call
    ho = c.handover_out()
    o, valid = c.spatial(ho, "_handover")
    assert valid
    keep = ho.get().copy()
    ho2 = Out(keep.shape, fill=keep)
    valid, _ = c.basis(ho2, True, mr.HANDOVER_P, "_handover_spatial", D=o["D"].get().copy())
    assert valid and np.array_equal(ho2.get(), keep)


# ------------------------------------------------------------------------------- hand-over
def _loss_from_handover(c, ho):
    B, N, M, F, T, K = c.shape
    h = c.h
    d = {k: up(h[k]) for k in NAMES}
    ref, bar = mr.loss_data(c.X, h["Q"], h["D"], h["basis"], h["act"], extra=mr.HANDOVER_P)
    o = Out((B,))
    c.ops.fastmnmf_loss_data_handover(d["D"], d["basis"], d["act"], ho.t, M, T, out=o.t)
    check("fastmnmf_loss_data_handover", c.tag, o.get(), ref, bar)
    ns = c.ops.fastmnmf_loss_handover_slots(*c.shape)
    assert ns == c.plan["loss_slots"] > 0
    slots = Out((ns, B), fill=np.zeros((ns, B)))
    c.ops.fastmnmf_loss_data_handover_slots(d["D"], d["basis"], d["act"], ho.t, M, T, slots.t, B)
    slots.get()
    o2 = Out((B,))
    c.ops.fold_scalar_slots(slots.t, B, ns, o2.t)
    check("fastmnmf_loss_data_handover_slots", c.tag, o2.get(), ref, bar + ns * U * np.abs(ref))
    plain = Out((B,))
    c.ops.fastmnmf_loss_data(c.Xd, d["Q"], d["D"], d["basis"], d["act"], out=plain.t)
    pref, pbar = mr.loss_data(c.X, h["Q"], h["D"], h["basis"], h["act"])
    check("fastmnmf_loss_data", c.tag, plain.get(), pref, pbar)
    assert np.all(np.abs(plain.get() - o.get()) <= np.asarray(bar + pbar, dtype=np.float64))


@pytest.mark.parametrize("M,N,T,K", [(2, 2, 32, 3), (3, 2, 34, 8), (4, 3, 32, 9), (4, 4, 34, 16),
                                     (3, 3, 32, 16)])
def test_handover(M, N, T, K):
    """The basis and activation steps from a buffer that is rebuilt inside the call (*valid = 0), left
    by a SPATIAL call, and left by SPATIAL | NORMALIZE (pscale != 1: the buffer holds |Q x|^2 of the
    rows before their division); *valid after every step subset; the buffer as the product
    P pscale; the losses from it."""
    exp = _tiled_expect(T, K)
    c = Case(2, N, M, 17, T, K, expect=exp)
    _, hplan = c.ops.fastmnmf_route(*c.shape, handover=True)
    assert hplan["glds_spatial"] == exp["glds_cov"] and hplan["handover"] == 1
    # rebuilt inside the call
    for step in (c.basis, c.activation):
        ho = c.handover_out()
        valid, _ = step(ho, False, mr.HANDOVER_P, "_handover_rebuilt")
        assert valid
        ref, bar = mr.handover_buffer(c.X, c.h["Q"])
        check("fastmnmf_handover_buffer_rebuilt", c.tag, c.handover_product(ho), ref, bar)
    # *valid on return: steps that move Q without a spatial pass behind them leave it invalid
    for steps, want in ((BASIS | ACT, True), (DIAG, False), (DIAG | SPATIAL, True), (NORM, False),
                        (SPATIAL | NORM, True), (BASIS | DIAG, False)):
        o, _ = c.fresh()
        assert c.update(o, steps, c.handover_out(), False) == want, steps
    # left by SPATIAL, and by SPATIAL | NORMALIZE
    for steps, name in ((SPATIAL, "_handover_spatial"), (SPATIAL | NORM, "_handover_normalized")):
        # the spatial pass that writes the buffer (LDS-DMA at T % 16 == 0, else P_WRITE) and the
        # normalisation that stores the fresh scale: D and Q elementwise, the rest bitwise
        ho = c.handover_out()
        o, valid = (c.spatial if steps == SPATIAL else c.spatial_normalize)(ho, "_handover")
        assert valid
        Q1, D1 = o["Q"].get().copy(), o["D"].get().copy()
        ref, bar = mr.handover_buffer(c.X, Q1)
        check("fastmnmf_handover_buffer" + name, c.tag, c.handover_product(ho), ref, bar)
        if steps & NORM:
            buf = ho.get()
            assert np.all(buf[-c.shape[0] * M:] != 1.0)  # pscale carries the normalisation
        keep = ho.get().copy()
        for step in (c.basis, c.activation):
            ho2 = Out(keep.shape, fill=keep)
            valid, _ = step(ho2, True, mr.HANDOVER_P, name, Q=Q1, D=D1)
            assert valid and np.array_equal(ho2.get(), keep)  # read, not rebuilt
    # a NORMALIZE call of its own on a valid buffer divides the scale it finds; a second one finds
    # rows already normalised (psi = 1 up to rounding).  Each call rounds the rows of Q and the scale
    # once more: HANDOVER_P's budget again, less than one whole bar per call
    ho = c.handover_out()
    o, valid = c.spatial(ho, "_handover")
    assert valid
    for rep in (1, 2):
        Q0, D0 = o["Q"].get().copy(), o["D"].get().copy()
        assert c.update(o, NORM, ho, True)
        Qn, barQ, Dn, barD, _ = mr.normalize(Q0, c.C, D0, c.flooring)
        check("fastmnmf_normalize_Q_handover", c.tag, o["Q"].get(), Qn, barQ)
        check("fastmnmf_normalize_D_handover", c.tag, o["D"].get(), Dn, barD)
        c.untouched(o, c.h, "basis", "act")
        ref, bar = mr.handover_buffer(c.X, o["Q"].get())
        check("fastmnmf_handover_buffer_renormalized", c.tag, c.handover_product(ho), ref,
              bar * (1 + rep))
    ho = c.handover_out()
    o, _ = c.fresh()
    assert c.update(o, SPATIAL, ho, False)
    _loss_from_handover(c, ho)


# ------------------------------------------------------------------------------- generic, runtime
@pytest.mark.parametrize("K", [5, 8, 9, 20])
@pytest.mark.parametrize("M,N", [(5, 5), (6, 2), (8, 8), (3, 1), (2, 6)])
def test_generic_family(M, N, K):
    """5..8 channels or sources (and a single source): fmnmf_generic.hip; KT = 8 on both sides of
    8 bases; T = 65: a second block of one frame.  diagonalizer_covariance is unsupported there."""
    Case(2, N, M, 9, 65, K, family=GENERIC).all_steps(cov="unsupported")


@pytest.mark.parametrize("K", [4, 9])
@pytest.mark.parametrize("B,M,N", [(2, 9, 9), (1, 16, 3), (2, 4, 12), (1, 16, 16)])
def test_runtime_family(B, M, N, K):
    """9..16 channels or sources: fmnmf_rt.hip, with the fused diagonaliser covariance."""
    Case(B, N, M, 9, 40, K, family=RUNTIME).all_steps(cov="fused")


# ------------------------------------------------------------------------------- floors
FLOOR_SHAPES = [(2, 3, 3, 17, 32, 8, TILED), (2, 2, 3, 17, 33, 17, TILED), (1, 5, 5, 9, 65, 8, GENERIC),
                (1, 3, 9, 9, 40, 4, RUNTIME)]


@pytest.mark.parametrize("flooring", [MAXF, ADDF, NOF])
@pytest.mark.parametrize("B,N,M,F,T,K,family", FLOOR_SHAPES)
def test_floors(B, N, M, F, T, K, family, flooring):
    """Updated basis and activation values on both sides of eps (a share of them floored: asserted on
    the reference), psi floored on a known set of rows; MAX, ADD and NONE."""
    c = Case(B, N, M, F, T, K, family=family, flooring=flooring,
             state=mr.gen_floor_state(7 + M, B, N, M, F, T, K))
    for step in (c.basis, c.activation):
        _, ref = step()
        if flooring[0] == pr.FLOOR_MAX:
            share = float(np.mean(ref == LD(pr.EPS)))
            assert 0.05 < share < 0.95, "floored share {}".format(share)
    c = Case(B, N, M, F, T, K, family=family, flooring=flooring)
    Qs, floored = mr.gen_floor_rows(c.h["Q"], c.C)
    psi = c.normalize("_floored", Q=Qs)
    if flooring[0] == pr.FLOOR_MAX:
        assert np.array_equal(psi == LD(pr.EPS), floored)


@pytest.mark.parametrize("flooring", [MAXF, ADDF, (pr.FLOOR_ADD, 0.3)])
@pytest.mark.parametrize("K", [8, 16, 17])
def test_separate_floors(K, flooring):
    """The closed-form kernels at K <= 8 and K <= 16 and the general one above (MAX, floor inactive);
    ADD leaves the closed forms: eps = 1e-10 and eps = 0.3, where R + eps I is far from R."""
    c = Case(2, 3, 3, 17, 33, K, expect={"kq": 2 if K <= 8 else 4 if K <= 16 else 0})
    c.separate(flooring)


@pytest.mark.parametrize("B,N,M,F,T,K,family", [
    (2, 3, 3, 17, 33, 8, TILED), (2, 2, 4, 17, 33, 16, TILED), (2, 4, 2, 17, 33, 17, TILED),
    (1, 3, 3, 65, 32, 3, TILED), (1, 5, 5, 9, 65, 8, GENERIC), (1, 3, 9, 9, 40, 4, RUNTIME)])
def test_separate_active_eigenvalue_floor(B, N, M, F, T, K, family):
    """MAX with eps = 0.3 on a state scaled so that the floor of to_psd moves about half of the
    eigenvalues of R_ij, in most points of every mixture (both asserted on the reference): the bins
    the closed-form kernels (K <= 8, K <= 16) hand to the general one, the general kernel above 16
    bases, and the floored branch of the generic and run-time families.  Same normwise bar; c from
    the float64 composition (eigh, floor, rebuild, solve)."""
    eps = 0.3
    exp = {"kq": 2 if K <= 8 else 4 if K <= 16 else 0} if family == TILED else None
    c = Case(B, N, M, F, T, K, family=family, expect=exp,
             state=mr.gen_wiener_floor_state(9 + M + K, B, N, M, F, T, K, eps))
    c.separate((pr.FLOOR_MAX, eps), "_active_floor", active=True)


# ------------------------------------------------------------------------------- profile
def _write_profile(raw, path):
    worst = {}
    for line in open(raw):
        f = line.rstrip("\n").split("\t")
        key = (f[0], f[1].split(" ")[0])
        if key not in worst or float(f[4]) > float(worst[key][4]):
            worst[key] = f
    with open(path, "w") as out:
        out.write("# largest measured error of every FastGaussMNMF entry point and route, tests/test_gpu_"
                  "mnmf_pass_elementwise.py on an MI355X\n# entry point, route: worst case; error and bar "
                  "in units of u = 2^-53 of the reference value at the worst element (normwise entries: "
                  "in units of kappa u); ratio = error / bar\n")
        for key in sorted(worst):
            f = worst[key]
            out.write("{:44s} {:52s} err {:>10s} u  bar {:>10s} u  ratio {}{}\n".format(
                f[0], f[1], f[2], f[3], f[4], "  " + f[5] if len(f) > 5 else ""))


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if _NOFAST_ARG in sys.argv:
        sys.path.insert(0, root)
        _nofast_child()
        sys.exit(0)
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles")
    raw = os.path.join(out_dir, "mnmf_pass_elementwise.raw")
    if os.path.exists(raw):
        os.remove(raw)
    os.environ["SSSPY_PASS_PROFILE_RAW"] = raw
    rc = pytest.main([os.path.abspath(__file__), "-m", "gpu", "-q", "--maxfail=15", "--durations=8"]
                     + sys.argv[2:])
    if os.path.exists(raw):
        _write_profile(raw, os.path.join(out_dir, "mnmf_pass_elementwise.txt"))
        os.remove(raw)
    sys.exit(int(rc))
