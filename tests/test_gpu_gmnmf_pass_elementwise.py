"""Every GaussMNMF entry point alone -- each ``steps`` bit of ssspy_gmnmf_update from a fresh copy of
the same state, ssspy_gmnmf_loss and ssspy_gmnmf_separate -- element by element against the
extended-precision restatement of tests/gmnmf_reference.py (its module docstring spells out the bars;
the solve constants are 8 x the float64 yardsticks measured on the CPU, no element left out).  Arrays a
step must not touch come back bitwise.  Inputs carry a NaN band, outputs sit between sentinel bands,
the workspace is exactly ssspy_gmnmf_workspace_bytes with a canary behind it (up / Out / check of
tests/test_gpu_pass_elementwise.py).

Routes.  Every case first asserts the entries of ssspy_gmnmf_route (csrc/gmnmf_plan.hpp: the struct
the launchers read) that it claims to exercise.  The repair cases also read the flag words the packed
kernels leave in the workspace, at the plan's FLAGS_OFFSET.

Run as a script on the GPU to rewrite profiles/gmnmf_pass_elementwise.txt.
"""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmnmf_reference as gr  # noqa: E402
import mnmf_reference as mr  # noqa: E402
import pass_reference as pr  # noqa: E402
from test_gpu_mnmf_pass_elementwise import _line, _normwise  # noqa: E402
from test_gpu_pass_elementwise import Out, _mods, check, up  # noqa: E402

pytestmark = pytest.mark.gpu

LD, U = pr.LD, pr.U
MAXF, ADDF, NOF = (pr.FLOOR_MAX, pr.EPS), (pr.FLOOR_ADD, pr.EPS), (pr.FLOOR_NONE, 0.0)
LITERAL, PACKED, ROWS8 = range(3)
REGISTERS, LDS_TILE, MEMORY = range(3)
BASIS, ACT, SPATIAL, NORM, LATENT = gr.BASIS, gr.ACTIVATION, gr.SPATIAL, gr.NORMALIZE, gr.LATENT
NAMES = ("basis", "act", "H", "latent")


class Case:
    """One shape: host state, its plan, the shared long-double points and fresh device copies."""

    def __init__(self, B, N, M, F, T, K, expect=None, flooring=MAXF, part=False, state=None):
        _, self.dv, _, self.ops = _mods()
        self.shape, self.flooring, self.part = (B, N, M, F, T, K), flooring, part
        self.plan = self.ops.gmnmf_route(B, N, M, F, T, K, partitioning=part)
        for key, val in (expect or {}).items():
            assert self.plan[key] == val, "{}: plan[{}] = {} instead of {} ({})".format(
                self.shape, key, self.plan[key], val, self.plan)
        seed = B * 7 + N * 5 + M * 11 + F * 3 + T * 2 + K
        self.X, basis, act, H, z = state or gr.gen_state(seed, B, N, M, F, T, K, part)
        self.h = dict(basis=basis, act=act, H=H, latent=z)
        self.Xd = up(self.X)
        self.ws, self.wsb = self.ops.gmnmf_workspace(B, N, M, F, T, K, self.dv.device())
        p = self.plan
        self.tag = "{}{}/s{}/b{}{} B{} N{} M{} F{} T{} K{} f{}".format(
            "packed{}".format(p["trace_sources"]) if p["packed"] else "full",
            "+wide" if p["wide"] else "", p["spatial_form"], p["basis_form"],
            "+part" if part else "", B, N, M, F, T, K, flooring[0])
        self._pt = None

    @property
    def pt(self):
        if self._pt is None:
            h = self.h
            self._pt = gr.Points(self.X, h["basis"], h["act"], h["H"], self.flooring, h["latent"])
        return self._pt

    def ref_args(self):
        h = self.h
        return (self.X, h["basis"], h["act"], h["H"], self.flooring, h["latent"])

    def fresh(self):
        h = self.h
        return {k: Out(h[k].shape, k == "H", fill=h[k]) for k in NAMES if h[k] is not None}

    def update(self, o, steps):
        self.ops.gmnmf_update(self.Xd, o["basis"].t, o["act"].t, o["H"].t, steps, self.flooring,
                              self.ws, self.wsb, latent=o["latent"].t if self.part else None)

    def untouched(self, o, *names):
        for k in names:
            if self.h[k] is not None:
                assert np.array_equal(o[k].get().view(np.float64),
                                      np.ascontiguousarray(self.h[k]).view(np.float64)), \
                    "{}: the step changed {}".format(self.tag, k)

    def flags(self, count):
        torch = _mods()[0]
        off = self.plan["flags_offset"]
        assert off % 4 == 0 and off + 4 * count <= self.wsb
        return self.ws.view(torch.int32)[off // 4: off // 4 + count].cpu().numpy()

    # ---- one step each, from the same state
    def basis(self):
        o = self.fresh()
        self.update(o, BASIS)
        ref, bar = gr.update_basis(*self.ref_args(), pt=self.pt)
        check("gmnmf_basis", self.tag, o["basis"].get(), ref, bar)
        self.untouched(o, "act", "H", "latent")

    def activation(self):
        o = self.fresh()
        self.update(o, ACT)
        ref, bar = gr.update_activation(*self.ref_args(), pt=self.pt)
        check("gmnmf_activation", self.tag, o["act"].get(), ref, bar)
        self.untouched(o, "basis", "H", "latent")

    def spatial(self):
        o = self.fresh()
        self.update(o, SPATIAL)
        ref, bar, moved, kap = gr.update_spatial(*self.ref_args(), pt=self.pt)
        got = o["H"].get()
        assert np.all(np.isfinite(got.view(np.float64)))
        e = gr.spatial_error(got, ref, kap)
        _normwise("gmnmf_spatial", self.tag, e, gr.C["gmean"], gr.MEASURED["gmean"], kap)
        self.untouched(o, "basis", "act", "latent")
        return moved

    def normalize(self):
        o = self.fresh()
        self.update(o, NORM)
        Hn, barH, Tn, barT = gr.normalize(self.h["basis"], self.h["H"], self.h["latent"])
        check("gmnmf_normalize_H", self.tag, o["H"].get(), Hn, barH)
        if self.part:  # with partitioning the scale cannot move into the shared basis
            self.untouched(o, "basis")
        else:
            check("gmnmf_normalize_basis", self.tag, o["basis"].get(), Tn, barT)
        self.untouched(o, "act", "latent")

    def latent(self):
        o = self.fresh()
        self.update(o, LATENT)
        ref, bar = gr.update_latent(*self.ref_args(), pt=self.pt)
        check("gmnmf_latent", self.tag, o["latent"].get(), ref, bar)
        self.untouched(o, "basis", "act", "H")

    def _pair(self):
        """The per-source pair ssspy_gmnmf_loss / _separate take (float64 expansion, as the caller's)."""
        h = self.h
        Te, Vr = gr.expand(h["basis"], h["act"], h["latent"], np.float64)
        return np.ascontiguousarray(Te), np.ascontiguousarray(Vr)

    def loss(self):
        B = self.shape[0]
        Te, Vr = self._pair()
        ref, bar, _ = gr.loss(self.X, Te, Vr, self.h["H"], self.flooring,
                              pt=None if self.part else self.pt)
        o = Out((B,))
        self.ops.gmnmf_loss(self.Xd, up(Te), up(Vr), up(self.h["H"]), self.flooring, out=o.t)
        check("gmnmf_loss", self.tag, o.get(), ref, bar)

    def separate(self):
        B, N, M, F, T, K = self.shape
        Te, Vr = self._pair()
        Y, pt = gr.separate(self.X, Te, Vr, self.h["H"], M - 1, self.flooring,
                            pt=None if self.part else self.pt)
        o = Out((B, N, F, T), True)
        self.ops.gmnmf_separate(self.Xd, up(Te), up(Vr), up(self.h["H"]), M - 1, self.flooring, out=o.t)
        got = o.get()
        assert np.all(np.isfinite(got.view(np.float64)))
        e = mr.separate_error(got, Y, self.X, pt.kappa)
        _normwise("gmnmf_separate", self.tag, e, gr.C["separate"], gr.MEASURED["separate"], pt.kappa)

    def all_steps(self):
        self.basis()
        self.activation()
        moved = self.spatial()
        self.normalize()
        if self.part:
            self.latent()
        self.loss()
        self.separate()
        return moved


def _form_expect(N, M):
    return {"packed": int(M >= 4), "trace_sources": 0 if M < 4 else (4 if N <= 4 else 8),
            "wide": int(N > 8), "spatial_form": LITERAL if M < 4 else (PACKED if M <= 6 else ROWS8),
            "basis_form": REGISTERS, "basis_bpw": 1}


# ------------------------------------------------------------------------------- forms
@pytest.mark.parametrize("flooring", [MAXF, ADDF, NOF])
@pytest.mark.parametrize("T", [40, 129])
@pytest.mark.parametrize("N", [1, 4, 5, 8, 9, 16])
@pytest.mark.parametrize("M", [2, 3, 4, 5, 6, 7, 8])
def test_forms(M, N, T, flooring):
    """Full-storage kernels (2, 3 channels), packed point kernels compiled for 4 and 8 sources, the
    16-source forms; literal, packed and 8-lane spatial updates.  T = 129: the second 128-frame block
    has one live lane."""
    exp = _form_expect(N, M)
    exp["point_blocks"] = (T + 127) // 128 * 9 * 2
    Case(2, N, M, 9, T, 3, expect=exp, flooring=flooring).all_steps()


# ------------------------------------------------------------------------------- basis forms
@pytest.mark.parametrize("T,form,kc", [(512, REGISTERS, 8), (513, LDS_TILE, 7), (4096, LDS_TILE, 1),
                                       (4097, MEMORY, 0)])
def test_basis_forms(T, form, kc):
    """Rows of A / Bt in registers; the LDS tile with 9 basis indices as 7 + 2, then one at a time;
    the activation straight from memory."""
    Case(1, 2, 2, 5, T, 9, expect={"basis_form": form, "basis_kc": kc}).basis()


def test_basis_lds_tile_raw_sums():
    """T = 513 with latent variables: k_gmnmf_basis writes the (num, den) pairs (`raw`), for the
    basis and for the latent step."""
    c = Case(1, 2, 2, 5, 513, 9, expect={"basis_form": LDS_TILE, "basis_kc": 7}, part=True)
    c.basis()
    c.latent()


def test_basis_two_bins_per_wave_ragged_workgroup():
    """513 bins in workgroups of 8: the last one holds a single bin."""
    Case(4, 8, 2, 513, 4, 2, expect={"basis_bpw": 2, "basis_form": REGISTERS}).basis()


# ------------------------------------------------------------------------------- activation chunks
@pytest.mark.parametrize("F,chunks,bpc", [(8, 1, 8), (9, 2, 5), (17, 3, 6), (130, 16, 9)])
def test_activation_chunks(F, chunks, bpc):
    """One chunk, two, ragged waves, and 16 chunks of 9 bins of which the last is empty and the one
    before holds 4; K = 9: the second k-slab has one live index."""
    Case(1, 1, 2, F, 40, 9, expect={"act_chunks": chunks, "act_bins_per_chunk": bpc,
                                    "act_kslabs": 2}).activation()


# ------------------------------------------------------------------------------- repair
@pytest.mark.parametrize("M", [4, 6, 8])
def test_point_repair(M):
    """MAX floor with eps = 0.3; at three frames of the first 128-frame block the floor moves
    eigenvalues of R_ij, nowhere else: the packed kernels flag exactly those blocks and the
    full-storage kernels redo them."""
    eps, frames = 0.3, (3, 64, 127)
    B, N, F, T, K = 1, 3, 9, 200, 3
    c = Case(B, N, M, F, T, K, expect={"packed": 1, "point_blocks": 2 * F * B},
             flooring=(pr.FLOOR_MAX, eps),
             state=gr.gen_repair_points(5 + M, B, N, M, F, T, K, eps, frames))
    lo = c.pt.ev_raw.min(axis=-1)                                  # (B,F,T)
    chosen = np.zeros(T, bool)
    chosen[list(frames)] = True
    assert np.all(lo[:, :, chosen] < eps) and np.all(lo[:, :, ~chosen] > np.sqrt(M) * eps)
    c.basis()
    flags = c.flags(c.plan["point_blocks"]).reshape(B, F, 2)      # [b][i][frame block]
    assert np.all(flags[:, :, 0] == 1) and np.all(flags[:, :, 1] == 0)
    c.activation()
    c.spatial()
    c.loss()
    c.separate()


@pytest.mark.parametrize("M,form", [(4, PACKED), (7, ROWS8)])
def test_spatial_repair(M, form):
    """One silent bin: to_psd of P and of H Q H floors there (asserted on the reference).  The packed
    spatial updates floor H Q H and the mean themselves and leave the fast route where P needs the
    floor: they flag the 64-matrix blocks holding that bin's matrices and the literal kernel redoes
    them."""
    eps, silent = 1e-3, 5
    B, N, F, T, K = 1, 3, 70, 40, 3
    c = Case(B, N, M, F, T, K, expect={"spatial_form": form, "matrix_blocks": 4},
             flooring=(pr.FLOOR_MAX, eps), state=gr.gen_silent_bin(3 + M, B, N, M, F, T, K, eps, silent))
    moved = c.spatial()                                             # (B,N,F) floored eigenvalues
    assert np.all(moved[:, :, silent] >= M)  # every eigenvalue of P there (about 1e-5), and some more
    flags = c.flags(c.plan["matrix_blocks"])
    idx = (np.arange(N) * F + silent) // 64                         # blocks of (b = 0, n, silent)
    # (a block without a floored eigenvalue may still be flagged: the fast route's test is a
    # sufficient bound; one such block must exist and stay on the fast route)
    floored = np.zeros(4, bool)
    floored[np.unique((np.nonzero(moved.reshape(-1))[0]) // 64)] = True
    assert np.all(flags[idx] == 1)
    assert np.all(floored[idx]) and np.all(flags[floored] == 1)
    assert set(flags.tolist()) == {0, 1}


# ------------------------------------------------------------------------------- partitioning
@pytest.mark.parametrize("F,T", [(9, 40), (40, 9)])
@pytest.mark.parametrize("K", [3, 9])
@pytest.mark.parametrize("N", [3, 9])
@pytest.mark.parametrize("M", [2, 4, 7])
def test_partitioning(M, N, K, F, T):
    """Shared basis and activation with latent variables, both sides of max(F, T) in the expansion;
    NORMALIZE leaves the basis bitwise."""
    c = Case(2, N, M, F, T, K, expect={"latent_lds_bytes": N * K * 8, "wide": int(N > 8)}, part=True)
    c.all_steps()


def test_partitioning_largest_latent():
    """16 sources x 1024 bases: 128 KB of latent LDS, 129 KB of bin LDS."""
    c = Case(1, 16, 2, 2, 3, 1024, expect={"latent_lds_bytes": 128 * 1024,
                                           "bin_lds_bytes": 129 * 1024}, part=True)
    c.all_steps()


# ------------------------------------------------------------------------------- LDS bounds
def _refused(B, N, M, F, T, K):
    """UNSUPPORTED from every entry point, every state array bitwise unchanged."""
    _, dv, _, ops = _mods()
    with pytest.raises(ValueError):
        ops.gmnmf_route(B, N, M, F, T, K)
    X, basis, act, H, _ = gr.gen_state(1, B, N, M, F, T, K)
    h = dict(basis=basis, act=act, H=H)
    o = {k: Out(h[k].shape, k == "H", fill=h[k]) for k in h}
    ws, wsb = ops.gmnmf_workspace(B, N, M, F, T, K, dv.device())
    Xd = up(X)
    with pytest.raises(NotImplementedError):
        ops.gmnmf_update(Xd, o["basis"].t, o["act"].t, o["H"].t, BASIS | ACT | SPATIAL | NORM, MAXF, ws, wsb)
    with pytest.raises(NotImplementedError):
        ops.gmnmf_loss(Xd, o["basis"].t, o["act"].t, o["H"].t, MAXF)
    y = Out((B, N, F, T), True)
    with pytest.raises(NotImplementedError):
        ops.gmnmf_separate(Xd, o["basis"].t, o["act"].t, o["H"].t, 0, MAXF, out=y.t)
    y.get()
    for k in h:
        assert np.array_equal(o[k].get().view(np.float64), np.ascontiguousarray(h[k]).view(np.float64))


def test_lds_bound_above_8_sources():
    """16 sources, 8 channels: the largest n_basis the plan admits runs and meets the bars; one more
    is refused with the state unchanged."""
    ops = _mods()[3]
    K = 1
    while True:
        try:
            ops.gmnmf_route(1, 16, 8, 2, 3, K + 1)
        except ValueError:
            break
        K += 1
    assert 500 < K < 700
    c = Case(1, 16, 8, 2, 3, K, expect={"wide": 1})
    assert c.plan["bin_lds_bytes"] == 16 * 64 * 16 + 16 * K * 8
    c.all_steps()
    _refused(1, 16, 8, 2, 3, K + 1)


@pytest.mark.parametrize("K", [800, 1100])
def test_lds_attribute_up_to_8_sources(K):
    """8 sources, 2 channels: the bin's basis rows take more than 48 KB (K = 800) and more than 64 KB
    (1100) of dynamic LDS: the attribute is raised for these launches too."""
    c = Case(1, 8, 2, 2, 3, K, expect={"wide": 0, "packed": 0})
    assert c.plan["bin_lds_bytes"] > (48 if K == 800 else 64) * 1024
    c.all_steps()


def test_lds_bound_up_to_8_sources():
    """K = 2600 at 8 sources: above the 160 KB of a workgroup, refused before anything is touched."""
    _refused(1, 8, 2, 2, 3, 2600)


# ------------------------------------------------------------------------------- profile
def _write_profile(raw, path):
    worst = {}
    for line in open(raw):
        f = line.rstrip("\n").split("\t")
        key = (f[0], f[1].split(" ")[0])
        if key not in worst or float(f[4]) > float(worst[key][4]):
            worst[key] = f
    with open(path, "w") as out:
        out.write("# largest measured error of every GaussMNMF entry point and route tag, tests/test_gpu_"
                  "gmnmf_pass_elementwise.py on an MI355X\n# entry point, route tag (point kernels / "
                  "spatial form / basis form): worst case; error and bar in units of u = 2^-53 of the "
                  "reference value at the worst element (normwise entries: in units of kappa u); ratio = "
                  "error / bar\n# float64 yardsticks (kappa-normalised error of the NumPy restatement "
                  "against the long-double one, CPU) and the constants 8 x them:\n")
        for k in sorted(gr.C):
            out.write("#   {:10s} yardstick {:6.2f}  c {:7.2f}\n".format(k, gr.MEASURED[k], gr.C[k]))
        for key in sorted(worst):
            f = worst[key]
            out.write("{:24s} {:64s} err {:>10s} u  bar {:>10s} u  ratio {}{}\n".format(
                f[0], f[1], f[2], f[3], f[4], "  " + f[5] if len(f) > 5 else ""))


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles")
    raw = os.path.join(out_dir, "gmnmf_pass_elementwise.raw")
    if os.path.exists(raw):
        os.remove(raw)
    os.environ["SSSPY_PASS_PROFILE_RAW"] = raw
    rc = pytest.main([os.path.abspath(__file__), "-m", "gpu", "-q", "--maxfail=15", "--durations=8"]
                     + sys.argv[2:])
    if os.path.exists(raw):
        _write_profile(raw, os.path.join(out_dir, "gmnmf_pass_elementwise.txt"))
        os.remove(raw)
    sys.exit(int(rc))
