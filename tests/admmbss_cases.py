"""What the fixture generator (tests/golden/make_golden_admmbss.py) and the CPU and GPU tests of
ADMMBSS / MaskingADMMBSS / ADMMIVA / PDSIVA share: the list of fixtures and how each was made, the
mixtures (scaled to RMS 0.1: at RMS 1 the reference's own ADMM iteration diverges), the penalties and
user closures, the snapshot callback and the comparison with a fixture."""

import numpy as np

import pdsbss_cases as pc
from conftest import rel_err
from conftest import option as _option

RMS = 0.1
MASK_C = 0.01

# name -> how the fixture is made.  penalties: names of pdsbss_cases.PENALTIES, in order.
SPECS = {
    "admmbss_l1_n3": dict(N=3, F=17, T=50, penalties=["l1"], scale_restoration="projection_back"),
    "admmbss_l21bins_n2": dict(N=2, F=9, T=40, penalties=["l21_bins"]),
    "admmbss_l21bins_n3": dict(N=3, F=17, T=50, penalties=["l21_bins"]),
    "admmbss_l21bins_n4": dict(N=4, F=33, T=64, penalties=["l21_bins"], reference_id=2),
    "admmbss_l21bins_n8_noscale": dict(N=8, F=9, T=64, penalties=["l21_bins"],
                                       scale_restoration=False),
    "admmbss_l21bins_n10": dict(N=10, F=7, T=64, penalties=["l21_bins"]),
    "admmbss_l21frames_n3_alpha": dict(N=3, F=17, T=50, penalties=["l21_frames"], alpha=1.25),
    "admmbss_l21sources_n3": dict(N=3, F=17, T=50, penalties=["l21_sources"]),
    "admmbss_two_n4_mdp_loss": dict(N=4, F=17, T=64, penalties=["l21_bins", "l1"], record_loss=True,
                                    scale_restoration="minimal_distortion_principle"),
    "admmbss_l21bins_n3_relax": dict(N=3, F=17, T=50, penalties=["l21_bins"], relaxation=1.5,
                                     rho=0.5, record_loss=True),
    "admmbss_l21bins_n4_init": dict(N=4, F=17, T=64, penalties=["l21_bins"], inject=True,
                                    relaxation=1.5),
    "admmbss_closure_n3": dict(N=3, F=17, T=50, penalties=["elastic"], record_loss=True),
    # (no loss: the reference's MaskingADMMBSS cannot record one, its compute_loss iterates over the
    # single penalty_fn)
    "admmbss_masking_n3": dict(N=3, F=17, T=50, cls="MaskingADMMBSS", penalties=["mask"],
                               record_loss=None, reference_id=1),
    "admmiva_default_n3": dict(N=3, F=17, T=50, cls="ADMMIVA", penalties=[], record_loss=True),
    "admmiva_user_n3": dict(N=3, F=17, T=50, cls="ADMMIVA", penalties=[], record_loss=True,
                            user=True, rho=2.0),
    "pdsiva_default_n3": dict(N=3, F=17, T=50, cls="PDSIVA", penalties=[], record_loss=True),
    "pdsiva_user_n3": dict(N=3, F=17, T=50, cls="PDSIVA", penalties=[], record_loss=True, user=True),
    "admmbss_l21bins_n3_batch": dict(N=3, F=9, T=40, B=3, penalties=["l21_bins"], record_loss=True,
                                     relaxation=1.25),
}
CASES = list(SPECS)
DEFAULTS = dict(cls="ADMMBSS", seed=1, B=1, rho=1.0, relaxation=1.0, alpha=None, record_loss=False,
                scale_restoration=True, reference_id=0, inject=False, user=False, n_iter=10)
ADMM_STATES = ("auxiliary1", "dual1", "auxiliary2", "dual2")


def spec_of(name):
    return dict(DEFAULTS, **SPECS[name])


def state_names(cls):
    return ("dual",) if cls == "PDSIVA" else ADMM_STATES


def mixture(seed, N, F, T):
    """pdsbss_cases.laplace_mixture scaled to RMS 0.1, (N, F, T)."""
    X = pc.laplace_mixture(seed, N, F, T)
    return X * (RMS / np.sqrt(np.mean(np.abs(X) ** 2)))


def mixtures(spec):
    """The input of a spec: (N, F, T), or (B, N, F, T) for a batched one (seed + 20 b)."""
    N, F, T = spec["N"], spec["F"], spec["T"]
    if spec["B"] == 1:
        return mixture(spec["seed"], N, F, T)
    return np.stack([mixture(spec["seed"] + 20 * b, N, F, T) for b in range(spec["B"])])


def injected_state(seed, Q, N, F, T):
    """A non-identity demix_filter and non-zero auxiliary / dual variables."""
    rng = np.random.default_rng(seed + 7)

    def noise(*shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)

    return {"demix_filter": np.eye(N) + 0.2 * noise(F, N, N),
            "auxiliary1": np.eye(N) + 0.2 * noise(F, N, N), "dual1": 0.05 * noise(F, N, N),
            "auxiliary2": 0.05 * noise(Q, N, F, T), "dual2": 0.05 * noise(Q, N, F, T)}


# ---- user closures
def smooth_mask(z):
    """|z|^2 / (|z|^2 + c): smooth in z, no flooring kink."""
    p = np.abs(z) ** 2
    return p / (p + MASK_C)


def user_contrast(y):
    """Twice the norm over bins, (n_sources, n_frames)."""
    return 2 * np.linalg.norm(y, axis=1)


def user_prox(z, step_size=1):
    """The proximal operator of user_contrast, written out (no named operator: the host runs it)."""
    norm = np.sqrt(np.sum(np.abs(z) ** 2, axis=1, keepdims=True))
    norm = np.where(norm < 2 * step_size, 2 * step_size, norm)
    return np.maximum(1 - 2 * step_size / norm, 0) * z


def build_kwargs(spec, prox_ns):
    """Constructor arguments from a spec (or the meta data of a fixture, see ``golden_spec``)."""
    kwargs = dict(scale_restoration=spec["scale_restoration"], record_loss=spec["record_loss"],
                  reference_id=spec["reference_id"])
    if spec["cls"] != "PDSIVA":
        kwargs["rho"] = spec["rho"]
    if spec["alpha"] is None:
        kwargs["relaxation"] = spec["relaxation"]
    else:
        kwargs["alpha"] = spec["alpha"]
    names = list(spec["penalties"])
    if spec["cls"] in ("ADMMIVA", "PDSIVA"):
        if spec["user"]:
            kwargs.update(contrast_fn=user_contrast, prox_penalty=user_prox)
        return kwargs
    if spec["cls"] == "MaskingADMMBSS":
        kwargs["mask_fn"] = smooth_mask
        if spec["record_loss"]:
            kwargs["penalty_fn"] = pc.PENALTIES[names[0]]
        return kwargs
    kwargs["prox_penalty"] = [pc.prox_of(n, prox_ns) for n in names]
    if len(names) == 1:
        kwargs["prox_penalty"] = kwargs["prox_penalty"][0]
    if spec["record_loss"]:
        kwargs["penalty_fn"] = [pc.PENALTIES[n] for n in names]
    return kwargs


def golden_spec(g):
    """The spec a fixture was made with, from its meta data."""
    alpha = float(g["meta_alpha"])
    record = int(g["meta_record_loss"])
    shape = [int(v) for v in g["meta_shape"]]
    return dict(cls=str(g["meta_cls"]), seed=int(g["meta_seed"]), B=int(g["meta_B"]),
                rho=float(g["meta_rho"]), relaxation=float(g["meta_relaxation"]),
                alpha=None if np.isnan(alpha) else alpha,
                record_loss=None if record < 0 else bool(record),
                scale_restoration=_option(g["meta_scale_restoration"]),
                reference_id=int(g["meta_reference_id"]), inject="auxiliary10" in g,
                user=bool(g["meta_user"]), n_iter=int(g["meta_n_iter"]),
                penalties=[str(p) for p in g["meta_penalties"]], N=shape[0], F=shape[1], T=shape[2])


def golden_init(g):
    if "auxiliary10" not in g:
        return {}
    return {name: g[name + "0"] for name in ("demix_filter",) + ADMM_STATES}


class Snapshots:
    """demix_filter and the states of the class after every iteration (count 0: the initial call)."""

    def __init__(self, cls):
        self.names = ("demix_filter",) + state_names(cls)
        self.count, self.store = -1, {}

    def __call__(self, method):
        self.count += 1
        for name in self.names:
            self.store["it{}_{}".format(self.count, name)] = np.array(getattr(method, name),
                                                                      copy=True)


def check_loss(got, want, loss_rtol):
    """Finite entries to ``loss_rtol``; non-finite ones (the first iteration from the zero state,
    where W = 0) by position and sign."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite)
    assert np.array_equal(got[~finite], want[~finite]) and not np.isnan(got).any()
    np.testing.assert_allclose(got[finite], want[finite], rtol=loss_rtol)


def check_against_golden(g, m, Y, snap, tol, loss_rtol, show=None):
    """The snapshots the fixture holds, the loss list, the final filters and the output."""
    checked = 0
    for key in sorted(g):
        if key.startswith("it"):
            err = rel_err(snap.store[key], g[key])
            if show:
                print(show, key, err)
            assert err < tol, key
            checked += 1
    assert checked == 3 * len(snap.names)
    if g["loss"].size:
        check_loss(np.array(m.loss), g["loss"], loss_rtol)
    else:
        assert m.loss is None
    errs = (rel_err(np.asarray(m.demix_filter), g["final_demix_filter"]),
            rel_err(Y, g["final_output"]))
    if show:
        print(show, "final", errs)
    assert max(errs) < tol
