"""What the fixture generator (tests/golden/make_golden_pdsbss.py) and the CPU and GPU tests of the
proximal classes share: the list of fixtures and how each was made, the mixtures, the penalties and
user closures, the snapshot callback and the comparison with a fixture."""

import functools

import numpy as np

from conftest import rel_err
from conftest import option as _option

# name -> how the fixture is made.  penalties: names of PENALTIES below, in order.
SPECS = {
    "pdsbss_l21bins_n2": dict(N=2, F=9, T=40, penalties=["l21_bins"]),
    "pdsbss_l21bins_n3": dict(N=3, F=17, T=64, penalties=["l21_bins"]),
    "pdsbss_l21bins_n4_init": dict(N=4, F=17, T=96, penalties=["l21_bins"], inject=True),
    # (seeds 7 and 2: at seed 1 the reference moves by 1.2e-10 / 7.1e-11 under the generator's 1e-15
    # perturbation, over or close to its 1e-10 limit; at these by 3e-14 / 6e-14)
    "pdsbss_l21bins_n8_noscale": dict(N=8, F=9, T=128, seed=7, penalties=["l21_bins"],
                                      scale_restoration=False),
    "pdsbss_l21bins_n10_ref3": dict(N=10, F=7, T=128, seed=2, penalties=["l21_bins"],
                                    reference_id=3),
    "pdsbss_l1_n3": dict(N=3, F=17, T=64, penalties=["l1"], scale_restoration="projection_back"),
    "pdsbss_l21frames_n3_alpha": dict(N=3, F=17, T=64, penalties=["l21_frames"], alpha=1.25),
    "pdsbss_two_n4_mdp_loss": dict(N=4, F=17, T=96, penalties=["l21_bins", "l1"], mu1=0.5,
                                   relaxation=1.5, record_loss=True,
                                   scale_restoration="minimal_distortion_principle"),
    "pdsbss_closure_n3": dict(N=3, F=17, T=64, penalties=["elastic"], record_loss=True),
    # (no loss: the reference's MaskingPDSBSS cannot record one, its compute_loss iterates over the
    # single penalty_fn)
    "pdsbss_masking_n3": dict(N=3, F=17, T=64, cls="MaskingPDSBSS", penalties=["mask"],
                              reference_id=1),
}
CASES = list(SPECS)
DEFAULTS = dict(cls="PDSBSS", seed=1, mu1=1.0, mu2=1.0, relaxation=1.0, alpha=None,
                record_loss=None, scale_restoration=True, reference_id=0, inject=False, n_iter=10)
MASK_THRESHOLD = 0.5


def spec_of(name):
    return dict(DEFAULTS, **SPECS[name])


def laplace_mixture(seed, N, F, T):
    """Laplace sources through a Gaussian mixing matrix per bin, (N, F, T)."""
    rng = np.random.default_rng(seed)
    S = rng.laplace(size=(N, F, T)) + 1j * rng.laplace(size=(N, F, T))
    A = rng.standard_normal((F, N, N)) + 1j * rng.standard_normal((F, N, N))
    return np.einsum("fnm,mft->nft", A, S)


def injected_state(seed, Q, N, F, T):
    """A non-identity demix_filter (F, N, N) and a non-zero dual (Q, N, F, T)."""
    rng = np.random.default_rng(seed + 7)
    W0 = np.eye(N) + 0.2 * (rng.standard_normal((F, N, N)) + 1j * rng.standard_normal((F, N, N)))
    dual0 = 0.05 * (rng.standard_normal((Q, N, F, T)) + 1j * rng.standard_normal((Q, N, F, T)))
    return W0, dual0


# ---- penalties (for the loss) and user closures that are none of the named operators
def penalty_l21_bins(y):
    return np.sum(np.linalg.norm(y, axis=1))


def penalty_l21_frames(y):
    return np.sum(np.linalg.norm(y, axis=2))


def penalty_l21_sources(y):
    return np.sum(np.linalg.norm(y, axis=0))


def penalty_l1(y):
    return np.sum(np.abs(y))


def penalty_elastic(y):
    return np.sum(np.abs(y) + 0.5 * np.abs(y) ** 2)


def prox_elastic(z, step_size=1):
    """prox of |y| + |y|^2 / 2: the l1 shrinkage, then 1 / (1 + step_size)."""
    norm = np.abs(z)
    norm = np.where(norm < step_size, step_size, norm)
    return np.maximum(1 - step_size / norm, 0) * z / (1 + step_size)


def soft_mask(z):
    """A soft-threshold mask on the norm over bins; (n_sources, 1, n_frames), broadcasts."""
    norm = np.linalg.norm(z, axis=1, keepdims=True)
    return np.maximum(1 - MASK_THRESHOLD / np.maximum(norm, 1e-12), 0)


def prox_of(name, prox_ns):
    """The proximal operator of a named penalty from ``prox_ns`` (a namespace with l1 / l21)."""
    if name == "l21_bins":
        return functools.partial(prox_ns.l21, axis2=1)
    if name == "l21_frames":
        return prox_ns.l21  # (the reference's default, axis2=-1)
    if name == "l21_sources":
        return functools.partial(prox_ns.l21, axis2=0)
    if name == "l1":
        return prox_ns.l1
    if name == "elastic":
        return prox_elastic
    raise KeyError(name)


PENALTIES = {"l21_bins": penalty_l21_bins, "l21_frames": penalty_l21_frames, "l1": penalty_l1,
             "l21_sources": penalty_l21_sources,
             "elastic": penalty_elastic, "mask": penalty_l21_bins}


def build_kwargs(spec, prox_ns):
    """Constructor arguments from a spec (or the meta data of a fixture, see ``golden_spec``)."""
    kwargs = dict(mu1=spec["mu1"], mu2=spec["mu2"], scale_restoration=spec["scale_restoration"],
                  record_loss=spec["record_loss"], reference_id=spec["reference_id"])
    if spec["alpha"] is None:
        kwargs["relaxation"] = spec["relaxation"]
    else:
        kwargs["alpha"] = spec["alpha"]
    names = list(spec["penalties"])
    if spec["cls"] == "MaskingPDSBSS":
        kwargs["mask_fn"] = soft_mask
        if spec["record_loss"]:
            kwargs["penalty_fn"] = PENALTIES[names[0]]
        return kwargs
    kwargs["prox_penalty"] = [prox_of(n, prox_ns) for n in names]
    if len(names) == 1:
        kwargs["prox_penalty"] = kwargs["prox_penalty"][0]
    if spec["record_loss"]:
        kwargs["penalty_fn"] = [PENALTIES[n] for n in names]
    return kwargs


def golden_spec(g):
    """The spec a fixture was made with, from its meta data."""
    alpha = float(g["meta_alpha"])
    record = int(g["meta_record_loss"])
    return dict(cls=str(g["meta_cls"]), seed=int(g["meta_seed"]), mu1=float(g["meta_mu1"]),
                mu2=float(g["meta_mu2"]), relaxation=float(g["meta_relaxation"]),
                alpha=None if np.isnan(alpha) else alpha,
                record_loss=None if record < 0 else bool(record),
                scale_restoration=_option(g["meta_scale_restoration"]),
                reference_id=int(g["meta_reference_id"]), inject="demix_filter0" in g,
                n_iter=int(g["meta_n_iter"]), penalties=[str(p) for p in g["meta_penalties"]],
                N=int(g["meta_shape"][0]), F=int(g["meta_shape"][1]), T=int(g["meta_shape"][2]))


def golden_init(g):
    if "demix_filter0" not in g:
        return {}
    return {"demix_filter": g["demix_filter0"], "dual": g["dual0"]}


class Snapshots:
    """demix_filter and dual after every iteration (count 0: the initial call)."""

    names = ("demix_filter", "dual")

    def __init__(self):
        self.count, self.store = -1, {}

    def __call__(self, method):
        self.count += 1
        for name in self.names:
            self.store["it{}_{}".format(self.count, name)] = np.array(getattr(method, name),
                                                                      copy=True)


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
    assert checked == 6
    if g["loss"].size:
        np.testing.assert_allclose(np.array(m.loss), g["loss"], rtol=loss_rtol)
    else:
        assert m.loss is None
    errs = (rel_err(np.asarray(m.demix_filter), g["final_demix_filter"]),
            rel_err(Y, g["final_output"]))
    if show:
        print(show, "final", errs)
    assert max(errs) < tol
