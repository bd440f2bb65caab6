"""Helpers shared by the CPU and GPU tests of the time-domain ICA classes and by the generator of
their golden vectors (tests/golden/make_golden_ica.py): the fixture names, the nonlinearities the
fixtures were made with and the comparison against a fixture."""

import numpy as np

from conftest import rel_err

CASES = [
    "ica_glap_n2",
    "ica_glap_n3_hol",
    "ica_glap_n4_zeros",
    "ica_nglap_n4",
    "ica_nglap_n3_init",
    "ica_nglap_n8_hol",
    "ica_nglap_n16",
    "ica_grad_n3_logistic_hol",
    "ica_ngrad_n4_logcosh",
    "ica_grad_n2_closure",
    "ica_ngrad_n3_closure_hol",
    "ica_fast_n2_logistic",
    "ica_fast_n4_logcosh",
    "ica_fast_n8_logistic",
    "ica_fast_n16_logcosh",
    "ica_fast_n3_closure",
]

SNAP_NAMES = ("it1_demix_filter", "it2_demix_filter", "itlast_demix_filter")


# ---- the nonlinearities of the fixtures, as the textbook NumPy formulas ---------------------------
def logistic_contrast(y):
    return np.log(1 + np.exp(y))


def logistic_score(y):
    return 1 / (1 + np.exp(-y))


def logistic_d_score(y):
    s = 1 / (1 + np.exp(-y))
    return s * (1 - s)


def logcosh_contrast(y):
    return np.log(np.cosh(y))


def logcosh_score(y):
    return np.tanh(y)


def logcosh_d_score(y):
    return 1 - np.tanh(y) ** 2


# an opaque closure per generic class: a smoothed Laplace model and a scaled log-cosh
def smooth_abs_contrast(y, eps=1e-2):
    return np.sqrt(y * y + eps)


def smooth_abs_score(y, eps=1e-2):
    return y / np.sqrt(y * y + eps)


def scaled_logcosh(a=1.5):
    def contrast_fn(y):
        return np.log(np.cosh(a * y)) / a

    def score_fn(y):
        return np.tanh(a * y)

    def d_score_fn(y):
        return a * (1 - np.tanh(a * y) ** 2)

    return contrast_fn, score_fn, d_score_fn


FORMULAS = {
    "logistic": (logistic_contrast, logistic_score, logistic_d_score),
    "logcosh": (logcosh_contrast, logcosh_score, logcosh_d_score),
}


def nonlinearity(name, cls, named=None):
    """Keyword arguments of the callables of a fixture.  ``named``: a module with the named triples
    (ssspy_amd.bss.ica) to take "logistic" / "logcosh" from instead of the formulas above."""
    fast = cls == "FastICA"
    if "Laplace" in cls:
        return {}
    if name == "closure":
        if fast:
            fns = scaled_logcosh()
        elif cls == "GradICA":
            fns = (smooth_abs_contrast, smooth_abs_score, None)
        else:
            fns = (lambda y: smooth_abs_contrast(y), lambda y: smooth_abs_score(y), None)
    elif named is not None:
        fns = named.NAMED[name]
    else:
        fns = FORMULAS[name]
    kwargs = dict(contrast_fn=fns[0], score_fn=fns[1])
    if fast:
        kwargs["d_score_fn"] = fns[2]
    return kwargs


def gen_sources(seed, N, T, zero_run=None):
    """Laplace sources through a mixing matrix I + 0.4 randn, RMS about 0.3; ``zero_run`` = (start,
    stop): those samples of every channel are exactly zero (sign(0))."""
    rng = np.random.default_rng(seed)
    S = rng.laplace(size=(N, T))
    A = np.eye(N) + 0.4 * rng.standard_normal((N, N))
    X = A @ S
    X *= 0.3 / np.sqrt(np.mean(X * X))
    if zero_run is not None:
        X[:, zero_run[0]:zero_run[1]] = 0.0
    return X


class Snapshots:
    """The filters after iterations 1, 2 and the last."""

    def __init__(self, n_iter):
        self.n_iter, self.count, self.store = n_iter, -1, {}

    def __call__(self, method):
        self.count += 1
        W = np.array(method.demix_filter, copy=True)
        if self.count in (1, 2):
            self.store["it{}_demix_filter".format(self.count)] = W
        if self.count == self.n_iter:
            self.store["itlast_demix_filter"] = W


def golden_kwargs(g, named=None):
    cls = str(g["meta_cls"])
    kwargs = nonlinearity(str(g["meta_nonlinearity"]), cls, named)
    if cls != "FastICA":
        kwargs.update(step_size=float(g["meta_step_size"]),
                      is_holonomic=bool(g["meta_is_holonomic"]))
    return kwargs


def golden_init(g):
    return {"demix_filter": g["demix_filter0"].copy()} if "demix_filter0" in g else {}


def check_against_golden(g, m, Y, snap, tol, loss_rtol, report=None):
    """Filters, snapshots and output to ``tol`` relative Frobenius, the loss list to ``loss_rtol``."""
    errs = {"final_demix_filter": rel_err(m.demix_filter, g["final_demix_filter"]),
            "final_output": rel_err(Y, g["final_output"])}
    for name in SNAP_NAMES:
        errs[name] = rel_err(snap.store[name], g[name])
    loss = np.asarray(m.loss, dtype=np.float64)
    errs["loss"] = float(np.max(np.abs(loss - g["loss"]) / np.abs(g["loss"])))
    if report is not None:
        print("{}: {}".format(report, ", ".join("{} {:.1e}".format(k, v) for k, v in errs.items())))
    for name, err in errs.items():
        assert err < (loss_rtol if name == "loss" else tol), (name, err)
    np.testing.assert_allclose(loss, g["loss"], rtol=loss_rtol)
