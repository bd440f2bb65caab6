"""What the FastIVA / FasterIVA tests share: the fixture list, the closures, the snapshot callback
and the comparisons that respect the phase gauge of the whitening (tests/fast_iva_numpy.py).

``demix_filter`` and ``whitened_input`` are defined up to a diagonal unitary D per bin, so they are
never compared elementwise: filters are compared through their action W P on the unwhitened input
(P the whitening filter, recovered from ``whitened_input`` and ``input``), up to one phase per row.
"""

import functools

import numpy as np

from oracle import spatial as sp

SNAP_ITERS = (1, 2)
SMOOTH = 0.1


def laplace_closures():
    """G = 2 r, G' = 2, G'' = 0."""
    def contrast_fn(y):
        return 2 * np.linalg.norm(y, axis=1)

    def d_contrast_fn(r):
        return 2 * np.ones_like(r)

    def dd_contrast_fn(r):
        return np.zeros_like(r)

    return dict(contrast_fn=contrast_fn, d_contrast_fn=d_contrast_fn, dd_contrast_fn=dd_contrast_fn)


def smooth_closures():
    """G = 2 sqrt(r^2 + 0.1): G'' != 0."""
    def contrast_fn(y):
        return 2 * np.sqrt(np.sum(np.abs(y) ** 2, axis=1) + SMOOTH)

    def d_contrast_fn(r):
        return 2 * r / np.sqrt(r ** 2 + SMOOTH)

    def dd_contrast_fn(r):
        return 2 * SMOOTH / (r ** 2 + SMOOTH) ** 1.5

    return dict(contrast_fn=contrast_fn, d_contrast_fn=d_contrast_fn, dd_contrast_fn=dd_contrast_fn)


CLOSURES = {"laplace": laplace_closures, "smooth": smooth_closures}


def closures_for(cls, contrast):
    kw = CLOSURES[contrast]()
    if cls == "FasterIVA":
        kw.pop("dd_contrast_fn")
    return kw


def custom_floor(x):
    """A flooring callable that is none of the reference's three."""
    return np.maximum(x, 1e-8) + 1e-12


def flooring_for(spec, module):
    """``module`` supplies max_flooring / add_flooring (the reference's, the product's or the
    restatement's: the product recognises them by name)."""
    kind, eps = spec
    if kind == "max":
        return functools.partial(module.max_flooring, eps=eps)
    if kind == "add":
        return functools.partial(module.add_flooring, eps=eps)
    if kind == "custom":
        return custom_floor
    return None


# name -> settings.  Shapes: the table of the issue; n_iter is the generator's upper bound, lowered
# per fixture until the reference's own movement under a 2^-50 perturbation is at most 1e-10.
# (the max floor of 3.0 / 5.0 acts on 2 r for some frames and not for others: the whitened frame
#  norms of these mixtures lie on both sides of it)
CASES = {
    "fastiva_n2": dict(cls="FastIVA", shape=(2, 5, 17), seed=500),
    "fastiva_n3_smooth_add": dict(cls="FastIVA", shape=(3, 7, 33), seed=501, contrast="smooth",
                                  flooring=("add", 1e-3), scale_restoration=False),
    "fastiva_n4_init_pb": dict(cls="FastIVA", shape=(4, 17, 70), seed=502, init_filter=True,
                               scale_restoration="projection_back", reference_id=1),
    "fastiva_n8_mdp": dict(cls="FastIVA", shape=(8, 9, 40), seed=503,
                           scale_restoration="minimal_distortion_principle", reference_id=2),
    "fastiva_n9_maxfloor": dict(cls="FastIVA", shape=(9, 3, 48), seed=504, flooring=("max", 3.0)),
    "fastiva_n16_none": dict(cls="FastIVA", shape=(16, 2, 80), seed=505, flooring=("none", 0.0),
                             contrast="smooth"),
    "fastiva_n3_custom": dict(cls="FastIVA", shape=(3, 7, 33), seed=506, flooring=("custom", 0.0)),
    "fasteriva_n2": dict(cls="FasterIVA", shape=(2, 5, 17), seed=510),
    "fasteriva_n3_smooth_maxfloor": dict(cls="FasterIVA", shape=(3, 7, 33), seed=511,
                                         contrast="smooth", flooring=("max", 5.0),
                                         scale_restoration=False),
    "fasteriva_n4_init_mdp": dict(cls="FasterIVA", shape=(4, 17, 70), seed=512, init_filter=True,
                                  scale_restoration="minimal_distortion_principle"),
    "fasteriva_n8_add": dict(cls="FasterIVA", shape=(8, 9, 40), seed=513, flooring=("add", 1e-3),
                             reference_id=5),
    "fasteriva_n9_custom": dict(cls="FasterIVA", shape=(9, 3, 48), seed=514,
                                flooring=("custom", 0.0)),
    "fasteriva_n16": dict(cls="FasterIVA", shape=(16, 2, 80), seed=515, scale_restoration=False),
    "fasteriva_n4_none": dict(cls="FasterIVA", shape=(4, 17, 70), seed=516, flooring=("none", 0.0)),
}
DEFAULTS = dict(contrast="laplace", flooring=("max", 1e-10), scale_restoration=True, reference_id=0,
                init_filter=False)
TRANSFORM_FIXTURE = "fastiva_transforms"


def settings(name):
    return dict(DEFAULTS, **CASES[name])


def gen_mixture(seed, N, F, T):
    """Sources with a heavy-tailed envelope per frame, mixed per bin."""
    rng = np.random.default_rng(seed)
    env = rng.gamma(0.6, size=(N, 1, T)) + 0.05
    S = env * (rng.standard_normal((N, F, T)) + 1j * rng.standard_normal((N, F, T)))
    A = rng.standard_normal((F, N, N)) + 1j * rng.standard_normal((F, N, N))
    return sp.separate(S, A)


def initial_filter(seed, N, F):
    """A unitary start that is not the identity (the filters act on the whitened mixture)."""
    rng = np.random.default_rng(seed + 7)
    A = rng.standard_normal((F, N, N)) + 1j * rng.standard_normal((F, N, N))
    return np.linalg.qr(A)[0]


def regauge_filter(W, D):
    """W D^H: the filter that does to D Z what W does to Z.  D (n_bins, n_channels)."""
    return W * D.conj()[:, np.newaxis, :]


def filter_action(method, X=None):
    """W P (n_bins, n_sources, n_channels): what the filters do to the unwhitened input."""
    X = np.asarray(method.input if X is None else X)
    Z = np.asarray(method.whitened_input)
    return np.asarray(method.demix_filter) @ sp.demix_from_output(Z, X)


class ActionSnapshots:
    """Callback that keeps W P after the iterations of SNAP_ITERS (and counts the calls)."""

    def __init__(self):
        self.count = -1  # the initial call happens before the first iteration
        self.store = {}

    def __call__(self, method):
        self.count += 1
        if self.count in SNAP_ITERS:
            self.store["it{}_action".format(self.count)] = filter_action(method)


def err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def err_up_to_row_phase(a, b):
    """Relative Frobenius error after removing one unit factor per row of the last axis, taken from
    the inner product with the expected row: (F, N, N) filters row by row, (N, F, T) outputs per
    (source, bin)."""
    a, b = np.asarray(a), np.asarray(b)
    inner = np.sum(b * a.conj(), axis=-1, keepdims=True)
    mag = np.abs(inner)
    phase = np.where(mag > 0, inner / np.where(mag > 0, mag, 1), 1)
    return err(a * phase, b)
