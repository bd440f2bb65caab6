"""The IPSDTA fixtures (tests/golden/ipsdta_*.npz): their settings, inputs and helpers, shared by the
generator (tests/golden/make_golden_ipsdta.py), the CPU replay and the GPU tests."""

import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VCD_FIXTURE = "ipsdta_vcd_operator"
CUSTOM_EPS = 1e-9


def custom_floor(x):
    """A flooring callable that is none of the reference's three."""
    return np.maximum(x, CUSTOM_EPS) + 1e-12


def _case(cls, shape, n_blocks, n_basis, seed, dof=None, flooring="max", source_normalization=True,
          scale_restoration=True, reference_id=0, inject=False):
    return dict(cls=cls, shape=shape, n_blocks=n_blocks, n_basis=n_basis, seed=seed, dof=dof,
                flooring=flooring, source_normalization=source_normalization,
                scale_restoration=scale_restoration, reference_id=reference_id, inject=inject)


CASES = {
    "ipsdta_gauss_f8_b4": _case("GaussIPSDTA", (2, 8, 20), 4, 2, 601),
    "ipsdta_t3_f8_b4": _case("TIPSDTA", (2, 8, 20), 4, 2, 602, dof=3),
    "ipsdta_gauss_f9_b4_rem1": _case("GaussIPSDTA", (2, 9, 24), 4, 2, 603),
    "ipsdta_t100_f9_b4_rem1": _case("TIPSDTA", (2, 9, 24), 4, 2, 604, dof=100),
    "ipsdta_gauss_f31_b4_rem3": _case("GaussIPSDTA", (2, 31, 20), 4, 2, 605),
    "ipsdta_t3_f31_b4_mdp": _case("TIPSDTA", (2, 31, 20), 4, 2, 606, dof=3,
                                  scale_restoration="minimal_distortion_principle"),
    "ipsdta_gauss_l1": _case("GaussIPSDTA", (3, 6, 20), 6, 2, 607),
    "ipsdta_t100_l1_nonorm": _case("TIPSDTA", (3, 6, 20), 6, 2, 608, dof=100,
                                   source_normalization=False),
    "ipsdta_gauss_b1_l8": _case("GaussIPSDTA", (2, 8, 24), 1, 3, 609),
    "ipsdta_gauss_n8": _case("GaussIPSDTA", (8, 10, 40), 5, 2, 610),
    "ipsdta_t3_k1_ref1": _case("TIPSDTA", (3, 9, 30), 4, 1, 611, dof=3, reference_id=1),
    "ipsdta_gauss_none_norestore": _case("GaussIPSDTA", (3, 17, 40), 5, 3, 612, flooring="none",
                                         scale_restoration=False),
    "ipsdta_t100_add": _case("TIPSDTA", (2, 8, 20), 4, 2, 613, dof=100, flooring="add"),
    "ipsdta_gauss_custom_inject": _case("GaussIPSDTA", (3, 9, 24), 4, 2, 614, flooring="custom",
                                        inject=True),
    "ipsdta_t3_inject": _case("TIPSDTA", (4, 17, 36), 4, 2, 615, dof=3, inject=True),
}


def flooring_for(kind, module):
    """The flooring callable of a case from ``module`` (the reference's or the project's flooring)."""
    if kind == "none":
        return None
    if kind == "max":
        return functools.partial(module.max_flooring, eps=1e-10)
    if kind == "add":
        return functools.partial(module.add_flooring, eps=1e-10)
    return custom_floor


def numpy_floor(kind):
    """(floor on arrays, flooring_fn(0)) for the restatement."""
    if kind == "none":
        return (lambda x: x), 0.0
    if kind == "max":
        return (lambda x: np.maximum(x, 1e-10)), 1e-10
    if kind == "add":
        return (lambda x: x + 1e-10), 1e-10
    return custom_floor, float(custom_floor(0))


def gen_mixture(seed, N, F, T):
    """Laplacian sources with a frame envelope, mixed per bin by a well-conditioned matrix."""
    rng = np.random.default_rng(seed)
    S = (rng.laplace(size=(N, F, T)) + 1j * rng.laplace(size=(N, F, T)))
    S *= (0.3 + rng.random((N, 1, T))) * (0.5 + rng.random((N, F, 1)))
    A = np.eye(N) + 0.4 * (rng.standard_normal((F, N, N)) + 1j * rng.standard_normal((F, N, N)))
    return np.einsum("fnm,mft->nft", A, S)


def initial_state(cfg):
    """The injected demix_filter, basis and activation of a case with ``inject``."""
    N, F, T = cfg["shape"]
    rng = np.random.default_rng(cfg["seed"] + 7)
    W = np.eye(N) + 0.2 * (rng.standard_normal((F, N, N)) + 1j * rng.standard_normal((F, N, N)))
    nb, K = cfg["n_blocks"], cfg["n_basis"]
    L, rem = F // nb, F % nb
    mats = []
    for C, size in ((nb - rem, L), (rem, L + 1)):
        if C:
            G = rng.standard_normal((N, K, C, size, size)) + 1j * rng.standard_normal((N, K, C, size, size))
            mats.append(G @ np.conj(np.swapaxes(G, -2, -1)) / size + 0.1 * np.eye(size))
    basis = tuple(mats) if len(mats) > 1 else mats[0]
    activation = 0.1 + rng.random((N, K, T))
    return dict(demix_filter=W, basis=basis, activation=activation)


def err(a, b):
    """Relative Frobenius distance of a from b."""
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def basis_of(data, prefix):
    """basis (or the (low, high) pair) stored under ``prefix``."""
    if prefix + "_high" in data.files:
        return data[prefix + "_low"], data[prefix + "_high"]
    return data[prefix + "_low"]


class Snapshots:
    """Callback: output and demix_filter after iterations 1 and 2 (call 0 is the initial one)."""

    def __init__(self):
        self.calls, self.store = 0, {}

    def __call__(self, method):
        if self.calls in (1, 2):
            self.store["output_it{}".format(self.calls)] = np.array(
                method.separate(method.input, demix_filter=method.demix_filter))
            self.store["demix_filter_it{}".format(self.calls)] = np.array(method.demix_filter)
        self.calls += 1
