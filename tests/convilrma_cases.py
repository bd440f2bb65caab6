"""Shared generators of the ConvILRMA tests: the shape list, the mixtures (those of the WPE tests) and
the seeded NMF factors.

Every shape was run through the restatement (tests/convilrma_numpy.py) on the CPU with 3 iterations
before the list was fixed (benchmarks/tools/convilrma_sensitivity.py,
profiles/convilrma_sensitivity.txt): a shape is kept only if the restatement fails no pivot and moves
by at most 1e-11 under a 1e-15 relative perturbation of the input."""

import numpy as np

import convilrma_numpy
import wpe_cases

# (n_channels, taps, delay, n_bins, n_frames, n_mixtures, n_basis, domain)
CASES = (
    (2, 1, 1, 2, 24, 1, 1, 2),      # the smallest shape, one basis
    (3, 4, 3, 2, 97, 2, 3, 2),      # odd order L = 12, delay > 1, a batch
    (4, 10, 3, 3, 257, 1, 4, 1),    # n_frames is one past a tile of 256; the pow path
    (8, 7, 2, 3, 300, 1, 2, 2),     # Lb = 64, the limit
    (2, 16, 3, 2, 1700, 1, 2, 2),   # 2 * (1700 + 15) * 16 bytes > 48 KiB: the slab is re-read
    (4, 0, 1, 3, 33, 1, 32, 2),     # taps = 0: GaussILRMA-IP1; n_basis = 32, the limit
)
SMALL = CASES[:3]
N_ITER = 3


def case_id(case):
    return "M{}-K{}-D{}-F{}-T{}-B{}-Kb{}-p{}".format(*case)


def make_mixture(case, seed=0):
    """wpe_cases.make_mixture: (M, F, T), or (B, M, F, T) when B > 1."""
    return wpe_cases.make_mixture(case[:6], seed)


def make_factors(case, seed=0):
    """(basis, activation) of a case: max_flooring(eps=1e-10) of uniform draws, basis first, as the
    class draws them from ``rng=numpy.random.default_rng([seed + 7, *case])``."""
    M, _, _, F, T, B, Kb, _ = case
    rng = np.random.default_rng([seed + 7] + list(case))
    shape = (B, M, F, T) if B > 1 else (M, F, T)
    return convilrma_numpy.make_factors(shape, Kb, rng)
