"""Shared generators of the WPD tests: the shape list, the mixtures (those of the WPE tests), the masks
and random steering vectors."""

import numpy as np

import wpe_cases

# (n_channels, taps, delay, n_sources, n_bins, n_frames, n_mixtures)
CASES = (
    (1, 1, 1, 1, 1, 8, 1),       # the smallest shape
    (2, 3, 1, 2, 3, 40, 1),      # a small two-source case
    (3, 4, 3, 3, 2, 97, 2),      # odd order Lb = 15, delay > 1, a batch
    (4, 10, 3, 2, 3, 257, 1),    # n_frames is one past a tile of 256
    (8, 7, 2, 2, 2, 300, 1),     # Lb = 64, the limit
    (2, 16, 3, 1, 2, 1700, 1),   # 2 * (1700 + 15) * 16 bytes > 48 KiB: the slab is re-read
    (4, 0, 1, 4, 3, 33, 1),      # taps = 0: the variance-weighted MPDR
    (2, 1, 1, 16, 1, 20, 1),     # 16 masks
)
SMALL = CASES[:3]


def case_id(case):
    return "M{}-K{}-D{}-N{}-F{}-T{}-B{}".format(*case)


def make_mixture(case, seed=0):
    """wpe_cases.make_mixture of the same (M, F, T, B): (M, F, T), or (B, M, F, T) when B > 1."""
    M, K, D, _, F, T, B = case
    return wpe_cases.make_mixture((M, K, D, F, T, B), seed)


def make_mask(case, seed=0):
    """uniform(0.05, 1) normalised over the sources: (N, F, T), or (B, N, F, T) when B > 1."""
    M, _, _, N, F, T, B = case
    rng = np.random.default_rng([seed + 1, M, N, F, T, B])
    mask = rng.uniform(0.05, 1.0, (B, N, F, T))
    mask /= mask.sum(axis=1, keepdims=True)
    return mask if B > 1 else mask[0]


def make_steering(case, seed=0):
    """Random steering vectors with entries of modulus in [0.5, 1.5]: (F, N, M), or (B, F, N, M)."""
    M, _, _, N, F, T, B = case
    rng = np.random.default_rng([seed + 2, M, N, F, T, B])
    v = rng.uniform(0.5, 1.5, (B, F, N, M)) * np.exp(2j * np.pi * rng.random((B, F, N, M)))
    return v if B > 1 else v[0]
