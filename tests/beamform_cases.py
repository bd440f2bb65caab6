"""Shared generators of the beamformer tests: masked test mixtures and the shape list."""

import numpy as np

# (n_channels, n_sources, n_bins, n_frames, n_mixtures)
CASES = (
    (1, 1, 1, 5, 1),       # the smallest shape
    (2, 1, 1, 7, 1),       # two channels, one source
    (3, 2, 3, 97, 2),      # odd n_channels, a batch
    (4, 3, 3, 257, 1),     # n_frames is one past a tile of 256
    (5, 1, 2, 64, 1),      # with an explicit (n_bins, n_frames) noise mask shared by the sources
    (8, 16, 2, 300, 1),    # both limits: 2 * 16 * 36 = 1152 sums over 256 threads
    (2, 2, 2, 1700, 1),    # 2 * 1700 * 16 bytes > 48 KiB: the slab is re-read, not resident
)
SHARED_NOISE_CASE = CASES[4]
STREAMING_CASE = CASES[6]
ELEMENTWISE = CASES[:4] + (CASES[5],)
NOISE_LEVEL = 0.1
ACTIVITY = 0.5

# (name, kind of the restatement, keyword arguments of the restatement, class name, class keywords)
BEAMFORMERS = (
    ("mvdr", "mvdr", {"loading": 1e-6}, "MVDR", {}),
    ("gev-reference", "gev", {"loading": 1e-6, "normalization": "reference"}, "GEV", {}),
    ("gev-ban", "gev", {"loading": 1e-6, "normalization": "ban"}, "GEV", {"normalization": "ban"}),
    ("mwf", "mwf", {"loading": 0.0, "mu": 1.0}, "MWF", {}),
)


def case_id(case):
    return "M{}-N{}-F{}-T{}-B{}".format(*case)


def make_case(case, seed=0):
    """x_t = sum_n h_n s_nt + 0.1 noise per bin, with random steering vectors h_n and sources of RMS 1
    that are active in half of the frames; the masks are the ideal ratio masks
    |h_n|^2 |s_nt|^2 / (sum_n' |h_n'|^2 |s_n't|^2 + noise power), so the top generalised eigenvalue
    of every source is well separated.  Returns (X, mask, noise_mask): (M, F, T), (N, F, T) -- with a
    leading mixture axis when B > 1 -- and noise_mask None except for SHARED_NOISE_CASE, where it is
    the (F, T) ratio of the noise power."""
    M, N, F, T, B = case
    rng = np.random.default_rng([seed, M, N, F, T, B])

    def cnormal(shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)

    h = cnormal((B, F, N, M))
    active = rng.random((B, N, F, T)) < ACTIVITY
    s = cnormal((B, N, F, T)) * active
    s /= np.sqrt(np.maximum(np.mean(np.abs(s) ** 2, axis=-1, keepdims=True), 1e-30))
    X = np.einsum("bfnm,bnft->bmft", h, s) + NOISE_LEVEL * cnormal((B, M, F, T))
    power = np.sum(np.abs(h) ** 2, axis=-1).transpose(0, 2, 1)[..., None] * np.abs(s) ** 2
    noise_power = M * NOISE_LEVEL ** 2
    total = power.sum(axis=1, keepdims=True) + noise_power
    mask = power / total
    noise_mask = noise_power / total[:, 0] if case == SHARED_NOISE_CASE else None
    if B == 1:
        X, mask = X[0], mask[0]
        noise_mask = None if noise_mask is None else noise_mask[0]
    return X, mask, noise_mask
