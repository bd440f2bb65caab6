"""Shared generators of the ConvIVA tests: the shape list and the mixtures (those of the WPE tests).

Every shape was run through the restatement (tests/conviva_numpy.py) on the CPU with both contrasts
and 3 iterations before the list was fixed (benchmarks/tools/conviva_sensitivity.py,
profiles/conviva_sensitivity.txt): none fails a pivot and none moves by more than 1e-11 under a 1e-15
relative perturbation of the input."""

import wpe_cases

# (n_channels, taps, delay, n_bins, n_frames, n_mixtures)
CASES = (
    (2, 1, 1, 2, 24, 1),      # the smallest shape
    (3, 4, 3, 2, 97, 2),      # odd order L = 12, delay > 1, a batch
    (4, 10, 3, 3, 257, 1),    # n_frames is one past a tile of 256
    # Lb = 64, the limit (3 bins: with 2 the Gauss contrast overfits, cond R = 8e6, and the
    # restatement itself moves by 1.5e-11)
    (8, 7, 2, 3, 300, 1),
    (2, 16, 3, 2, 1700, 1),   # 2 * (1700 + 15) * 16 bytes > 48 KiB: the slab is re-read
    (4, 0, 1, 3, 33, 1),      # taps = 0: AuxIVA-IP1
)
SMALL = CASES[:3]
CONTRASTS = ("laplace", "gauss")
N_ITER = 3


def case_id(case):
    return "M{}-K{}-D{}-F{}-T{}-B{}".format(*case)


def make_mixture(case, seed=0):
    """wpe_cases.make_mixture: (M, F, T), or (B, M, F, T) when B > 1."""
    return wpe_cases.make_mixture(case, seed)
