#!/usr/bin/env python3
"""Golden vectors of GaussMNMF at 9-16 sources (2-8 channels).

Runs ONLY where the reference checkout is available, as make_golden.py does (whose ``run_gmnmf``
it reuses unchanged):

    python tests/golden/make_golden_gmnmf_sources.py

Writes six ``tests/golden/*.npz`` fixtures; re-running it reproduces them byte for byte.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import gen_mixture, run_gmnmf  # noqa: E402


def main():
    run_gmnmf("gmnmf_m2_n9", M=2, F=8, T=24, K=2, seed=300, n_sources=9, spatial_init=True)
    run_gmnmf("gmnmf_m4_n12", M=4, F=6, T=30, K=3, seed=301, n_sources=12, gen=gen_mixture)
    run_gmnmf("gmnmf_m8_n16", M=8, F=4, T=32, K=2, seed=302, n_sources=16, gen=gen_mixture,
              n_iter=4)
    run_gmnmf("gmnmf_part_m3_n10", M=3, F=8, T=24, K=12, seed=303, n_sources=10,
              gen=gen_mixture, spatial_init=True, partitioning=True)
    run_gmnmf("gmnmf_m6_n16_nonorm_add", M=6, F=4, T=24, K=2, seed=304, n_sources=16,
              normalization=False, flooring=("add", 1e-6), n_iter=6)
    # (the eigenvalue floor of to_psd active at most points, as gmnmf_floor_m5)
    run_gmnmf("gmnmf_floor_m5_n9", M=5, F=6, T=24, K=3, seed=305, n_sources=9, gen=gen_mixture,
              spatial_init=True, flooring=("max", 0.3), n_iter=10)


if __name__ == "__main__":
    main()
