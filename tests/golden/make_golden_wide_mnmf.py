#!/usr/bin/env python3
"""Golden vectors of FastGaussMNMF at 9-16 channels and above 8 sources.

Runs ONLY where the reference checkout is available, as make_golden.py does (whose ``run_mnmf``
and ``run_custom_floor`` it reuses unchanged):

    python tests/golden/make_golden_wide_mnmf.py

Writes seven ``tests/golden/*.npz`` fixtures; re-running it reproduces them byte for byte.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import run_custom_floor, run_mnmf  # noqa: E402


def main():
    run_mnmf("fmnmf_ip1_m10", M=10, F=7, T=40, K=2, seed=200)
    run_mnmf("fmnmf_ip1_m16_n3", M=16, F=6, T=64, K=3, seed=201, n_sources=3)
    run_mnmf("fmnmf_ip2_m12", M=12, F=6, T=48, K=2, seed=202, diag_algo="IP2")
    run_mnmf("fmnmf_ip2_m16_comb", M=16, F=5, T=64, K=2, seed=205, diag_algo="IP2",
             pairs="combination")
    run_mnmf("fmnmf_ip1_m4_n12", M=4, F=6, T=40, K=2, seed=203, n_sources=12)
    run_mnmf("fmnmf_ip1_m9_nonorm_add", M=9, F=7, T=36, K=3, seed=204, normalization=False,
             flooring=("add", 1e-6))
    run_custom_floor("customfloor_fmnmf_m10", kind="fmnmf", seed=206, N=10, F=6, T=40)


if __name__ == "__main__":
    main()
