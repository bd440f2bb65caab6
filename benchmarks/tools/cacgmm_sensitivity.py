#!/usr/bin/env python3
"""How far the NumPy restatement of CACGMM (tests/cacgmm_numpy.py) moves under a 1e-15 relative
perturbation of its input, on the test mixtures: the yardstick of the GPU tests' bars
(tests/test_gpu_cacgmm.py uses 1000 x the largest movement per quantity).  CPU only.

    python benchmarks/tools/cacgmm_sensitivity.py > profiles/cacgmm_sensitivity.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cacgmm_numpy as cn  # noqa: E402

COND_LIMIT = 1e6


def main():
    worst = dict(output=0.0, posterior=0.0, mixing=0.0, covariance=0.0, loss=0.0)
    print("# max |restatement(X (1 + 1e-15 xi)) - restatement(X)|, xi ~ N(0, 1) from default_rng(99 + d), "
          "d = 0..2; rng=default_rng(0), n_iter=5")
    print("# covariance: the (source, bin) pairs whose condition number stayed below 1e6 at every "
          "iteration; loss: relative")
    print("{:>18s} {:>9s} {:>10s} {:>10s} {:>10s} {:>10s} {:>10s}".format(
        "case (M,N,F,T)", "excluded", "output", "posterior", "mixing", "covariance", "loss"))
    for case in cn.CASES:
        M, N, F, T = case
        X = cn.make_mixture(*case)
        base = cn.run(X, np.random.default_rng(0), n_sources=N)
        keep = (np.linalg.cond(base["covariance"]) < COND_LIMIT).all(axis=0)
        moved = dict.fromkeys(worst, 0.0)
        for d in range(3):
            xi = np.random.default_rng(99 + d).standard_normal(X.shape)
            other = cn.run(X * (1 + 1e-15 * xi), np.random.default_rng(0), n_sources=N)
            for key in ("output", "posterior"):
                moved[key] = max(moved[key], np.abs(other[key] - base[key]).max())
            moved["mixing"] = max(moved["mixing"], np.abs(other["mixing"] - base["mixing"]).max())
            diff = np.abs(other["covariance"] - base["covariance"]).max(axis=(-2, -1))
            moved["covariance"] = max(moved["covariance"], diff[:, keep].max() if keep.any() else 0.0)
            moved["loss"] = max(moved["loss"],
                                np.abs(other["loss"] / base["loss"] - 1).max())
        print("{:>18s} {:8.1f}% {:10.2e} {:10.2e} {:10.2e} {:10.2e} {:10.2e}".format(
            str(case), 100 * (1 - keep.mean()), *(moved[k] for k in worst)))
        for key in worst:
            worst[key] = max(worst[key], moved[key])
    print("# largest:  " + "  ".join("{} {:.2e}".format(k, v) for k, v in worst.items()))
    print("# bars (x 1000): " + "  ".join("{} {:.1e}".format(k, 1000 * v) for k, v in worst.items()))


if __name__ == "__main__":
    main()
