#!/usr/bin/env python3
"""How far the NumPy restatement of OverIVA (tests/overiva_numpy.py) moves under a 1e-15 relative
perturbation of its input, on the test mixtures: the yardstick of the GPU tests' bars
(tests/test_gpu_overiva.py uses 1000 x the largest movement per quantity, capped at 1e-6 and at 1e-5
relative for the loss).  CPU only.

    python benchmarks/tools/overiva_sensitivity.py > profiles/overiva_sensitivity.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import overiva_numpy as on  # noqa: E402

KEYS = ("output", "demix_filter", "background_filter", "loss")
CONFIGS = (on.LAPLACE_MAX, on.GAUSS_ADD)


def main():
    worst = dict.fromkeys(KEYS, 0.0)
    print("# max |restatement(X (1 + 1e-15 xi)) - restatement(X)|, xi ~ N(0, 1) from default_rng(99 + d), "
          "d = 0..2; n_iter=5, projection back; loss: relative")
    print("# compared: the run is one of overiva_numpy.RUNS, the end-to-end comparisons of the GPU test; "
          "only those enter the bars")
    print("{:>18s} {:>8s} {:>8s} {:>10s} {:>12s} {:>17s} {:>10s}".format(
        "case (M,N,F,T)", "contrast", "compared", *KEYS))
    for case in on.CASES:
        M, N, F, T = case
        X = on.make_mixture(*case)
        for contrast, flooring in CONFIGS:
            base = on.run(X, n_sources=N, contrast=contrast, flooring=flooring)
            moved = dict.fromkeys(KEYS, 0.0)
            for d in range(3):
                xi = np.random.default_rng(99 + d).standard_normal(X.shape)
                other = on.run(X * (1 + 1e-15 * xi), n_sources=N, contrast=contrast, flooring=flooring)
                for key in KEYS[:3]:
                    moved[key] = max(moved[key], np.abs(other[key] - base[key]).max())
                moved["loss"] = max(moved["loss"], np.abs(other["loss"] / base["loss"] - 1).max())
            used = (case, (contrast, flooring)) in on.RUNS
            print("{:>18s} {:>8s} {:>8s} {:10.2e} {:12.2e} {:17.2e} {:10.2e}".format(
                str(case), contrast, "yes" if used else "no", *(moved[k] for k in KEYS)))
            for key in KEYS:
                if used:
                    worst[key] = max(worst[key], moved[key])
    print("# largest of the compared runs:  " + "  ".join("{} {:.2e}".format(k, v) for k, v in worst.items()))
    print("# bars (x 1000, capped at 1e-6; loss 1e-5): " + "  ".join(
        "{} {:.1e}".format(k, min(1000 * v, 1e-5 if k == "loss" else 1e-6)) for k, v in worst.items()))


if __name__ == "__main__":
    main()
