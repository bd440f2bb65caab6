#!/usr/bin/env python3
"""How far the NumPy restatement of ConvIVA (tests/conviva_numpy.py) moves under a 1e-15 relative
perturbation of its input, per test shape (tests/conviva_cases.py) and contrast: the yardstick of the
bars of tests/test_gpu_conviva.py, which allows 1000 x the movement of each shape -- a different
summation order is a perturbation of that size, amplified by cond(R) and by the sweep like this one.
Every shape has to finish with no failed pivot and every movement has to come out <= 1e-11: a shape
above that is ill-determined and has to be replaced by a better-conditioned draw, not loosened.  CPU
only.

    python benchmarks/tools/conviva_sensitivity.py > profiles/conviva_sensitivity.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conviva_cases  # noqa: E402
import conviva_numpy  # noqa: E402

KEYS = ("output", "convolutional_filter", "loss")
DRAWS = 3
# a movement of exactly zero still gets a bar: the rounding of a handful of operations on numbers of
# order one
FLOOR = 1e-15
LIMIT = 1e-11


def perturbed(X, d):
    xi = np.random.default_rng(99 + d).standard_normal(X.shape)
    return X * (1 + 1e-15 * xi)


def movement(case, contrast, n_iter=conviva_cases.N_ITER):
    """max |restatement(X (1 + 1e-15 xi)) - restatement(X)| per quantity (loss: relative), the number
    of failed pivots and the largest cond(R) met."""
    _, taps, delay = case[:3]
    X = conviva_cases.make_mixture(case)
    kwargs = dict(taps=taps, delay=delay, n_iter=n_iter, contrast=contrast)
    base = conviva_numpy.run(X, **kwargs)
    moved = dict.fromkeys(KEYS, FLOOR)
    for d in range(DRAWS):
        other = conviva_numpy.run(perturbed(X, d), **kwargs)
        for key in KEYS[:2]:
            moved[key] = max(moved[key], float(np.abs(other[key] - base[key]).max()))
        rel = np.abs(np.asarray(other["loss"]) / np.asarray(base["loss"]) - 1).max()
        moved["loss"] = max(moved["loss"], float(rel))
    return moved, base["failed"], base["max_cond"]


def main():
    print("# max |restatement(X (1 + 1e-15 xi)) - restatement(X)|, xi ~ N(0, 1) from default_rng(99 + d), "
          "d = 0..{}; n_iter={}, max_flooring(eps=1e-10), diagonal_loading=0, projection back on channel "
          "0; loss: relative; floor {:.0e}".format(DRAWS - 1, conviva_cases.N_ITER, FLOOR))
    print("# bar of tests/test_gpu_conviva.py = 1000 x the movement of the shape and contrast")
    print("{:>24s} {:>9s} {:>7s} {:>10s} {:>10s} {:>21s} {:>10s}   bars".format(
        "case (M,K,D,F,T,B)", "contrast", "failed", "cond(R)", *KEYS))
    for case in conviva_cases.CASES:
        for contrast in conviva_cases.CONTRASTS:
            moved, failed, cond = movement(case, contrast)
            print("{:>24s} {:>9s} {:7d} {:10.2e} {:10.2e} {:21.2e} {:10.2e}   {}".format(
                str(case).replace(" ", ""), contrast, failed, cond, *(moved[k] for k in KEYS),
                "  ".join("{:.1e}".format(1000 * moved[k]) for k in KEYS)), flush=True)
            assert failed == 0, "a pivot failed: replace the draw"
            assert max(moved.values()) <= LIMIT, "ill-determined shape: replace the draw"


if __name__ == "__main__":
    main()
