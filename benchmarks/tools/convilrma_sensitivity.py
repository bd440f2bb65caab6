#!/usr/bin/env python3
"""How far the NumPy restatement of ConvILRMA (tests/convilrma_numpy.py) moves under a 1e-15 relative
perturbation of its input, per test shape (tests/convilrma_cases.py): the yardstick of the bars of
tests/test_gpu_convilrma.py, which allows 1000 x the movement of each shape -- a different summation
order is a perturbation of that size, amplified by cond(R), by the sweep and by the NMF updates like
this one.  Every shape has to finish with no failed pivot and every movement has to come out <= 1e-11:
a shape above that is ill-determined (an over-complete NMF on 2-3 bins overfits) and has to be
replaced by the nearest shape with more bins or frames, not loosened.  CPU only.

    python benchmarks/tools/convilrma_sensitivity.py > profiles/convilrma_sensitivity.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import convilrma_cases  # noqa: E402
import convilrma_numpy  # noqa: E402

KEYS = ("output", "convolutional_filter", "basis", "activation", "loss")
DRAWS = 3
# a movement of exactly zero still gets a bar: the rounding of a handful of operations on numbers of
# order one
FLOOR = 1e-15
LIMIT = 1e-11


def perturbed(X, d):
    xi = np.random.default_rng(99 + d).standard_normal(X.shape)
    return X * (1 + 1e-15 * xi)


def movement(case, n_iter=convilrma_cases.N_ITER):
    """max |restatement(X (1 + 1e-15 xi)) - restatement(X)| per quantity (loss: relative; basis and
    activation: relative to the largest entry), the number of failed pivots and the largest cond(R)."""
    _, taps, delay, _, _, _, _, domain = case
    X = convilrma_cases.make_mixture(case)
    basis, activation = convilrma_cases.make_factors(case)
    kwargs = dict(taps=taps, delay=delay, domain=domain, n_iter=n_iter, basis=basis,
                  activation=activation)
    base = convilrma_numpy.run(X, **kwargs)
    moved = dict.fromkeys(KEYS, FLOOR)
    for d in range(DRAWS):
        other = convilrma_numpy.run(perturbed(X, d), **kwargs)
        for key in KEYS[:2]:
            moved[key] = max(moved[key], float(np.abs(other[key] - base[key]).max()))
        for key in KEYS[2:4]:
            moved[key] = max(moved[key], float(np.abs(other[key] - base[key]).max()
                                               / np.abs(base[key]).max()))
        rel = np.abs(np.asarray(other["loss"]) / np.asarray(base["loss"]) - 1).max()
        moved["loss"] = max(moved["loss"], float(rel))
    return moved, base["failed"], base["max_cond"]


def main(cases=convilrma_cases.CASES):
    print("# max |restatement(X (1 + 1e-15 xi)) - restatement(X)|, xi ~ N(0, 1) from default_rng(99 + d), "
          "d = 0..{}; n_iter={}, max_flooring(eps=1e-10), diagonal_loading=0, power normalisation, "
          "projection back on channel 0; loss: relative; basis, activation: relative to the largest "
          "entry; floor {:.0e}".format(DRAWS - 1, convilrma_cases.N_ITER, FLOOR))
    print("# bar of tests/test_gpu_convilrma.py = 1000 x the movement of the shape")
    print("{:>30s} {:>7s} {:>10s} {:>10s} {:>10s} {:>10s} {:>10s} {:>10s}   bars".format(
        "case (M,K,D,F,T,B,Kb,p)", "failed", "cond(R)", "output", "filter", "basis", "activation",
        "loss"))
    ok = True
    for case in cases:
        moved, failed, cond = movement(case)
        print("{:>30s} {:7d} {:10.2e} {:10.2e} {:10.2e} {:10.2e} {:10.2e} {:10.2e}   {}".format(
            str(case).replace(" ", ""), failed, cond, *(moved[k] for k in KEYS),
            "  ".join("{:.1e}".format(1000 * moved[k]) for k in KEYS)), flush=True)
        ok = ok and failed == 0 and max(moved.values()) <= LIMIT
    assert ok, "a pivot failed or a shape is ill-determined: replace the shape"


if __name__ == "__main__":
    main()
