#!/usr/bin/env python3
"""How far the NumPy restatement of WPD (tests/wpd_numpy.py) moves under a 1e-15 relative
perturbation of its input, per test shape (tests/wpd_cases.py) and form (mask, steering): the
yardstick of the bars of tests/test_gpu_wpd.py, which allows 1000 x the movement of each shape -- a
different summation order is a perturbation of that size, amplified by cond(R) like this one.  Every
output bar has to come out <= 1e-7: a shape above that is ill-determined and has to be replaced by a
better-conditioned draw, not loosened.  CPU only.

    python benchmarks/tools/wpd_sensitivity.py > profiles/wpd_sensitivity.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import wpd_cases  # noqa: E402
import wpd_numpy  # noqa: E402

KEYS = ("output", "convolutional_filter", "loss")
N_ITER = 3
DRAWS = 3
# a movement of exactly zero still gets a bar: the rounding of a handful of operations on numbers of
# order one
FLOOR = 1e-15


def perturbed(X, d):
    xi = np.random.default_rng(99 + d).standard_normal(X.shape)
    return X * (1 + 1e-15 * xi)


def movement(case, steering, n_iter=N_ITER):
    """max |restatement(X (1 + 1e-15 xi)) - restatement(X)| per quantity (loss: relative), and the
    largest cond(R) of the last iteration."""
    _, taps, delay = case[:3]
    X = wpd_cases.make_mixture(case)
    kwargs = dict(taps=taps, delay=delay, n_iter=n_iter)
    if steering:
        kwargs["steering_vector"] = wpd_cases.make_steering(case)
    else:
        kwargs["mask"] = wpd_cases.make_mask(case)
    base = wpd_numpy.run(X, statistics=True, **kwargs)
    moved = dict.fromkeys(KEYS, FLOOR)
    for d in range(DRAWS):
        other = wpd_numpy.run(perturbed(X, d), **kwargs)
        for key in KEYS[:2]:
            moved[key] = max(moved[key], float(np.abs(other[key] - base[key]).max()))
        rel = np.abs(np.asarray(other["loss"]) / np.asarray(base["loss"]) - 1).max()
        moved["loss"] = max(moved["loss"], float(rel))
    R = base["R"].reshape(-1, *base["R"].shape[-2:])
    return moved, max(float(np.linalg.cond(r)) for r in R)


COMPOSITION_CASE = (3, 3, 1, 2, 5, 64, 1)


def composition():
    """The same movement for the composition test: WPD(taps=3, delay=1), 3 iterations, on (3 channels,
    5 bins, 64 frames) with two masks held fixed (the test feeds the posterior of its device run of
    CACGMM to both sides).  The masks here stand in for that posterior: the draw of wpd_cases and a
    sharp random soft assignment, the larger movement of the two."""
    M, taps, delay, N, F, T, _ = COMPOSITION_CASE
    X = wpd_cases.make_mixture(COMPOSITION_CASE)
    logits = 3.0 * np.random.default_rng(7).standard_normal((N, F, T))
    soft = np.exp(logits) / np.exp(logits).sum(axis=0, keepdims=True)
    moved = FLOOR
    for mask in (wpd_cases.make_mask(COMPOSITION_CASE), soft):
        base = wpd_numpy.run(X, mask, taps, delay, n_iter=N_ITER)["output"]
        for d in range(DRAWS):
            other = wpd_numpy.run(perturbed(X, d), mask, taps, delay, n_iter=N_ITER)["output"]
            moved = max(moved, float(np.abs(other - base).max()))
    return moved


def main():
    print("# max |restatement(X (1 + 1e-15 xi)) - restatement(X)|, xi ~ N(0, 1) from default_rng(99 + d), "
          "d = 0..{}; n_iter={}, max_flooring(eps=1e-6), diagonal_loading=1e-6; loss: relative; floor "
          "{:.0e}".format(DRAWS - 1, N_ITER, FLOOR))
    print("# bar of tests/test_gpu_wpd.py = 1000 x the movement of the shape and form")
    print("{:>26s} {:>9s} {:>10s} {:>10s} {:>21s} {:>10s}   bars".format(
        "case (M,K,D,N,F,T,B)", "form", "cond(R)", *KEYS))
    for case in wpd_cases.CASES:
        for steering in (False, True):
            moved, cond = movement(case, steering)
            print("{:>26s} {:>9s} {:10.2e} {:10.2e} {:21.2e} {:10.2e}   {}".format(
                str(case).replace(" ", ""), "steering" if steering else "mask", cond,
                *(moved[k] for k in KEYS),
                "  ".join("{:.1e}".format(1000 * moved[k]) for k in KEYS)))
            assert 1000 * moved["output"] <= 1e-7, "ill-determined shape: replace the draw"
    moved = composition()
    print("composition {}: {:.2e}   bar {:.1e}".format(
        str(COMPOSITION_CASE).replace(" ", ""), moved, 1000 * moved))
    assert 1000 * moved <= 1e-7


if __name__ == "__main__":
    main()
