#!/usr/bin/env python3
"""How far the NumPy restatement of WPE (tests/wpe_numpy.py) moves under a 1e-15 relative
perturbation of its input, per test shape (tests/wpe_cases.py): the yardstick of the bars of
tests/test_gpu_wpe.py, which allows 1000 x the movement of each shape -- a different summation order
is a perturbation of that size, amplified by cond(R) like this one.  A shape that moves by more than
1e-6 is ill-determined and has to be replaced by a better-conditioned draw.  CPU only.

    python benchmarks/tools/wpe_sensitivity.py > profiles/wpe_sensitivity.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import wpe_cases  # noqa: E402
import wpe_numpy  # noqa: E402

KEYS = ("output", "prediction_filter", "loss")
N_ITER = 3


def movement(case, n_iter=N_ITER, draws=3):
    """max |restatement(X (1 + 1e-15 xi)) - restatement(X)| per quantity (loss: relative), and the
    largest cond(R) of the last iteration."""
    _, taps, delay = case[:3]
    X = wpe_cases.make_mixture(case)
    base = wpe_numpy.run(X, taps, delay, n_iter=n_iter, statistics=True)
    moved = dict.fromkeys(KEYS, 0.0)
    for d in range(draws):
        xi = np.random.default_rng(99 + d).standard_normal(X.shape)
        other = wpe_numpy.run(X * (1 + 1e-15 * xi), taps, delay, n_iter=n_iter)
        for key in KEYS[:2]:
            moved[key] = max(moved[key], float(np.abs(other[key] - base[key]).max()))
        rel = np.abs(np.asarray(other["loss"]) / np.asarray(base["loss"]) - 1).max()
        moved["loss"] = max(moved["loss"], float(rel))
    R = base["R"].reshape(-1, *base["R"].shape[-2:])
    return moved, max(float(np.linalg.cond(r)) for r in R)


def main():
    print("# max |restatement(X (1 + 1e-15 xi)) - restatement(X)|, xi ~ N(0, 1) from default_rng(99 + d), "
          "d = 0..2; n_iter={}, max_flooring(eps=1e-10); loss: relative".format(N_ITER))
    print("# bar of tests/test_gpu_wpe.py = 1000 x the movement of the shape")
    print("{:>24s} {:>10s} {:>10s} {:>18s} {:>10s}   bars".format(
        "case (M,K,D,F,T,B)", "cond(R)", *KEYS))
    for case in wpe_cases.CASES:
        moved, cond = movement(case)
        print("{:>24s} {:10.2e} {:10.2e} {:18.2e} {:10.2e}   {}".format(
            str(case).replace(" ", ""), cond, *(moved[k] for k in KEYS),
            "  ".join("{:.1e}".format(1000 * moved[k]) for k in KEYS)))
        assert max(moved.values()) <= 1e-6, "ill-determined shape: replace the draw"
    print("composition {}: {:.2e}   bar {:.1e}".format(
        str(COMPOSITION_CASE).replace(" ", ""), composition(), 1000 * composition()))


COMPOSITION_CASE = (2, 3, 1, 9, 64, 1)


def composition():
    """The same movement for the composition test: GaussILRMA(n_basis=2), 3 iterations (the NumPy
    oracle, fixed basis and activation), behind WPE(taps=3, delay=1), 2 iterations, on (2, 9, 64)."""
    sys.path.insert(0, ROOT)
    from oracle.ilrma import GaussILRMAOracle

    M, K, D, F, T, _ = COMPOSITION_CASE
    X = wpe_cases.make_mixture(COMPOSITION_CASE)
    basis = np.random.default_rng(1).random((M, F, 2))
    activation = np.random.default_rng(2).random((M, 2, T))

    def chain(Z):
        Y = wpe_numpy.run(Z, K, D, n_iter=2)["output"]
        return GaussILRMAOracle(n_basis=2).run(Y, n_iter=3, basis=basis, activation=activation)

    base, moved = chain(X), 0.0
    for d in range(3):
        xi = np.random.default_rng(99 + d).standard_normal(X.shape)
        moved = max(moved, float(np.abs(chain(X * (1 + 1e-15 * xi)) - base).max()))
    return moved


if __name__ == "__main__":
    main()
