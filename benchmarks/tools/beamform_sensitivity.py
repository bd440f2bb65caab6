#!/usr/bin/env python3
"""How far the NumPy restatement of the mask-based beamformers (tests/beamform_numpy.py) moves under
a 1e-15 relative perturbation of its input, per test shape (tests/beamform_cases.py) and beamformer:
the yardstick of the bars of tests/test_gpu_beamform.py, which allows 1000 x the movement -- a
different summation order is a perturbation of that size, amplified by cond(Phi_v) and the eigen-gap
like this one.  Every bar has to come out <= 1e-8 on outputs of RMS about 1: a shape that moves by
more has a degenerate eigen-gap or an ill-conditioned Phi_v and has to be replaced by another draw.
CPU only.

    python benchmarks/tools/beamform_sensitivity.py > profiles/beamform_sensitivity.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beamform_cases  # noqa: E402
import beamform_numpy  # noqa: E402

KEYS = ("output", "demix_filter")
DRAWS = 3
# a movement of exactly zero (one channel, where w = 1 up to a factor) still gets a bar: the rounding
# of a handful of operations on numbers of order one
FLOOR = 1e-15


def perturbed(X, d):
    xi = np.random.default_rng(99 + d).standard_normal(X.shape)
    return X * (1 + 1e-15 * xi)


def movement(case, kind, kwargs):
    X, mask, noise_mask = beamform_cases.make_case(case)
    base = beamform_numpy.run(X, mask, noise_mask, kind=kind, **kwargs)
    moved = dict.fromkeys(KEYS, FLOOR)
    for d in range(DRAWS):
        other = beamform_numpy.run(perturbed(X, d), mask, noise_mask, kind=kind, **kwargs)
        for key in KEYS:
            moved[key] = max(moved[key], float(np.abs(other[key] - base[key]).max()))
    rms = float(np.sqrt(np.mean(np.abs(base["output"]) ** 2)))
    cond = max(float(np.linalg.cond(v))
               for v in base["noise_covariance"].reshape(-1, *base["noise_covariance"].shape[-2:]))
    return moved, rms, cond


COMPOSITION_CASE = (3, 2, 9, 64, 1)  # (n_channels, n_sources, n_bins, n_frames, n_mixtures)


def composition():
    """The same movement for the composition test: MVDR(reference_id=0) behind WPE(taps=3, delay=1),
    3 iterations, on (3 channels, 9 bins, 64 frames) with two masks held fixed (the test feeds the
    posterior of its device run to both sides).  The masks here stand in for that posterior: the
    ideal ratio masks of the draw and a random soft assignment, the larger movement of the two."""
    import wpe_numpy

    X, irm, _ = beamform_cases.make_case(COMPOSITION_CASE)
    logits = np.random.default_rng(7).standard_normal(irm.shape)
    soft = np.exp(logits) / np.exp(logits).sum(axis=0, keepdims=True)

    def chain(Z, mask):
        Y = wpe_numpy.run(Z, 3, 1, n_iter=3)["output"]
        return beamform_numpy.run(Y, mask, None, kind="mvdr", loading=1e-6)["output"]

    moved = FLOOR
    for mask in (irm, soft):
        base = chain(X, mask)
        for d in range(DRAWS):
            moved = max(moved, float(np.abs(chain(perturbed(X, d), mask) - base).max()))
    return moved


def main():
    print("# max |restatement(X (1 + 1e-15 xi)) - restatement(X)|, xi ~ N(0, 1) from default_rng(99 + d), "
          "d = 0..{}; floor {:.0e}".format(DRAWS - 1, FLOOR))
    print("# bar of tests/test_gpu_beamform.py = 1000 x the movement of the shape and beamformer")
    print("{:>20s} {:>14s} {:>9s} {:>10s} {:>10s} {:>12s}   bars".format(
        "case (M,N,F,T,B)", "beamformer", "rms(out)", "cond(Phi_v)", *KEYS))
    for case in beamform_cases.CASES:
        for name, kind, kwargs, _, _ in beamform_cases.BEAMFORMERS:
            moved, rms, cond = movement(case, kind, kwargs)
            print("{:>20s} {:>14s} {:9.2e} {:10.2e} {:10.2e} {:12.2e}   {}".format(
                str(case).replace(" ", ""), name, rms, cond, *(moved[k] for k in KEYS),
                "  ".join("{:.1e}".format(1000 * moved[k]) for k in KEYS)))
            assert 1000 * max(moved.values()) <= 1e-8, "ill-determined shape: replace the draw"
    moved = composition()
    print("composition {}: {:.2e}   bar {:.1e}".format(
        str(COMPOSITION_CASE).replace(" ", ""), moved, 1000 * moved))
    assert 1000 * moved <= 1e-8


if __name__ == "__main__":
    main()
