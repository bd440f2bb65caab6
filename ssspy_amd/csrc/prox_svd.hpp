// The proximal operator of -mu log|det X| of one N x N complex matrix held by one lane:
//   prox(X) = U diag(f(sigma)) V^H,  f(s) = (s + sqrt(s^2 + 4 mu)) / 2,  X = U diag(sigma) V^H
// (ref: ssspy/linalg/prox.py:62-91), by a one-sided (Hestenes) complex Jacobi on X itself: the columns
// of G = X V are rotated until they are orthogonal, with the rotations of the Hermitian Jacobi
// (jacobi_rot, hermitian.hpp) on the 2 x 2 Gram matrices of the column pairs.  Then ||g_k|| =
// sigma_k and prox(X) = sum_k g_k (f(sigma_k) / sigma_k) v_k^H: U is never formed for a non-zero
// singular value.  Working on X, not on X X^H, keeps the error at eps * kappa instead of
// eps * kappa^2 (the arguments PDSBSS hands over reach kappa = 5e3 within ten iterations).
//
// Where a singular value is zero (a column of G vanishes) the result is not determined; the column is
// replaced by a unit vector orthogonal to the other left singular vectors, so the result is finite and
// has the singular values f(sigma).
#pragma once

#include "common.hpp"
#include "hermitian.hpp"

namespace ssspy {

constexpr int PROX_SVD_SWEEPS = 30;
// columns p, q count as orthogonal when |g_p^H g_q|^2 <= PROX_SVD_TOL2 |g_p|^2 |g_q|^2
// (|cos| <= 3e-15: the rounding of a 16-term Gram product is 1e-15, a tighter bound never ends)
constexpr double PROX_SVD_TOL2 = 1e-29;
// a column of the scaled matrix (largest entry in [1/2, 1)) with a squared norm below this is zero
constexpr double PROX_SVD_ZERO2 = 1e-140;

// A (N x N, row-major, leading dimension N): X on entry, on return the columns u_k f(sigma_k);
// V: the right singular vectors in its columns; sv: N doubles of scratch.  prox(X) = A V^H.
// Every lane of the wave must be in the call (the sweep loop ends on a wave vote).
// The sweep loop gives up after PROX_SVD_SWEEPS without a signal: cyclic Jacobi converges
// quadratically, so finite input leaves on the vote long before, and the limit only bounds the run
// time on input that cannot converge (NaN or Inf entries).  Such input gives NaN output: fmax
// drops a NaN from the scale, but its column's norm is NaN and stays so to the end.
__device__ inline void prox_neg_logdet_lane(c128 *A, c128 *V, double *sv, int N, double mu) {
  double amax = 0.0;
  for (int e = 0; e < N * N; ++e) amax = fmax(amax, fmax(fabs(A[e].x), fabs(A[e].y)));
  // scale by a power of two (exact) so that Gram products neither overflow nor underflow
  const bool scalable = amax > 0.0 && amax < 1.79e308;
  const int ex = scalable ? __builtin_amdgcn_frexp_exp(amax) : 0;
  for (int e = 0; e < N * N; ++e) A[e] = cmake(ldexp(A[e].x, -ex), ldexp(A[e].y, -ex));
  for (int r = 0; r < N; ++r)
    for (int c = 0; c < N; ++c) V[r * N + c] = cmake(r == c ? 1.0 : 0.0, 0.0);
  for (int sweep = 0; sweep < PROX_SVD_SWEEPS; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        double alpha = 0.0, beta = 0.0;
        c128 gamma = cmake(0.0, 0.0);  // g_p^H g_q
        for (int r = 0; r < N; ++r) {
          const c128 ap = A[r * N + p], aq = A[r * N + q];
          alpha += cabs2(ap);
          beta += cabs2(aq);
          cfma(gamma, cconj(ap), aq);
        }
        const double mag2 = cabs2(gamma);
        if (mag2 > PROX_SVD_TOL2 * alpha * beta && mag2 >= 1e-300) {
          rotated = true;
          const JacobiRot rot = jacobi_rot(gamma, alpha, beta);
          const double cs = rot.cs;
          const c128 su = rot.su, sub = cconj(rot.su);
          // g_p' = c g_p - s conj(u) g_q ; g_q' = s u g_p + c g_q, and the same on V
          for (int r = 0; r < N; ++r) {
            const c128 ap = A[r * N + p], aq = A[r * N + q];
            c128 np_ = cmake(cs * ap.x, cs * ap.y);
            cfms(np_, sub, aq);
            c128 nq_ = cmake(cs * aq.x, cs * aq.y);
            cfma(nq_, su, ap);
            A[r * N + p] = np_;
            A[r * N + q] = nq_;
            const c128 vp = V[r * N + p], vq = V[r * N + q];
            c128 mp_ = cmake(cs * vp.x, cs * vp.y);
            cfms(mp_, sub, vq);
            c128 mq_ = cmake(cs * vq.x, cs * vq.y);
            cfma(mq_, su, vp);
            V[r * N + p] = mp_;
            V[r * N + q] = mq_;
          }
        }
      }
    if (__all(!rotated)) break;
  }
  // singular values of the scaled matrix; the non-zero columns become the left singular vectors
  bool any_zero = false;
  for (int k = 0; k < N; ++k) {
    double a2 = 0.0;
    for (int r = 0; r < N; ++r) a2 += cabs2(A[r * N + k]);
    if (a2 >= PROX_SVD_ZERO2) {
      const double s = sqrt(a2), inv = 1.0 / s;
      sv[k] = s;
      for (int r = 0; r < N; ++r) A[r * N + k] = cscale(A[r * N + k], inv);
    } else if (a2 == a2) {
      sv[k] = -1.0;  // (a zero column, to be completed)
      any_zero = true;
    } else {
      sv[k] = a2;  // NaN in, NaN out: the column is never completed and f(NaN) scales it below
    }
  }
  if (any_zero) {
    for (int k = 0; k < N; ++k) {
      if (!(sv[k] < 0.0)) continue;  // (stands, or NaN)
      // the unit vector e_j farthest from the span of the columns that stand
      int best = 0;
      double best_res = -1.0;
      for (int j = 0; j < N; ++j) {
        double res = 1.0;
        for (int c = 0; c < N; ++c)
          if (sv[c] >= 0.0) res -= cabs2(A[j * N + c]);
        if (res > best_res) {
          best_res = res;
          best = j;
        }
      }
      for (int r = 0; r < N; ++r) A[r * N + k] = cmake(r == best ? 1.0 : 0.0, 0.0);
      for (int pass = 0; pass < 2; ++pass)  // Gram-Schmidt, twice
        for (int c = 0; c < N; ++c) {
          if (!(sv[c] >= 0.0)) continue;
          c128 dot = cmake(0.0, 0.0);  // u_c^H w
          for (int r = 0; r < N; ++r) cfma(dot, cconj(A[r * N + c]), A[r * N + k]);
          for (int r = 0; r < N; ++r) cfms(A[r * N + k], A[r * N + c], dot);
        }
      double w2 = 0.0;
      for (int r = 0; r < N; ++r) w2 += cabs2(A[r * N + k]);
      const double inv = 1.0 / sqrt(w2);
      for (int r = 0; r < N; ++r) A[r * N + k] = cscale(A[r * N + k], inv);
      sv[k] = 0.0;
    }
  }
  for (int k = 0; k < N; ++k) {
    const double s = ldexp(sv[k], ex);
    const double f = 0.5 * (s + sqrt(fma(s, s, 4.0 * mu)));
    for (int r = 0; r < N; ++r) A[r * N + k] = cscale(A[r * N + k], f);
  }
}

// entry (r, c) of A V^H
__device__ inline c128 prox_entry(const c128 *A, const c128 *V, int N, int r, int c) {
  c128 s = cmake(0.0, 0.0);
  for (int k = 0; k < N; ++k) cfma(s, A[r * N + k], cconj(V[c * N + k]));
  return s;
}

}  // namespace ssspy
