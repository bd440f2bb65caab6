// Small Hermitian matrices held by one lane: Jacobi eigen-decomposition and functions of a
// matrix through it (to_psd, inverse, square roots, Cholesky).  Every routine is stated once, on a
// flat row-major matrix with leading dimension d.n(), for a dimension descriptor d:
//   Fixed<M>        size at compile time, loops fully unrolled: the matrix sits in registers
//   Fixed<M, true>  size at compile time, loops rolled: the matrix is indexed at run time and sits in
//                   the lane's private memory -- for the repair kernels that hold an M x M working set
//                   per lane from 5 channels on (unrolled they spill 500-2 400 VGPRs and their code is
//                   megabytes; they run only where an eigenvalue floor may act).  Jacobi, rebuild and
//                   matmul are calls there, not inlined.
//   Runtime{n}      size at run time (to SSSPY_RT_MAX_SOURCES), loops rolled, private memory
// What differs between the descriptors beyond the storage is a named trait below.
#pragma once

#include "common.hpp"
#include "ssspy_amd.h"

namespace ssspy {

template <int M, bool ROLLED = false>
struct Fixed {
  static constexpr int cap = M;                          // rows of a caller's array
  static constexpr int unroll = ROLLED ? 1 : M * M + 1;  // above every trip count: fully unrolled
  static constexpr bool called = ROLLED;
  // kept differences between the size routes ("Per-lane Hermitian routines")
  static constexpr bool skips_resolved_pairs = false;  // the cluster threshold came with 9..16 only
  static constexpr bool psd_full_rebuild = true;       // to_psd: all M^2 sums, averaged with the adjoint
  static constexpr bool shadows_tail = false;          // a lane past the end leaves its wave's votes
  __device__ constexpr int n() const { return M; }
  // rolled, the sweeps and sums are; the passes over single entries have always stayed unrolled
  __device__ constexpr Fixed<M> entrywise() const { return {}; }
};
struct Runtime {
  int size;
  static constexpr int cap = SSSPY_RT_MAX_SOURCES;
  static constexpr int unroll = 1;
  static constexpr bool called = false;
  static constexpr bool skips_resolved_pairs = true;
  static constexpr bool psd_full_rebuild = false;  // to_psd: the upper triangle, mirrored
  static constexpr bool shadows_tail = true;       // a lane past the end works on the last matrix
  __device__ int n() const { return size; }
  __device__ Runtime entrywise() const { return *this; }
};

// The rotation that annihilates A[p][q] of a Hermitian matrix: cs, su = s u (u = apq / |apq|) and
// tm = t |apq| (A_pp -= tm, A_qq += tm).  Round 6: reciprocals and square roots by v_rcp_f64 /
// v_rsq_f64 + two Newton steps (~1 ulp; the 8-lane form herm_rows8.hpp has used them since round 5)
// instead of three IEEE divides and two square roots -- ~170 of a rotation's dependent
// instructions in kernels that are chains of rotations (IPA's LQPQM, the Hermitian operators).
// Range: |apq|^2 is brought to [1/4, 2) by its exponent before the reciprocal square root and
// scaled back, tau is capped at 1e150 (beyond it t < 5e-151: the rotation is the identity to any
// rounding) -- no slow branch; |apq|^2 below 1e-300 (or NaN) leaves the pair alone.
struct JacobiRot {
  double cs, tm;
  c128 su;
};
__device__ __forceinline__ double jr_rsq(double x) {
  double r = __builtin_amdgcn_rsq(x);
  double h = 0.5 * x * r;
  double e = fma(-h, r, 0.5);
  r = fma(r, e, r);
  h = 0.5 * x * r;
  e = fma(-h, r, 0.5);
  return fma(r, e, r);
}
__device__ __forceinline__ double jr_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  double e = fma(-x, r, 1.0);
  r = fma(r, e, r);
  e = fma(-x, r, 1.0);
  return fma(r, e, r);
}
__device__ __forceinline__ JacobiRot jacobi_rot(c128 apq, double app, double aqq) {
  const double mag2 = cabs2(apq);
  const bool tiny = !(mag2 >= 1e-300);
  const int half = __builtin_amdgcn_frexp_exp(tiny ? 1.0 : mag2) >> 1;  // mag2 = s 4^half, s in [1/4, 2)
  const double inv = tiny ? 0.0 : ldexp(jr_rsq(ldexp(mag2, -2 * half)), -half);  // 1 / |apq|
  const double mag = tiny ? 0.0 : mag2 * inv;
  const c128 u = tiny ? cmake(1.0, 0.0) : cmake(apq.x * inv, apq.y * inv);
  const double tau = tiny ? 0.0 : (aqq - app) * 0.5 * inv;
  const double atau = fmin(fabs(tau), 1e150);
  const double w = fma(atau, atau, 1.0);
  const double tabs = jr_rcp(fma(w, jr_rsq(w), atau));  // 1 / (|tau| + sqrt(1 + tau^2))
  const double t = tiny ? 0.0 : (tau >= 0.0 ? tabs : -tabs);
  JacobiRot r;
  r.cs = jr_rsq(fma(t, t, 1.0));
  const double sn = t * r.cs;
  r.su = cmake(sn * u.x, sn * u.y);
  r.tm = t * mag;
  return r;
}

// (A + A^H) / 2 in place
template <class D>
__device__ __forceinline__ void hermitize(D d, c128 *A) {
  const int n = d.n();
#pragma unroll D::unroll
  for (int a = 0; a < n; ++a) {
    A[a * n + a] = cmake(A[a * n + a].x, 0.0);
#pragma unroll D::unroll
    for (int b = a + 1; b < n; ++b) {
      const c128 z = cmake(0.5 * (A[a * n + b].x + A[b * n + a].x),
                           0.5 * (A[a * n + b].y - A[b * n + a].y));
      A[a * n + b] = z;
      A[b * n + a] = cconj(z);
    }
  }
}

// Hermitian eigen-decomposition by cyclic complex Jacobi rotations: A = P diag(lam) P^H, lam left on
// the diagonal of A.  The sweep loop ends when every lane of the wave has a negligible off-diagonal,
// at most 12 sweeps: every lane of the wave that has not left the kernel must be in the call.
template <class D>
__device__ __forceinline__ void jacobi_sweeps(D d, c128 *A, c128 *P) {
  const int n = d.n();
#pragma unroll D::unroll
  for (int r = 0; r < n; ++r)
#pragma unroll D::unroll
    for (int c = 0; c < n; ++c) P[r * n + c] = cmake(r == c ? 1.0 : 0.0, 0.0);
#pragma unroll 1
  for (int sweep = 0; sweep < 12; ++sweep) {
    double off = 0.0, diag = 0.0;
#pragma unroll D::unroll
    for (int p = 0; p < n; ++p) {
      diag = fma(A[p * n + p].x, A[p * n + p].x, diag);
#pragma unroll D::unroll
      for (int q = p + 1; q < n; ++q) off += cabs2(A[p * n + q]);
    }
    if (__all(off <= 1e-34 * diag)) break;
    // skips_resolved_pairs: a pair whose coupling is below 1e-16 sqrt(|a_pp a_qq|) is left alone (the
    // relative criterion of the one-sided Jacobi methods).  Inside a cluster of eigenvalues the
    // diagonal difference and the coupling are both rounding noise once the cluster is resolved, their
    // ratio is an angle of order one, and the normwise criterion above sits at that noise level for
    // 13 x 13 and more: without the threshold such a matrix turns through all 12 sweeps and its
    // eigenvectors lose orthonormality turn by turn (16 x 16, eigenvalues 1 and one 1 + 1e-9: 670 u;
    // LAPACK: 53).  What is left standing is below u ||A|| in the residual.  A sweep in which no lane
    // turned a pair ends the loop.
    bool turned = false;
#pragma unroll D::unroll
    for (int p = 0; p < n - 1; ++p)
#pragma unroll D::unroll
      for (int q = p + 1; q < n; ++q) {
        const double app = A[p * n + p].x, aqq = A[q * n + q].x;
        if constexpr (D::skips_resolved_pairs) {
          if (cabs2(A[p * n + q]) <= 1e-32 * fabs(app * aqq)) continue;
          turned = true;
        }
        const JacobiRot rot = jacobi_rot(A[p * n + q], app, aqq);
        const double cs = rot.cs;
        const c128 su = rot.su;           // s u
        const c128 sub = cconj(rot.su);   // s conj(u)
#pragma unroll D::unroll
        for (int k = 0; k < n; ++k) {
          if (k != p && k != q) {
            const c128 akp = A[k * n + p], akq = A[k * n + q];
            // A'_kp = c A_kp - s conj(u) A_kq ; A'_kq = s u A_kp + c A_kq
            c128 nkp = cmake(cs * akp.x, cs * akp.y);
            cfms(nkp, sub, akq);
            c128 nkq = cmake(cs * akq.x, cs * akq.y);
            cfma(nkq, su, akp);
            A[k * n + p] = nkp;
            A[p * n + k] = cconj(nkp);
            A[k * n + q] = nkq;
            A[q * n + k] = cconj(nkq);
          }
        }
        A[p * n + p] = cmake(app - rot.tm, 0.0);
        A[q * n + q] = cmake(aqq + rot.tm, 0.0);
        A[p * n + q] = cmake(0.0, 0.0);
        A[q * n + p] = cmake(0.0, 0.0);
#pragma unroll D::unroll
        for (int k = 0; k < n; ++k) {
          const c128 vkp = P[k * n + p], vkq = P[k * n + q];
          c128 nkp = cmake(cs * vkp.x, cs * vkp.y);
          cfms(nkp, sub, vkq);
          c128 nkq = cmake(cs * vkq.x, cs * vkq.y);
          cfma(nkq, su, vkp);
          P[k * n + p] = nkp;
          P[k * n + q] = nkq;
        }
      }
    if constexpr (D::skips_resolved_pairs) {
      if (!__any(turned)) break;
    }
  }
}

// Out = P diag(w) P^H (exactly Hermitian)
template <class D>
__device__ __forceinline__ void rebuild_sums(D d, const c128 *P, const double *w, c128 *Out) {
  const int n = d.n();
#pragma unroll D::unroll
  for (int a = 0; a < n; ++a)
#pragma unroll D::unroll
    for (int b = a; b < n; ++b) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll D::unroll
      for (int k = 0; k < n; ++k) {
        const c128 t = cmulc(P[a * n + k], P[b * n + k]);  // P_ak conj(P_bk)
        s.x = fma(w[k], t.x, s.x);
        s.y = fma(w[k], t.y, s.y);
      }
      if (a == b) s.y = 0.0;
      Out[a * n + b] = s;
      Out[b * n + a] = cconj(s);
    }
}

// C = A B (general complex)
template <class D>
__device__ __forceinline__ void matmul_sums(D d, const c128 *A, const c128 *B, c128 *C) {
  const int n = d.n();
#pragma unroll D::unroll
  for (int a = 0; a < n; ++a)
#pragma unroll D::unroll
    for (int b = 0; b < n; ++b) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll D::unroll
      for (int k = 0; k < n; ++k) cfma(s, A[a * n + k], B[k * n + b]);
      C[a * n + b] = s;
    }
}

// jacobi, rebuild, matmul: the three bodies above, as calls where the descriptor says so (D::called)
template <class D>
__device__ __noinline__ void jacobi_call(D d, c128 *A, c128 *P) { jacobi_sweeps(d, A, P); }
template <class D>
__device__ __noinline__ void rebuild_call(D d, const c128 *P, const double *w, c128 *Out) {
  rebuild_sums(d, P, w, Out);
}
template <class D>
__device__ __noinline__ void matmul_call(D d, const c128 *A, const c128 *B, c128 *C) {
  matmul_sums(d, A, B, C);
}
template <class D>
__device__ __forceinline__ void jacobi(D d, c128 *A, c128 *P) {
  if constexpr (D::called) jacobi_call(d, A, P);
  else jacobi_sweeps(d, A, P);
}
template <class D>
__device__ __forceinline__ void rebuild(D d, const c128 *P, const double *w, c128 *Out) {
  if constexpr (D::called) rebuild_call(d, P, w, Out);
  else rebuild_sums(d, P, w, Out);
}
template <class D>
__device__ __forceinline__ void matmul(D d, const c128 *A, const c128 *B, c128 *C) {
  if constexpr (D::called) matmul_call(d, A, B, C);
  else matmul_sums(d, A, B, C);
}

// C = A B^H
template <class D>
__device__ __forceinline__ void matmul_h(D d, const c128 *A, const c128 *B, c128 *C) {
  const int n = d.n();
#pragma unroll D::unroll
  for (int a = 0; a < n; ++a)
#pragma unroll D::unroll
    for (int b = 0; b < n; ++b) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll D::unroll
      for (int k = 0; k < n; ++k) cfma(s, A[a * n + k], cconj(B[b * n + k]));
      C[a * n + b] = s;
    }
}

// C = A^H B
template <class D>
__device__ __forceinline__ void matmul_hl(D d, const c128 *A, const c128 *B, c128 *C) {
  const int n = d.n();
#pragma unroll D::unroll
  for (int a = 0; a < n; ++a)
#pragma unroll D::unroll
    for (int b = 0; b < n; ++b) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll D::unroll
      for (int k = 0; k < n; ++k) cfma(s, cconj(A[k * n + a]), B[k * n + b]);
      C[a * n + b] = s;
    }
}

// to_psd: Hermitise, eigen-decompose, floor the eigenvalues; returns the floored eigenvalues in
// lam and the eigenvectors in P (A is destroyed).  ref: ssspy/special/psd.py:11-71.
template <class D>
__device__ __forceinline__ void psd_eigen(D d, c128 *A, c128 *P, double *lam, int floor_kind,
                                          double eps) {
  const int n = d.n();
  using E = decltype(d.entrywise());
  hermitize(d.entrywise(), A);
  jacobi(d, A, P);
#pragma unroll E::unroll
  for (int k = 0; k < n; ++k) lam[k] = apply_floor(A[k * n + k].x, floor_kind, eps);
}

// Lower Cholesky factor of a Hermitian positive definite matrix in place (the strict upper part is
// neither read nor written); logdet = log det A.  False: a pivot was not positive.
template <class D>
__device__ __forceinline__ bool cholesky_factor(D d, c128 *A, double &logdet) {
  const int n = d.n();
  bool ok = true;
  double ld = 0.0;
#pragma unroll D::unroll
  for (int c = 0; c < n; ++c) {
    double dg = A[c * n + c].x;
#pragma unroll D::unroll
    for (int k = 0; k < c; ++k) dg -= cabs2(A[c * n + k]);
    ok = ok && (dg > 0.0);
    const double dd = dg > 0.0 ? dg : 1.0;
    const double l = sqrt(dd), il = 1.0 / l;
    ld += log(dd);
    A[c * n + c] = cmake(l, 0.0);
#pragma unroll D::unroll
    for (int r = c + 1; r < n; ++r) {
      c128 s = A[r * n + c];
#pragma unroll D::unroll
      for (int k = 0; k < c; ++k) cfms(s, A[r * n + k], cconj(A[c * n + k]));
      A[r * n + c] = cscale(s, il);
    }
  }
  logdet = ld;
  return ok;
}

// the same with the strict upper part zeroed
template <class D>
__device__ __forceinline__ bool cholesky_lower(D d, c128 *A) {
  const int n = d.n();
  double logdet;
  const bool ok = cholesky_factor(d, A, logdet);
#pragma unroll D::unroll
  for (int c = 0; c < n; ++c)
#pragma unroll D::unroll
    for (int r = 0; r < c; ++r) A[r * n + c] = cmake(0.0, 0.0);
  return ok;
}

// Inverse and log-determinant of a Hermitian positive definite matrix by Cholesky (A = L L^H,
// A^-1 = L^-H L^-1).  A is destroyed (its lower triangle becomes L), Li is scratch (L^-1).  Returns
// false when a pivot is not positive.
template <class D>
__device__ __forceinline__ bool chol_inverse(D d, c128 *A, c128 *Inv, c128 *Li, double &logdet) {
  const int n = d.n();
  const bool ok = cholesky_factor(d, A, logdet);
  // Linv (lower): forward substitution on the identity, the diagonal of L being real
#pragma unroll D::unroll
  for (int c = 0; c < n; ++c) {
#pragma unroll D::unroll
    for (int r = 0; r < n; ++r) Li[r * n + c] = cmake(0.0, 0.0);
    Li[c * n + c] = cmake(1.0 / A[c * n + c].x, 0.0);
#pragma unroll D::unroll
    for (int r = c + 1; r < n; ++r) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll D::unroll
      for (int k = c; k < r; ++k) cfms(s, A[r * n + k], Li[k * n + c]);
      Li[r * n + c] = cscale(s, 1.0 / A[r * n + r].x);
    }
  }
  // Inv = Linv^H Linv
#pragma unroll D::unroll
  for (int a = 0; a < n; ++a)
#pragma unroll D::unroll
    for (int b = a; b < n; ++b) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll D::unroll
      for (int k = b; k < n; ++k) {
        const c128 t = cmulc(Li[k * n + b], Li[k * n + a]);  // conj(Li[k][a]) Li[k][b]
        s.x += t.x;
        s.y += t.y;
      }
      if (a == b) s.y = 0.0;
      Inv[a * n + b] = s;
      Inv[b * n + a] = cconj(s);
    }
  return ok;
}

// inverse of a lower triangular matrix with a complex diagonal (lower triangular)
template <class D>
__device__ __forceinline__ void lower_inverse(D d, const c128 *L, c128 *Li) {
  const int n = d.n();
#pragma unroll D::unroll
  for (int c = 0; c < n; ++c) {
#pragma unroll D::unroll
    for (int r = 0; r < n; ++r) Li[r * n + c] = cmake(0.0, 0.0);
    Li[c * n + c] = crecip(L[c * n + c]);
#pragma unroll D::unroll
    for (int r = c + 1; r < n; ++r) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll D::unroll
      for (int k = c; k < r; ++k) cfms(s, L[r * n + k], Li[k * n + c]);
      Li[r * n + c] = cmul(s, crecip(L[r * n + r]));
    }
  }
}

// ascending eigenvalues by rank (ties by index: no dynamic indexing of the matrix) and the columns of
// P in that order, into matrix idx of lamb (.., n) and V (.., n, n)
template <class D>
__device__ __forceinline__ void store_sorted(D d, const c128 *Dg, const c128 *P, double *lamb, c128 *V,
                                             long long idx) {
  const int n = d.n();
#pragma unroll D::unroll
  for (int k = 0; k < n; ++k) {
    const double lk = Dg[k * n + k].x;
    int rank = 0;
#pragma unroll D::unroll
    for (int j = 0; j < n; ++j) {
      const double lj = Dg[j * n + j].x;
      rank += (lj < lk || (lj == lk && j < k)) ? 1 : 0;
    }
    lamb[idx * n + rank] = lk;
#pragma unroll D::unroll
    for (int r = 0; r < n; ++r) V[(idx * n + r) * n + rank] = P[r * n + k];
  }
}

// lam_min(A) > shift by the pivots of the Cholesky factorisation of A - shift I (W: working copy)
__device__ inline bool rt_shifted_pd(const c128 *A, c128 *W, int N, double shift) {
  bool ok = true;
  for (int c = 0; c < N; ++c) {
    double d = A[c * N + c].x - shift;
    for (int k = 0; k < c; ++k) d -= cabs2(W[c * N + k]);
    ok = ok && (d > 0.0);
    const double il = 1.0 / sqrt(d > 0.0 ? d : 1.0);
    for (int r = c + 1; r < N; ++r) {
      c128 sum = A[r * N + c];
      for (int k = 0; k < c; ++k) cfms(sum, W[r * N + k], cconj(W[c * N + k]));
      W[r * N + c] = cscale(sum, il);
    }
  }
  return ok;
}

// The fixed sizes under the names and array types of the hot kernels' call sites
template <int M>
__device__ __forceinline__ void hermitize(c128 (&A)[M][M]) { hermitize(Fixed<M>{}, &A[0][0]); }
template <int M, bool ROLLED = false>
__device__ __forceinline__ void jacobi_eigh(c128 (&A)[M][M], c128 (&P)[M][M]) {
  jacobi(Fixed<M, ROLLED>{}, &A[0][0], &P[0][0]);
}
template <int M, bool ROLLED = false>
__device__ __forceinline__ void herm_rebuild(const c128 (&P)[M][M], const double (&w)[M],
                                             c128 (&Out)[M][M]) {
  rebuild(Fixed<M, ROLLED>{}, &P[0][0], w, &Out[0][0]);
}
template <int M, bool ROLLED = false>
__device__ __forceinline__ void matmul(const c128 (&A)[M][M], const c128 (&B)[M][M],
                                       c128 (&C)[M][M]) {
  matmul(Fixed<M, ROLLED>{}, &A[0][0], &B[0][0], &C[0][0]);
}
template <int M, bool ROLLED = false>
__device__ __forceinline__ void psd_eigen(c128 (&A)[M][M], c128 (&P)[M][M], double (&lam)[M],
                                          int floor_kind, double eps) {
  psd_eigen(Fixed<M, ROLLED>{}, &A[0][0], &P[0][0], lam, floor_kind, eps);
}
// NOT MERGED: the register form of chol_inverse keeps its own statement.  Through the descriptor the
// same arithmetic schedules differently and costs the kernels that benchmarks time registers
// (k_gmnmf_separate<8, 8>: 0 -> 170 spilled VGPRs, scratch 3 424 -> 4 000 bytes; k_gmnmf_loss<8, 16>:
// 88 -> 98 AGPRs).  A fix to chol_inverse(D, ...) above has to be made here too.
template <int M>
__device__ __forceinline__ bool chol_inverse(c128 (&A)[M][M], c128 (&Inv)[M][M], double &logdet) {
  bool ok = true;
  double ld = 0.0;
  // in-place lower Cholesky: A[r][c], r >= c, becomes L
#pragma unroll
  for (int c = 0; c < M; ++c) {
    double d = A[c][c].x;
#pragma unroll
    for (int k = 0; k < c; ++k) d -= cabs2(A[c][k]);
    ok = ok && (d > 0.0);
    const double dd = d > 0.0 ? d : 1.0;
    const double l = sqrt(dd), il = 1.0 / l;
    ld += log(dd);
    A[c][c] = cmake(l, 0.0);
#pragma unroll
    for (int r = c + 1; r < M; ++r) {
      c128 s = A[r][c];
#pragma unroll
      for (int k = 0; k < c; ++k) cfms(s, A[r][k], cconj(A[c][k]));
      A[r][c] = cscale(s, il);
    }
  }
  logdet = ld;
  // Linv (lower): forward substitution on the identity
  c128 Li[M][M];
#pragma unroll
  for (int c = 0; c < M; ++c) {
#pragma unroll
    for (int r = 0; r < M; ++r) Li[r][c] = cmake(0.0, 0.0);
    Li[c][c] = cmake(1.0 / A[c][c].x, 0.0);
#pragma unroll
    for (int r = c + 1; r < M; ++r) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll
      for (int k = c; k < r; ++k) cfms(s, A[r][k], Li[k][c]);
      Li[r][c] = cscale(s, 1.0 / A[r][r].x);
    }
  }
  // Inv = Linv^H Linv
#pragma unroll
  for (int a = 0; a < M; ++a)
#pragma unroll
    for (int b = a; b < M; ++b) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll
      for (int k = b; k < M; ++k) {
        const c128 t = cmulc(Li[k][b], Li[k][a]);  // conj(Li[k][a]) Li[k][b]
        s.x += t.x;
        s.y += t.y;
      }
      if (a == b) s.y = 0.0;
      Inv[a][b] = s;
      Inv[b][a] = cconj(s);
    }
  return ok;
}

}  // namespace ssspy
