// Hermitian matrix functions of ssspy.linalg on the device, one matrix per lane: generalised
// eigen-decomposition (types 1-3), square root / inverse square root, geometric mean.  Each kernel
// is stated once for a dimension descriptor (hermitian.hpp): compiled in to 6 x 6 (registers), at
// run time for 9 x 9 .. 16 x 16 (private memory; correct, not tuned -- the reference's functions are
// numpy.linalg calls and take any size).  7 x 7 and 8 x 8 run on 8 lanes (hermitian_rows.hip).
//
// replaces: ssspy/linalg/eigh.py:8-81, :164-207 (eigh with B, _eigh), ssspy/linalg/sqrtm.py:8-64
//           (sqrtmh, invsqrtmh), ssspy/linalg/mean.py:6-83 (gmeanmh).
#include "common.hpp"
#include "hermitian_entry.hpp"
#include "ssspy_amd.h"

namespace ssspy {

// generalised Hermitian eigenproblem through the Cholesky factor of B (ref: eigh.py:164-207):
//   type 1: A z = lamb B z   (C = L^-1 A L^-H, z = L^-H y)
//   type 2: A B z = lamb z   (C = L^H A L,    z = L^-H y)
//   type 3: B A z = lamb z   (C = L^H A L,    z = L y)
// eigenvalues ascending; eigenvectors carry the decomposition's phase (as with LAPACK, arbitrary).
template <class D>
__global__ __launch_bounds__(64) void k_eigh_general(D d, const c128 *__restrict__ A,
                                                     const c128 *__restrict__ Bm, double *lamb,
                                                     c128 *Z, long long n, int type, int *info) {
  constexpr int CC = D::cap * D::cap;
  const HermLane ln = herm_lane(n);
  if (!D::shadows_tail && !ln.live) return;
  c128 Am[CC], L[CC], Li[CC], T[CC], P[CC];
  load_matrix(d, Am, A, ln.idx);
  load_matrix(d, L, Bm, ln.idx);
  const bool ok = cholesky_lower(d, L);
  if (!ok && info && ln.live) atomicAdd(info, 1);
  lower_inverse(d, L, Li);
  if (type == 1) {
    matmul(d, Li, Am, T);     // L^-1 A
    matmul_h(d, T, Li, Am);   // (L^-1 A) L^-H
  } else {
    matmul_hl(d, L, Am, T);   // L^H A
    matmul(d, T, L, Am);      // (L^H A) L
  }
  hermitize(d, Am);
  jacobi(d, Am, P);
  if (type == 3)
    matmul(d, L, P, T);
  else
    matmul_hl(d, Li, P, T);   // L^-H P
  if (ln.live) store_sorted(d, Am, T, lamb, Z, ln.idx);
}

// mode 0: X^(1/2); mode 1: P diag(1 / floor(sqrt(lam))) P^H  (ref: sqrtm.py:8-64)
template <class D>
__global__ __launch_bounds__(64) void k_sqrtmh(D d, const c128 *__restrict__ X, c128 *out,
                                               long long n, int mode, int floor_kind, double eps) {
  const int M = d.n();
  const HermLane ln = herm_lane(n);
  if (!D::shadows_tail && !ln.live) return;
  c128 Am[D::cap * D::cap], P[D::cap * D::cap];
  load_matrix(d, Am, X, ln.idx);
  hermitize(d, Am);
  jacobi(d, Am, P);
  double w[D::cap];
#pragma unroll D::unroll
  for (int k = 0; k < M; ++k) {
    const double s = sqrt(Am[k * M + k].x);  // NaN for a negative eigenvalue, as numpy.sqrt
    w[k] = mode == 0 ? s : 1.0 / apply_floor(s, floor_kind, eps);
  }
  rebuild(d, P, w, Am);
  if (ln.live) store_matrix(d, out, Am, ln.idx);
}

// geometric mean through Hermitian square roots: X # Y = X^1/2 (X^-1/2 Y X^-1/2)^1/2 X^1/2 with
//   type 1: A # B;  type 2: A^-1 # B;  type 3: A # B^-1   (ref: mean.py:6-83)
template <class D>
__global__ __launch_bounds__(64) void k_gmeanmh(D d, const c128 *__restrict__ A,
                                                const c128 *__restrict__ Bm, c128 *G, long long n,
                                                int type) {
  constexpr int CC = D::cap * D::cap;
  const int M = d.n();
  const HermLane ln = herm_lane(n);
  if (!D::shadows_tail && !ln.live) return;
  c128 Xm[CC], Ym[CC], P[CC], Out[CC], In[CC];
  // the matrix whose square roots frame the mean, and the one in the middle
  load_matrix(d, Xm, type == 3 ? Bm : A, ln.idx);
  load_matrix(d, Ym, type == 3 ? A : Bm, ln.idx);
  hermitize(d, Xm);
  hermitize(d, Ym);
  jacobi(d, Xm, P);
  // type 1: outer = X^1/2, inner = X^-1/2;  types 2, 3 (mean with an inverse): the roles swap
  double wo[D::cap], wi[D::cap];
#pragma unroll D::unroll
  for (int k = 0; k < M; ++k) {
    const double s = sqrt(Xm[k * M + k].x);
    wo[k] = type == 1 ? s : 1.0 / s;
    wi[k] = type == 1 ? 1.0 / s : s;
  }
  rebuild(d, P, wo, Out);
  rebuild(d, P, wi, In);
  matmul(d, In, Ym, Xm);
  matmul(d, Xm, In, Ym);
  hermitize(d, Ym);
  jacobi(d, Ym, P);
#pragma unroll D::unroll
  for (int k = 0; k < M; ++k) wo[k] = sqrt(fmax(Ym[k * M + k].x, 0.0));
  rebuild(d, P, wo, In);
  matmul(d, Out, In, Xm);
  matmul(d, Xm, Out, Ym);
  hermitize(d, Ym);
  if (ln.live) store_matrix(d, G, Ym, ln.idx);
}

}  // namespace ssspy

using namespace ssspy;

// KERNEL<Runtime> for 9..16, KERNEL<Fixed<M>> to 6 x 6
#define SSSPY_LAUNCH_HERM(KERNEL, ROUTE, M_, ST, ...)                                             \
  do {                                                                                            \
    const dim3 grid = herm_lanes_grid(n), block(64);                                              \
    if ((ROUTE) == HermRoute::RUNTIME) {                                                          \
      hipLaunchKernelGGL((KERNEL<Runtime>), grid, block, 0, ST, Runtime{M_}, __VA_ARGS__);        \
      return check_launch(#KERNEL "_rt");                                                         \
    }                                                                                             \
    DISPATCH_N6(M_, hipLaunchKernelGGL((KERNEL<Fixed<NN>>), grid, block, 0, ST, Fixed<NN>{},      \
                                       __VA_ARGS__));                                             \
    return check_launch(#KERNEL);                                                                 \
  } while (0)

extern "C" {

int ssspy_eigh_general(const void *A, const void *Bm, double *lamb, void *Z, long long n, int M,
                       int type, int *info, void *stream) {
  SSSPY_REQUIRE(A && Bm && lamb && Z && n > 0, "eigh_general: bad argument");
  SSSPY_REQUIRE(type >= 1 && type <= 3, "eigh_general: type must be 1, 2 or 3");
  const HermRoute route = hermitian_route(M);
  if (route == HermRoute::ROWS8)
    return eigh_general_rows(A, Bm, lamb, Z, n, M, type, info, as_stream(stream));
  SSSPY_LAUNCH_HERM(k_eigh_general, route, M, as_stream(stream), (const c128 *)A, (const c128 *)Bm,
                    lamb, (c128 *)Z, n, type, info);
}

int ssspy_sqrtmh(const void *X, void *out, long long n, int M, int inverse, int floor_kind,
                 double floor_eps, void *stream) {
  SSSPY_REQUIRE(X && out && n > 0, "sqrtmh: bad argument");
  const HermRoute route = hermitian_route(M);
  if (route == HermRoute::ROWS8)
    return sqrtmh_rows(X, out, n, M, inverse ? 1 : 0, floor_kind, floor_eps, as_stream(stream));
  SSSPY_LAUNCH_HERM(k_sqrtmh, route, M, as_stream(stream), (const c128 *)X, (c128 *)out, n,
                    inverse ? 1 : 0, floor_kind, floor_eps);
}

int ssspy_gmeanmh(const void *A, const void *Bm, void *G, long long n, int M, int type,
                  void *stream) {
  SSSPY_REQUIRE(A && Bm && G && n > 0, "gmeanmh: bad argument");
  SSSPY_REQUIRE(type >= 1 && type <= 3, "gmeanmh: type must be 1, 2 or 3");
  const HermRoute route = hermitian_route(M);
  if (route == HermRoute::ROWS8) return gmeanmh_rows(A, Bm, G, n, M, type, as_stream(stream));
  SSSPY_LAUNCH_HERM(k_gmeanmh, route, M, as_stream(stream), (const c128 *)A, (const c128 *)Bm,
                    (c128 *)G, n, type);
}

}  // extern "C"
