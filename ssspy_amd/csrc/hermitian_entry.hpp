// The Hermitian operators' entry points across translation units, and the route each size takes.
#pragma once

#include <hip/hip_runtime.h>

#include "hermitian.hpp"
#include "ssspy_amd.h"

namespace ssspy {

// hermitian_rows.hip: a matrix on 8 lanes (6 x 6 .. 8 x 8)
bool hermitian_rows_wanted(int M, int always_from);
int eigh_rows(const void *A, double *lamb, void *V, long long n, int M, int mode, int floor_kind,
              double eps, hipStream_t st);
int sqrtmh_rows(const void *X, void *out, long long n, int M, int mode, int floor_kind, double eps,
                hipStream_t st);
int gmeanmh_rows(const void *A, const void *Bm, void *G, long long n, int M, int type,
                 hipStream_t st);
int eigh_general_rows(const void *A, const void *Bm, double *lamb, void *Z, long long n, int M,
                      int type, int *info, hipStream_t st);

// 9 x 9 .. 16 x 16: the size at run time (correct, not tuned)
inline bool hermitian_rt_wanted(int M) { return M > SSSPY_MAX_SOURCES && M <= SSSPY_RT_MAX_SOURCES; }

// The kernel family a size goes to, in the order the entry points have always asked.  An entry point
// without a closed 2 x 2 form or a packed kernel takes the lane-per-matrix kernel there, which also
// turns away the sizes nobody takes.
enum class HermRoute { RUNTIME, CLOSED2, ROWS8, PACKED6, LANE };
inline HermRoute hermitian_route(int M, bool closed2 = false, bool packed6 = false) {
  if (hermitian_rt_wanted(M)) return HermRoute::RUNTIME;
  if (closed2 && M == 2) return HermRoute::CLOSED2;
  if (hermitian_rows_wanted(M, 7)) return HermRoute::ROWS8;
  if (packed6 && M == 6) return HermRoute::PACKED6;
  return HermRoute::LANE;
}

// a lane's matrix: past the end it is the last one, worked on for the wave's votes and not stored --
// unless the descriptor's lanes leave there
struct HermLane {
  long long idx;
  bool live;
};
__device__ __forceinline__ HermLane herm_lane(long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  return HermLane{i < n ? i : n - 1, i < n};
}

// matrix idx of a batch (.., n, n), to and from the lane's flat copy
template <class D>
__device__ __forceinline__ void load_matrix(D d, c128 *dst, const c128 *__restrict__ src,
                                            long long idx) {
  const int nn = d.n() * d.n();
#pragma unroll D::unroll
  for (int e = 0; e < nn; ++e) dst[e] = src[idx * nn + e];
}
template <class D>
__device__ __forceinline__ void store_matrix(D d, c128 *dst, const c128 *src, long long idx) {
  const int nn = d.n() * d.n();
#pragma unroll D::unroll
  for (int e = 0; e < nn; ++e) dst[idx * nn + e] = src[e];
}

inline dim3 herm_lanes_grid(long long n) { return dim3((unsigned)((n + 63) / 64)); }

}  // namespace ssspy
