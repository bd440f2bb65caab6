// What the passes of the primal-dual splitting separators share (pdsbss.hip, hva.hip): the thread
// count of a pass, the source-count dispatch and Z = dual_q + W2 x of one (bin, frame).
#pragma once

#include "common.hpp"

namespace ssspy {

constexpr int PDS_THREADS = 256;

// z_n = d_n + sum_m W2[n][m] x_m for the N rows of one (bin, frame); Wn: row-major N x N
template <int G, typename WPtr>
__device__ __forceinline__ void pds_form_z(c128 (&z)[G], const c128 *__restrict__ Xb,
                                           const c128 *Db, WPtr Wn, int N, long long FT, int j) {
  c128 x[G];
#pragma unroll
  for (int m = 0; m < G; ++m) x[m] = m < N ? Xb[m * FT + j] : cmake(0.0, 0.0);
#pragma unroll
  for (int n = 0; n < G; ++n) {
    z[n] = cmake(0.0, 0.0);
    if (n < N) {
      c128 y = cmake(0.0, 0.0);
#pragma unroll
      for (int m = 0; m < G; ++m)
        if (m < N) cfma(y, Wn[n * N + m], x[m]);
      z[n] = cadd(Db[n * FT + j], y);
    }
  }
}

static inline int pow2_group(int N) { return N <= 2 ? 2 : (N <= 4 ? 4 : (N <= 8 ? 8 : 16)); }

// G: the source count rounded up to a power of two
#define SSSPY_PDS_DISPATCH_G(N_, CALL)               \
  switch (::ssspy::pow2_group(N_)) {                 \
    case 2: { constexpr int GG = 2; CALL; } break;   \
    case 4: { constexpr int GG = 4; CALL; } break;   \
    case 8: { constexpr int GG = 8; CALL; } break;   \
    default: { constexpr int GG = 16; CALL; } break; \
  }

static inline bool pds_shape_ok(int B, int N, int F, int T) {
  return B > 0 && B <= 65535 && N >= 1 && N <= SSSPY_RT_MAX_SOURCES && F > 0 && T > 0;
}

}  // namespace ssspy
