// What the row-distributed kernels share: a bin on G lanes, lane r owns row r of a matrix and of its
// right-hand sides, so no lane ever holds an N x N matrix and nothing leaves the registers.
//   k_ip1_rows (spatial_kernels.hip), k_ip1_small (ilrma_small.hip)   A w = e_n        crecip_fast
//   k_ip2_rows (pairwise_kernels.hip)                                 A P = (e_m e_n)  crecip_fast
//   k_grad_step_rows (grad_iva.hip), k_fdica_steps (fdica.hip)        W Z^H = D^H, log|det W|,
//                                                                     A w = e_n        crecip (Smith)
// The LU solve itself is still written out at each of the five sites.  One shared text would have
// changed BITS: f = a[k] * pinv[k] and rhs * pinv[k] go through cmul, whose sums the compiler
// contracts around the first or the second product as it sees fit, differently at the five sites
// (measured, profiles/rows_lu_bits.txt).
#pragma once

#include "common.hpp"

namespace ssspy {

// lanes per bin of n <= 8 rows (the host asks at run time, the kernels at compile time)
constexpr int rows_group_of(int n) { return n <= 2 ? 2 : (n <= 4 ? 4 : 8); }
template <int N>
constexpr int rows_group() {
  return rows_group_of(N);
}

__device__ __forceinline__ c128 shfl_c(c128 v, int src, int width) {
  return cmake(__shfl(v.x, src, width), __shfl(v.y, src, width));
}

}  // namespace ssspy
