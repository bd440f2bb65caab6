// Device forms of the small public helpers of ssspy.special and ssspy.linalg that take torch device
// tensors (the convention of permutation alignment: NumPy stays on the host, tensors stay on the
// device):
//   softmax, logsumexp over one axis of a float64 tensor   (ssspy/special/softmax.py, logsumexp.py)
//   quadratic forms x^H A x of complex128 vectors          (ssspy/linalg/quadratic.py)
// A tensor reduced over one axis is addressed as (outer, len, inner), contiguous: element k of row
// (o, i) sits at (o * len + k) * inner + i, so an axis that is not the last is walked by its stride
// and nothing is transposed.  One wave owns a row: lane l takes elements l, l + 64, ... in order,
// then the 64 partial results meet in the xor butterfly of wave_sum -- a fixed order, the same bits
// on every run.  The maximum is subtracted before exp, as in the reference.  fp64, no atomics.
#include "common.hpp"
#include "ssspy_amd.h"

namespace ssspy {

namespace {

constexpr int ROWS_PER_BLOCK = 4;  // waves of a 256-thread workgroup, a row each

// numpy.max: the larger of the two, NaN if either is
__device__ __forceinline__ double max_nan(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ double wave_max_nan(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max_nan(v, __shfl_xor(v, off, 64));
  return v;
}

// mode 0: out (outer, len, inner) = exp(x - max) / sum exp(x - max)
// mode 1: out (outer, inner) = log(sum exp(x - max)) + max
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void k_softmax_rows(const double *__restrict__ X,
                                                                      double *out, long long rows,
                                                                      int len, long long inner,
                                                                      int mode) {
  const long long row = (long long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= rows) return;  // (a whole wave leaves: the shuffles below see full waves only)
  const int lane = threadIdx.x & 63;
  const long long o = row / inner, i = row - o * inner;
  const double *x = X + o * len * inner + i;
  double m = -INFINITY;
  for (int k = lane; k < len; k += 64) m = max_nan(m, x[(long long)k * inner]);
  m = wave_max_nan(m);
  double s = 0.0;
  for (int k = lane; k < len; k += 64) s += exp(x[(long long)k * inner] - m);
  s = wave_sum(s);
  if (mode == 1) {
    if (lane == 0) out[row] = log(s) + m;
    return;
  }
  double *y = out + o * len * inner + i;
  for (int k = lane; k < len; k += 64) y[(long long)k * inner] = exp(x[(long long)k * inner] - m) / s;
}

// out[i] = (x^H A) x: the row vector first, as the reference's matmul chain.  A lane per form.
__global__ __launch_bounds__(64) void k_quadratic(const c128 *__restrict__ X,
                                                  const c128 *__restrict__ A, c128 *out,
                                                  long long n, int N) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const c128 *x = X + i * N;
  const c128 *a = A + i * N * N;
  c128 acc = cmake(0.0, 0.0);
  for (int c = 0; c < N; ++c) {
    c128 t = cmake(0.0, 0.0);
    for (int r = 0; r < N; ++r) cfma(t, cconj(x[r]), a[r * N + c]);
    cfma(acc, t, x[c]);
  }
  out[i] = acc;
}

int launch_rows(const double *X, double *out, long long outer, int len, long long inner, int mode,
                const char *what, hipStream_t st) {
  SSSPY_REQUIRE(X && out && outer > 0 && len > 0 && inner > 0, "softmax / logsumexp: bad argument");
  SSSPY_REQUIRE(outer <= (1LL << 40) / inner, "softmax / logsumexp: too many rows");
  const long long rows = outer * inner;
  const long long blocks = (rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  SSSPY_REQUIRE(blocks < 2147483647LL, "softmax / logsumexp: too many rows");
  hipLaunchKernelGGL(k_softmax_rows, dim3((unsigned)blocks), dim3(64 * ROWS_PER_BLOCK), 0, st, X, out,
                     rows, len, inner, mode);
  return check_launch(what);
}

}  // namespace

}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_softmax(const double *X, double *out, long long outer, int len, long long inner,
                  void *stream) {
  return launch_rows(X, out, outer, len, inner, 0, "k_softmax_rows", as_stream(stream));
}

int ssspy_logsumexp(const double *X, double *out, long long outer, int len, long long inner,
                    void *stream) {
  return launch_rows(X, out, outer, len, inner, 1, "k_softmax_rows (logsumexp)", as_stream(stream));
}

int ssspy_quadratic(const void *X, const void *A, void *out, long long n, int N, void *stream) {
  SSSPY_REQUIRE(X && A && out && n > 0, "quadratic: bad argument");
  SSSPY_REQUIRE(n < 64LL * 2147483647LL, "quadratic: n out of range");
  if (N < 1 || N > SSSPY_RT_MAX_SOURCES)
    return fail(SSSPY_ERR_UNSUPPORTED, "quadratic takes vectors of 1 to 16 entries");
  hipLaunchKernelGGL(k_quadratic, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, as_stream(stream),
                     (const c128 *)X, (const c128 *)A, (c128 *)out, n, N);
  return check_launch("k_quadratic");
}

}  // extern "C"
