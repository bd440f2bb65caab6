// OverIVA (R. Scheibler, N. Ono, "Independent vector analysis with more microphones than sources",
// WASPAA 2019): AuxIVA-IP1 with N <= M demixing rows; the other M - N rows of the full filter
// W = [W_t ; [J, -I]] are a Gaussian background fixed by the orthogonality constraint
// [J, -I] C W_t^H = 0, i.e. J = (E2 C W_t^H)(E1 C W_t^H)^-1 with C the covariance of the mixture.
//
// Two kernels.  k_overiva_frame_power applies the N x M filter and sums |y|^2 over the bins (the
// frame-power pass of iva_kernels.hip for a non-square filter, same slab fold: no fp64 atomics).
// k_overiva_step runs the N sequential IP1 row updates on the full M x M filter -- the arithmetic of
// k_ip1 / k_ip1_rt: A = W V_n, LU with partial pivoting on A w = e_n, d = floor(sqrt(max(Re w^H V_n w,
// 0))), row n <- conj(w) / d -- and re-forms J after each; on request it first leaves log|det W| and
// Re tr(U C U^H), U = [J, -I], of the filter as it comes in.  One lane per (mixture, bin): 2..5
// channels compiled per M with the matrices in registers (smallmat.hpp), 6..16 with M at run time and
// the matrices in the lane's private memory (rt_dense.hpp) -- the compiled form spills 34 VGPRs at 5
// channels and 452 at 6 (profiles/overiva_kernel_resources.txt).
//
// A solve counts as singular (info is bumped, the class raises LinAlgError) when a pivot is not above
// PIVOT_RTOL * size times the largest entry its column had before the elimination: two identical
// channels leave a pivot of rounding size there, not an exact zero.
#include "common.hpp"
#include "rt_dense.hpp"
#include "smallmat.hpp"
#include "ssspy_amd.h"

namespace ssspy {

// channels up to which k_overiva_step<M> is used (-DSSSPY_OVERIVA_COMPILED_MAX=8 builds the forms
// the resource profile rejects, for that profile)
#ifndef SSSPY_OVERIVA_COMPILED_MAX
#define SSSPY_OVERIVA_COMPILED_MAX 5
#endif
constexpr double PIVOT_RTOL = 16.0 * 2.220446049250313e-16;

// ------------------------------------------------------------------------------- frame power
// A thread per frame, the filter rows wave-uniform.  grid: (ceil(T / 256), bin chunks, B); chunk c
// stores its sums to slab c of `dst` ((chunks, B, N, T); r2 itself with one chunk) and
// launch_fold_slabs adds the slabs in chunk order.  Wt: the N x M rows of bin (b, i) start at
// Wt + (b F + i) w_stride.  Y (B, N, F, T) or NULL.
template <int M>
__global__ __launch_bounds__(256) void k_overiva_frame_power(const c128 *__restrict__ X,
                                                             const c128 *__restrict__ Wt,
                                                             long long w_stride, c128 *Y,
                                                             double *dst, int N, int F, int T,
                                                             int bins_per_chunk) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.z;
  const int i_begin = blockIdx.y * bins_per_chunk;
  const int i_end = min(F, i_begin + bins_per_chunk);
  if (j >= T) return;
  double acc[M];
#pragma unroll
  for (int n = 0; n < M; ++n) acc[n] = 0.0;
  for (int i = i_begin; i < i_end; ++i) {
    c128 x[M];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = X[(((long long)b * M + m) * F + i) * T + j];
    const c128 *Wi = Wt + ((long long)b * F + i) * w_stride;
#pragma unroll
    for (int n = 0; n < M; ++n) {
      if (n < N) {  // (uniform)
        c128 y = cmake(0.0, 0.0);
#pragma unroll
        for (int m = 0; m < M; ++m) cfma(y, Wi[n * M + m], x[m]);
        acc[n] += cabs2(y);
        if (Y) Y[(((long long)b * N + n) * F + i) * T + j] = y;
      }
    }
  }
  double *slab = dst + (long long)blockIdx.y * gridDim.z * N * T;
#pragma unroll
  for (int n = 0; n < M; ++n)
    if (n < N) slab[((long long)b * N + n) * T + j] = acc[n];
}

// ------------------------------------------------------------------------------- step, compiled M
template <int M, int R>
__device__ __forceinline__ bool lu_solve_checked(Mat<M> &A, c128 (&rhs)[M][R]) {
  double cm[M];
#pragma unroll
  for (int c = 0; c < M; ++c) {
    cm[c] = 0.0;
#pragma unroll
    for (int r = 0; r < M; ++r) cm[c] = fmax(cm[c], cabs1(A.a[r][c]));
  }
  lu_forward<M, R>(A, rhs);
  bool ok = true;
#pragma unroll
  for (int k = 0; k < M; ++k) ok = ok && (cabs1(A.a[k][k]) > PIVOT_RTOL * M * cm[k]);
  lu_backward<M, R>(A, rhs);
  return ok;
}

// Rows N..M-1 of W <- [J, -I] with J = (E2 P)(E1 P)^-1, P = C W_t^H (M x N).  The transposed system
// (E1 P)^T J^T = (E2 P)^T is solved padded to M x M (identity in the rows / columns from N on, the
// right-hand side of background row k in column k), so that every index is static.
template <int M>
__device__ __forceinline__ bool refresh_background(Mat<M> &Wm, const Mat<M> &Cm, int N) {
  Mat<M> At;
  c128 rhs[M][M];
#pragma unroll
  for (int r = 0; r < M; ++r)
#pragma unroll
    for (int n = 0; n < M; ++n) {
      c128 p = cmake(0.0, 0.0);
#pragma unroll
      for (int m = 0; m < M; ++m) cfmac(p, Cm.a[r][m], Wm.a[n][m]);
      const bool src = n < N;
      At.a[n][r] = (src && r < N) ? p : cmake(n == r ? 1.0 : 0.0, 0.0);
      rhs[n][r] = (src && r >= N) ? p : cmake(0.0, 0.0);
    }
  const bool ok = lu_solve_checked<M, M>(At, rhs);
#pragma unroll
  for (int k = 0; k < M; ++k)
#pragma unroll
    for (int c = 0; c < M; ++c)
      if (k >= N) Wm.a[k][c] = c < N ? rhs[c][k] : cmake(c == k ? -1.0 : 0.0, 0.0);
  return ok;
}

// terms (nbins, 2) or NULL: log|det W| and Re tr(U C U^H) of the filter as it comes in.
// V (nbins, N, M, M) or NULL (no row updates; J is re-formed when `refresh`).
template <int M>
__global__ __launch_bounds__(64) void k_overiva_step(c128 *W, const c128 *__restrict__ V,
                                                     const c128 *__restrict__ C, long long nbins,
                                                     int N, int floor_kind, double eps, int *info,
                                                     double *terms, int refresh) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nbins) return;
  Mat<M> Wm, Cm;
  load_mat<M>(Wm, W + idx * (M * M));
  load_mat<M>(Cm, C + idx * (M * M));
  if (terms) {
    Mat<M> A = Wm;
    terms[idx * 2] = logabsdet<M>(A);
    double tr = 0.0;
#pragma unroll
    for (int r = 0; r < M; ++r) {
      c128 u[M];
#pragma unroll
      for (int c = 0; c < M; ++c) u[c] = cconj(Wm.a[r][c]);
      const double q = quad_form<M>(u, Cm);
      tr += r >= N ? q : 0.0;
    }
    terms[idx * 2 + 1] = tr;
  }
  bool ok = true;
  if (V) {
#pragma unroll 1
    for (int n = 0; n < N; ++n) {
      Mat<M> Un, A;
      load_mat<M>(Un, V + (idx * N + n) * (M * M));
      matmul<M>(A, Wm, Un);
      c128 rhs[M][1];
#pragma unroll
      for (int r = 0; r < M; ++r) rhs[r][0] = cmake(r == n ? 1.0 : 0.0, 0.0);
      ok = lu_solve_checked<M, 1>(A, rhs) && ok;
      c128 w[M];
#pragma unroll
      for (int r = 0; r < M; ++r) w[r] = rhs[r][0];
      double qf = quad_form<M>(w, Un);
      qf = qf < 0.0 ? 0.0 : qf;  // np.maximum(., 0): NaN propagates
      const double d = apply_floor(sqrt(qf), floor_kind, eps);
#pragma unroll
      for (int r = 0; r < M; ++r)
#pragma unroll
        for (int c = 0; c < M; ++c)
          if (r == n) Wm.a[r][c] = cmake(w[c].x / d, -w[c].y / d);
      if (N < M) ok = refresh_background<M>(Wm, Cm, N) && ok;
    }
  } else if (refresh && N < M) {
    ok = refresh_background<M>(Wm, Cm, N);
  }
  if (V || refresh) store_mat<M>(Wm, W + idx * (M * M));
  if (!ok && info) atomicAdd(info, 1);
}

// ------------------------------------------------------------------------------- step, run-time M
// the pivots rt_lu_solve left on the diagonal of A (n x n) against the column maxima taken before
__device__ inline bool rt_pivots_ok(const c128 *A, const double *cm, int n) {
  bool ok = true;
  for (int k = 0; k < n; ++k) ok = ok && (cabs1(A[k * n + k]) > PIVOT_RTOL * n * cm[k]);
  return ok;
}
__device__ inline void rt_column_max(const c128 *A, double *cm, int n) {
  for (int c = 0; c < n; ++c) {
    double v = 0.0;
    for (int r = 0; r < n; ++r) v = fmax(v, cabs1(A[r * n + c]));
    cm[c] = v;
  }
}

// the same as refresh_background<M> without the padding: A (N x N) = (E1 P)^T, Z (N x (M - N)) =
// (E2 P)^T, both in the caller's private memory
__device__ inline bool rt_refresh_background(c128 *Wm, const c128 *__restrict__ Cm, int M, int N,
                                             c128 *A, c128 *Z, double *cm) {
  const int R = M - N;
  for (int r = 0; r < M; ++r)
    for (int n = 0; n < N; ++n) {
      c128 p = cmake(0.0, 0.0);
      for (int m = 0; m < M; ++m) cfmac(p, Cm[r * M + m], Wm[n * M + m]);
      if (r < N) A[n * N + r] = p;
      else Z[n * R + (r - N)] = p;
    }
  rt_column_max(A, cm, N);
  rt_lu_solve(A, Z, N, R);
  const bool ok = rt_pivots_ok(A, cm, N);
  for (int j = 0; j < R; ++j)
    for (int c = 0; c < M; ++c)
      Wm[(N + j) * M + c] = c < N ? Z[c * R + j] : cmake(c == N + j ? -1.0 : 0.0, 0.0);
  return ok;
}

__global__ __launch_bounds__(64) void k_overiva_step_rt(c128 *W, const c128 *__restrict__ V,
                                                        const c128 *__restrict__ C, long long nbins,
                                                        int M, int N, int floor_kind, double eps,
                                                        int *info, double *terms, int refresh) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nbins) return;
  c128 Wm[RTN * RTN], A[RTN * RTN], Z[RTN * RTN], w[RTN];
  double cm[RTN];
  const c128 *__restrict__ Cm = C + idx * (long long)(M * M);
  for (int e = 0; e < M * M; ++e) Wm[e] = W[idx * (M * M) + e];
  if (terms) {
    for (int e = 0; e < M * M; ++e) A[e] = Wm[e];
    terms[idx * 2] = rt_logabsdet(A, M);
    double tr = 0.0;
    for (int r = N; r < M; ++r) {
      for (int c = 0; c < M; ++c) w[c] = cconj(Wm[r * M + c]);
      tr += rt_quad(w, Cm, M);
    }
    terms[idx * 2 + 1] = tr;
  }
  bool ok = true;
  if (V) {
    for (int n = 0; n < N; ++n) {
      const c128 *__restrict__ Un = V + (idx * N + n) * (long long)(M * M);
      for (int r = 0; r < M; ++r)
        for (int c = 0; c < M; ++c) {
          c128 acc = cmake(0.0, 0.0);
          for (int k = 0; k < M; ++k) cfma(acc, Wm[r * M + k], Un[k * M + c]);
          A[r * M + c] = acc;
        }
      rt_column_max(A, cm, M);
      for (int r = 0; r < M; ++r) w[r] = cmake(r == n ? 1.0 : 0.0, 0.0);
      rt_lu_solve(A, w, M, 1);
      ok = rt_pivots_ok(A, cm, M) && ok;
      double qf = rt_quad(w, Un, M);
      qf = qf < 0.0 ? 0.0 : qf;  // np.maximum(., 0): NaN propagates
      const double d = apply_floor(sqrt(qf), floor_kind, eps);
      for (int c = 0; c < M; ++c) Wm[n * M + c] = cmake(w[c].x / d, -w[c].y / d);
      if (N < M) ok = rt_refresh_background(Wm, Cm, M, N, A, Z, cm) && ok;
    }
  } else if (refresh && N < M) {
    ok = rt_refresh_background(Wm, Cm, M, N, A, Z, cm);
  }
  if (V || refresh)
    for (int e = 0; e < M * M; ++e) W[idx * (M * M) + e] = Wm[e];
  if (!ok && info) atomicAdd(info, 1);
}

// out[b] = sum_i terms[(b F + i) 2 + which]: one block per mixture, thread t adds bins t, t + 256, ...
// in order and the block folds in a fixed tree -- the same bits on every run
__global__ __launch_bounds__(256) void k_overiva_fold_terms(const double *__restrict__ terms,
                                                            double *logdet, double *trace, int F) {
  __shared__ double scratch[8];
  const int b = blockIdx.x;
  double ld = 0.0, tr = 0.0;
  for (int i = threadIdx.x; i < F; i += blockDim.x) {
    ld += terms[((long long)b * F + i) * 2];
    tr += terms[((long long)b * F + i) * 2 + 1];
  }
  const double lds = block_sum(ld, scratch);
  const double trs = block_sum(tr, scratch + 4);
  if (threadIdx.x == 0) {
    logdet[b] = lds;
    trace[b] = trs;
  }
}

}  // namespace ssspy

using namespace ssspy;

extern "C" {

static bool overiva_shape_ok(int M, int N) {
  return M >= 2 && M <= SSSPY_RT_MAX_SOURCES && N >= 1 && N <= M;
}

struct OverFramePlan {
  int bins_per_chunk, chunks;
};
// enough (frame tile, chunk, mixture) blocks to fill the chip, at most 128 slabs for the fold
static OverFramePlan overiva_frame_plan(int B, int F, int T) {
  const long long gx = (T + 255) / 256;
  long long want = 2048 / (gx * B);
  if (want < 1) want = 1;
  if (want > 128) want = 128;
  if (want > F) want = F;
  OverFramePlan p;
  p.bins_per_chunk = (int)((F + want - 1) / want);
  p.chunks = (F + p.bins_per_chunk - 1) / p.bins_per_chunk;
  return p;
}

size_t ssspy_overiva_frame_power_workspace_bytes(int B, int N, int F, int T) {
  if (B <= 0 || N <= 0 || F <= 0 || T <= 0) return 0;
  const OverFramePlan p = overiva_frame_plan(B, F, T);
  if (p.chunks <= 1) return 0;
  const long long total = (long long)B * N * T;
  return (size_t)p.chunks * total * sizeof(double) + fold_scratch_bytes(total, p.chunks);
}

#define OVERIVA_DISPATCH_M(M_, CALL)                                                       \
  switch (M_) {                                                                            \
    case 2: { constexpr int MM = 2; CALL; } break;                                         \
    case 3: { constexpr int MM = 3; CALL; } break;                                         \
    case 4: { constexpr int MM = 4; CALL; } break;                                         \
    case 5: { constexpr int MM = 5; CALL; } break;                                         \
    case 6: { constexpr int MM = 6; CALL; } break;                                         \
    case 7: { constexpr int MM = 7; CALL; } break;                                         \
    case 8: { constexpr int MM = 8; CALL; } break;                                         \
    case 9: { constexpr int MM = 9; CALL; } break;                                         \
    case 10: { constexpr int MM = 10; CALL; } break;                                       \
    case 11: { constexpr int MM = 11; CALL; } break;                                       \
    case 12: { constexpr int MM = 12; CALL; } break;                                       \
    case 13: { constexpr int MM = 13; CALL; } break;                                       \
    case 14: { constexpr int MM = 14; CALL; } break;                                       \
    case 15: { constexpr int MM = 15; CALL; } break;                                       \
    case 16: { constexpr int MM = 16; CALL; } break;                                       \
    default: return ::ssspy::fail(SSSPY_ERR_UNSUPPORTED, "overiva: 2..16 channels");       \
  }

int ssspy_overiva_frame_power(const void *X, const void *Wt, long long w_stride, void *Y, double *r2,
                              int B, int M, int N, int F, int T, void *workspace,
                              size_t workspace_bytes, void *stream) {
  SSSPY_REQUIRE(X && Wt && r2 && B > 0 && F > 0 && T > 0, "overiva_frame_power: bad argument");
  if (!overiva_shape_ok(M, N))
    return fail(SSSPY_ERR_UNSUPPORTED, "overiva_frame_power: 2..16 channels, 1..n_channels sources");
  SSSPY_REQUIRE(w_stride >= (long long)N * M, "overiva_frame_power: filter stride below N * M");
  hipStream_t st = as_stream(stream);
  const OverFramePlan p = overiva_frame_plan(B, F, T);
  const size_t need = ssspy_overiva_frame_power_workspace_bytes(B, N, F, T);
  SSSPY_REQUIRE(need == 0 || (workspace && workspace_bytes >= need),
                "overiva_frame_power: workspace too small");
  double *dst = p.chunks > 1 ? (double *)workspace : r2;
  dim3 grid((T + 255) / 256, p.chunks, B), block(256);
  OVERIVA_DISPATCH_M(M, hipLaunchKernelGGL((k_overiva_frame_power<MM>), grid, block, 0, st,
                                           (const c128 *)X, (const c128 *)Wt, w_stride, (c128 *)Y,
                                           dst, N, F, T, p.bins_per_chunk));
  int rc = check_launch("k_overiva_frame_power");
  if (rc || p.chunks == 1) return rc;
  const long long total = (long long)B * N * T;
  return launch_fold_slabs((const double *)workspace,
                           (char *)workspace + (size_t)p.chunks * total * sizeof(double), r2, total,
                           p.chunks, st);
}

size_t ssspy_overiva_step_workspace_bytes(int B, int F) {
  if (B <= 0 || F <= 0) return 0;
  return (size_t)B * F * 2 * sizeof(double);
}

int ssspy_overiva_step(void *W, const void *V, const void *C, int B, int F, int M, int N,
                       int floor_kind, double floor_eps, int *info, double *logdet, double *trace,
                       void *workspace, size_t workspace_bytes, void *stream) {
  SSSPY_REQUIRE(W && C && B > 0 && F > 0, "overiva_step: bad argument");
  if (!overiva_shape_ok(M, N))
    return fail(SSSPY_ERR_UNSUPPORTED, "overiva_step: 2..16 channels, 1..n_channels sources");
  SSSPY_REQUIRE((logdet == nullptr) == (trace == nullptr),
                "overiva_step: logdet and trace go together");
  SSSPY_REQUIRE(!logdet || (workspace && workspace_bytes >= ssspy_overiva_step_workspace_bytes(B, F)),
                "overiva_step: workspace too small");
  hipStream_t st = as_stream(stream);
  double *terms = logdet ? (double *)workspace : nullptr;
  const int refresh = !V && !logdet;
  const long long nbins = (long long)B * F;
  dim3 grid((unsigned)((nbins + 63) / 64)), block(64);
#define OVERIVA_STEP_CASE(MM)                                                                   \
  case MM:                                                                                      \
    hipLaunchKernelGGL((k_overiva_step<MM>), grid, block, 0, st, (c128 *)W, (const c128 *)V,    \
                       (const c128 *)C, nbins, N, floor_kind, floor_eps, info, terms, refresh); \
    break;
  switch (M) {
    OVERIVA_STEP_CASE(2)
    OVERIVA_STEP_CASE(3)
    OVERIVA_STEP_CASE(4)
    OVERIVA_STEP_CASE(5)
#if SSSPY_OVERIVA_COMPILED_MAX >= 8
    OVERIVA_STEP_CASE(6)
    OVERIVA_STEP_CASE(7)
    OVERIVA_STEP_CASE(8)
#endif
    default:
      hipLaunchKernelGGL(k_overiva_step_rt, grid, block, 0, st, (c128 *)W, (const c128 *)V,
                         (const c128 *)C, nbins, M, N, floor_kind, floor_eps, info, terms, refresh);
  }
#undef OVERIVA_STEP_CASE
  int rc = check_launch("k_overiva_step");
  if (rc || !logdet) return rc;
  hipLaunchKernelGGL(k_overiva_fold_terms, dim3(B), dim3(256), 0, st, (const double *)terms, logdet,
                     trace, F);
  return check_launch("k_overiva_fold_terms");
}

}  // extern "C"
