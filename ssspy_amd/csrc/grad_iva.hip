// Gradient and natural-gradient IVA (GradIVA / NaturalGradIVA and their Laplace / Gauss classes):
// the score weights and the per-bin step.  The score of the four named classes is phi_nj y_inj with
// one real weight per (source, frame), so mean_j phi y y^H of source n is W_i U_in W_i^H with the
// frame-weighted covariances U_in = mean_j phi_nj x_ij x_ij^H of the MIXTURE -- the two read-only
// passes of AuxIVA-IP1 (frame powers, weighted covariance) and the step below instead of IP1; the
// estimate itself is never formed.  ref: ssspy/bss/iva.py:764-818, :936-988, :2341-2973.
#include "common.hpp"
#include "rows_lu.hpp"
#include "rt_dense.hpp"

namespace ssspy {

// phi[b,n,j]: Laplace 1 / floor(r) (the floor on r itself, where the AuxIVA weight has it on 2 r),
// Gauss 1 / alpha with alpha = r^2 / n_bins written to `variance` (no floor: the reference has none),
// SSSPY_CONTRAST_GAUSS_FIXED 1 / variance with the variance as given
__global__ __launch_bounds__(256) void k_iva_score_weight(const double *__restrict__ r2,
                                                          double *weight, double *variance,
                                                          long long total, int F, int contrast,
                                                          int floor_kind, double eps) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const double p = r2[e];
  if (contrast == SSSPY_CONTRAST_GAUSS) {
    const double alpha = p / (double)F;
    variance[e] = alpha;
    weight[e] = 1.0 / alpha;
  } else if (contrast == SSSPY_CONTRAST_GAUSS_FIXED) {
    weight[e] = 1.0 / variance[e];
  } else {
    weight[e] = 1.0 / apply_floor(sqrt(p), floor_kind, eps);
  }
}

// ---- the step, a bin on G lanes (G = 2 for up to 2 sources, 4 up to 4, 8 up to 8): lane r owns row
// r of the filter, of P = mean_j phi(y) y^H and of everything derived from them, so no lane ever holds
// an N x N matrix and nothing leaves the registers.
//   row r of P: (w_r U_r) W^H from the covariances S (B, F, N, N, N), or row r of S (B, F, N, N)
//               itself when `ready` (the generic classes hand over mean_j phi(y) y^H)
//   D = P - I (holonomic) or offdiag(P)
//   NATURAL: W <- W - eta D W            (ssspy/bss/iva.py:969-983)
//   else:    W <- W - eta D W^-H         (:797-813): Z = D W^-H solves W Z^H = D^H; the LU of W with
//            partial pivoting is row-distributed as in k_ip1_rows (largest |re| + |im| among the rows
//            not yet used, the lowest row on ties), the N right-hand sides ride along; a zero pivot
//            bumps info[0]
//   LOGDET: log|det W| of the filters the step starts from (the sum of log|pivot|), one
//            share per workgroup at logdet[blockIdx.x * logdet_stride + b], the workgroup's bins added
//            in a fixed order -- no atomics, the same bits on every run.
//            Without it the natural-gradient form has no elimination at all.
// Lane groups past the last bin of a mixture load nothing (a neighbour group of the same workgroup
// rewrites that bin while they would read it): they run on an identity filter and zero statistics,
// so that every lane reaches the shuffles and the barrier, and store nothing.
// grid: (ceil(F / (256 / G)), B)
template <int N, int G, bool NATURAL, bool LOGDET>
__global__ __launch_bounds__(256) void k_grad_step_rows(c128 *W, const c128 *__restrict__ S,
                                                        int ready, int F, int holonomic, double eta,
                                                        int *info, double *logdet,
                                                        long long logdet_stride) {
  static_assert(G == 2 || G == 4 || G == 8, "group of 2, 4 or 8 lanes");
  static_assert(N <= G, "one lane per row");
  constexpr int BINS = 256 / G;
  __shared__ double scratch[4];
  const int r = threadIdx.x % G;  // my row
  const int b = blockIdx.y;
  const int i = blockIdx.x * BINS + threadIdx.x / G;
  const bool live = i < F;
  const long long id = (long long)b * F + (live ? i : F - 1);  // (idle groups: never dereferenced)
  const c128 zero = cmake(0.0, 0.0);
  const bool row = r < N;
  const int rr = row ? r : N - 1;
  c128 Wr[N], P[N], delta[N];
#pragma unroll
  for (int c = 0; c < N; ++c) {
    Wr[c] = live ? W[id * (N * N) + rr * N + c] : cmake(c == rr ? 1.0 : 0.0, 0.0);
    delta[c] = zero;
  }
  c128 t[N];  // w_r U_r
  if (ready) {
#pragma unroll
    for (int m = 0; m < N; ++m) P[m] = live ? S[id * (N * N) + rr * N + m] : zero;
  } else {
    const c128 *Un = S + (id * N + rr) * (N * N);
#pragma unroll
    for (int c = 0; c < N; ++c) t[c] = cmake(0.0, 0.0);
#pragma unroll
    for (int m = 0; m < N; ++m)
#pragma unroll
      for (int c = 0; c < N; ++c) cfma(t[c], Wr[m], live ? Un[m * N + c] : zero);
  }
  if (NATURAL || !ready) {
#pragma unroll
    for (int m = 0; m < N; ++m) {
      c128 wm[N];  // row m of W
#pragma unroll
      for (int c = 0; c < N; ++c) wm[c] = cmake(__shfl(Wr[c].x, m, G), __shfl(Wr[c].y, m, G));
      if (!ready) {
        c128 acc = cmake(0.0, 0.0);
        // (not cfmac: it adds the imaginary terms in the other order, different bits; fdica.hip has it)
#pragma unroll
        for (int c = 0; c < N; ++c) cfma(acc, t[c], cconj(wm[c]));
        P[m] = acc;
      }
      if (m == rr) P[m] = holonomic ? cmake(P[m].x - 1.0, P[m].y) : cmake(0.0, 0.0);
      if (NATURAL) {
#pragma unroll
        for (int c = 0; c < N; ++c) cfma(delta[c], P[m], wm[c]);
      }
    }
  } else {
#pragma unroll
    for (int m = 0; m < N; ++m)
      if (m == rr) P[m] = holonomic ? cmake(P[m].x - 1.0, P[m].y) : cmake(0.0, 0.0);
  }
  // from here on P holds row r of D
  double ld = 0.0;
  bool ok = true;
  if constexpr (!NATURAL || LOGDET) {
    c128 a[N], rhs[NATURAL ? 1 : N];
#pragma unroll
    for (int c = 0; c < N; ++c) a[c] = Wr[c];
    if constexpr (!NATURAL) {
      // row r of D^H: conj of column r of D, one element from every lane
#pragma unroll
      for (int c = 0; c < N; ++c) {
        rhs[c] = cmake(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const c128 v = cmake(__shfl(P[k].x, c, G), __shfl(P[k].y, c, G));  // D[c][k]
          if (k == rr) rhs[c] = cconj(v);
        }
      }
    }
    int order = row ? -1 : N;  // elimination step at which my row became the pivot row
    int plane[N];              // lane of the group that owns pivot k (uniform within the group)
    c128 pinv[N];              // 1 / pivot k, reused by the back substitution
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double bv = order < 0 ? cabs1(a[k]) : -1.0;
      int bl = r;
#pragma unroll
      for (int m = 1; m < G; m <<= 1) {
        const double ov = __shfl_xor(bv, m, G);
        const int ol = __shfl_xor(bl, m, G);
        const bool take = ov > bv || (ov == bv && ol < bl);
        bv = take ? ov : bv;
        bl = take ? ol : bl;
      }
      plane[k] = bl;
      if (r == bl) order = k;
      c128 prow[N], prhs[NATURAL ? 1 : N];
#pragma unroll
      for (int c = k; c < N; ++c) prow[c] = cmake(__shfl(a[c].x, bl, G), __shfl(a[c].y, bl, G));
      if constexpr (!NATURAL) {
#pragma unroll
        for (int c = 0; c < N; ++c)
          prhs[c] = cmake(__shfl(rhs[c].x, bl, G), __shfl(rhs[c].y, bl, G));
      }
      const c128 piv = prow[k];
      ok = ok && (piv.x != 0.0 || piv.y != 0.0);
      if constexpr (LOGDET) ld += 0.5 * log(cabs2(piv));
      pinv[k] = crecip(piv);
      if (order < 0) {  // still unused: eliminate column k
        const c128 f = cmul(a[k], pinv[k]);
#pragma unroll
        for (int c = k + 1; c < N; ++c) cfms(a[c], f, prow[c]);
        if constexpr (!NATURAL) {
#pragma unroll
          for (int c = 0; c < N; ++c) cfms(rhs[c], f, prhs[c]);
        }
      }
    }
    if constexpr (!NATURAL) {
#pragma unroll
      for (int k = N - 1; k >= 0; --k) {
        // row k of Z^H from the owner of pivot k, which has folded the rows above k in already;
        // Z[r][k] = conj(Z^H[k][r])
#pragma unroll
        for (int c = 0; c < N; ++c) {
          const c128 mine = cmul(rhs[c], pinv[k]);
          const c128 z = cmake(__shfl(mine.x, plane[k], G), __shfl(mine.y, plane[k], G));
          if (order < k) cfms(rhs[c], a[k], z);
          if (c == rr) delta[k] = cconj(z);
        }
      }
    }
  }
  if (live && row) {
#pragma unroll
    for (int c = 0; c < N; ++c)
      W[id * (N * N) + r * N + c] = cmake(Wr[c].x - eta * delta[c].x, Wr[c].y - eta * delta[c].y);
    if (!NATURAL && !ok && info && r == 0) atomicAdd(info, 1);
  }
  if constexpr (LOGDET) {  // (every thread reaches the barriers of block_sum)
    const double total = block_sum(live && r == 0 ? ld : 0.0, scratch);
    if (threadIdx.x == 0) logdet[(long long)blockIdx.x * logdet_stride + b] = total;
  }
}

// ---- the same step with the source count at run time (9..16 sources): a lane per bin, the matrices
// in the lane's private memory -- correct and simple, not tuned.  grid: (ceil(F / 64), B), one wave
__global__ __launch_bounds__(64) void k_grad_step_rt(c128 *W, const c128 *__restrict__ S, int ready,
                                                     int N, int F, int natural, int holonomic,
                                                     double eta, int *info, double *logdet,
                                                     long long logdet_stride) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 64 + threadIdx.x;
  const bool live = i < F;
  const long long id = (long long)b * F + (live ? i : F - 1);
  c128 Wm[RTN * RTN], A[RTN * RTN], D[RTN * RTN], t[RTN];
  // (lanes past the last bin load nothing and run on an identity filter and zero statistics)
  for (int e = 0; e < N * N; ++e)
    A[e] = Wm[e] = live ? W[id * (N * N) + e] : cmake(e / N == e % N ? 1.0 : 0.0, 0.0);
  for (int n = 0; n < N; ++n) {
    if (ready) {
      for (int m = 0; m < N; ++m)
        D[n * N + m] = live ? S[id * (N * N) + n * N + m] : cmake(0.0, 0.0);
    } else {
      const c128 *__restrict__ Un = S + (id * N + n) * (long long)(N * N);
      for (int c = 0; c < N; ++c) t[c] = cmake(0.0, 0.0);
      for (int m = 0; m < N; ++m)
        for (int c = 0; c < N; ++c)
          cfma(t[c], Wm[n * N + m], live ? Un[m * N + c] : cmake(0.0, 0.0));
      for (int m = 0; m < N; ++m) {
        c128 acc = cmake(0.0, 0.0);
        for (int c = 0; c < N; ++c) cfma(acc, t[c], cconj(Wm[m * N + c]));
        D[n * N + m] = acc;
      }
    }
    D[n * N + n] = holonomic ? cmake(D[n * N + n].x - 1.0, D[n * N + n].y) : cmake(0.0, 0.0);
  }
  double ld = 0.0;
  bool ok = true;
  if (natural) {
    if (logdet) ld = rt_logabsdet(A, N);
    for (int n = 0; n < N; ++n)
      for (int c = 0; c < N; ++c) {
        c128 acc = cmake(0.0, 0.0);
        for (int m = 0; m < N; ++m) cfma(acc, D[n * N + m], Wm[m * N + c]);
        A[n * N + c] = acc;
      }
  } else {
    // Z = D W^-H from W Z^H = D^H
    for (int n = 0; n < N; ++n) {
      D[n * N + n] = cconj(D[n * N + n]);
      for (int m = n + 1; m < N; ++m) {
        const c128 u = D[n * N + m];
        D[n * N + m] = cconj(D[m * N + n]);
        D[m * N + n] = cconj(u);
      }
    }
    ok = rt_lu_solve(A, D, N, N);
    for (int k = 0; k < N; ++k) ld += 0.5 * log(cabs2(A[k * N + k]));
    for (int n = 0; n < N; ++n)
      for (int c = 0; c < N; ++c) A[n * N + c] = cconj(D[c * N + n]);
  }
  if (live) {
    for (int e = 0; e < N * N; ++e)
      W[id * (N * N) + e] = cmake(Wm[e].x - eta * A[e].x, Wm[e].y - eta * A[e].y);
    if (!ok && info) atomicAdd(info, 1);
  }
  if (logdet) {
    const double total = wave_sum(live ? ld : 0.0);
    if (threadIdx.x == 0) logdet[(long long)blockIdx.x * logdet_stride + b] = total;
  }
}

static int grad_bins_per_block(int N) {
  if (N > SSSPY_MAX_SOURCES) return 64;
  return 256 / rows_group_of(N);
}

template <int N>
static int launch_grad_step(c128 *W, const c128 *S, int ready, int B, int F, int natural,
                            int holonomic, double eta, int *info, double *logdet,
                            long long logdet_stride, hipStream_t st) {
  constexpr int G = rows_group<N>();
  const dim3 grid((unsigned)((F + 256 / G - 1) / (256 / G)), (unsigned)B), block(256);
#define SSSPY_GRAD_STEP(NAT, LD)                                                                  \
  hipLaunchKernelGGL((k_grad_step_rows<N, G, NAT, LD>), grid, block, 0, st, W, S, ready, F,      \
                     holonomic, eta, info, logdet, logdet_stride)
  if (natural && logdet) SSSPY_GRAD_STEP(true, true);
  else if (natural) SSSPY_GRAD_STEP(true, false);
  else if (logdet) SSSPY_GRAD_STEP(false, true);
  else SSSPY_GRAD_STEP(false, false);
#undef SSSPY_GRAD_STEP
  return check_launch("k_grad_step_rows");
}

}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_iva_score_weight(const double *r2, double *weight, double *variance, int B, int N, int F,
                           int T, int contrast, int floor_kind, double floor_eps, void *stream) {
  SSSPY_REQUIRE(r2 && weight && B > 0 && N > 0 && F > 0 && T > 0, "iva_score_weight: bad argument");
  SSSPY_REQUIRE(contrast == SSSPY_CONTRAST_LAPLACE ||
                    ((contrast == SSSPY_CONTRAST_GAUSS || contrast == SSSPY_CONTRAST_GAUSS_FIXED) &&
                     variance),
                "iva_score_weight: bad contrast / variance");
  if (N > SSSPY_RT_MAX_SOURCES)
    return fail(SSSPY_ERR_UNSUPPORTED, "iva_score_weight: up to 16 sources");
  const long long total = (long long)B * N * T;
  hipLaunchKernelGGL(k_iva_score_weight, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     as_stream(stream), r2, weight, variance, total, F, contrast, floor_kind,
                     floor_eps);
  return check_launch("k_iva_score_weight");
}

int ssspy_iva_grad_step_logdet_slots(int B, int F, int N) {
  if (B <= 0 || F <= 0 || N < 1 || N > SSSPY_RT_MAX_SOURCES) return 0;
  const int bins = grad_bins_per_block(N);
  return (F + bins - 1) / bins;
}

int ssspy_iva_grad_step(void *W, const void *S, int stats_ready, int B, int F, int N, int natural,
                        int holonomic, double step_size, int *info, double *logdet,
                        long long logdet_stride, void *stream) {
  SSSPY_REQUIRE(W && S && W != S && B > 0 && B <= 65535 && F > 0 && N >= 1,
                "iva_grad_step: bad argument");
  SSSPY_REQUIRE(!logdet || logdet_stride >= B, "iva_grad_step: bad logdet stride");
  if (N > SSSPY_RT_MAX_SOURCES)
    return fail(SSSPY_ERR_UNSUPPORTED, "iva_grad_step: up to 16 sources");
  hipStream_t st = as_stream(stream);
  if (N > SSSPY_MAX_SOURCES) {
    hipLaunchKernelGGL(k_grad_step_rt, dim3((unsigned)((F + 63) / 64), (unsigned)B), dim3(64), 0, st,
                       (c128 *)W, (const c128 *)S, stats_ready ? 1 : 0, N, F, natural ? 1 : 0,
                       holonomic ? 1 : 0, step_size, info, logdet, logdet_stride);
    return check_launch("k_grad_step_rt");
  }
  DISPATCH_N(N, return launch_grad_step<NN>((c128 *)W, (const c128 *)S, stats_ready ? 1 : 0, B, F,
                                            natural ? 1 : 0, holonomic ? 1 : 0, step_size, info,
                                            logdet, logdet_stride, st));
  return SSSPY_OK;
}

}  // extern "C"
