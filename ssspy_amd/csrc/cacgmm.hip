// cACGMM (complex angular central Gaussian mixture model): the EM iteration of CACGMM.
//   E step  gamma_nij  = softmax_n(log alpha_in - log det B_in - M log q_nij),
//                        q_nij = floor(max(Re z_ij^H B_in^-1 z_ij, 0))
//   M step  alpha_in   = sum_j gamma_nij / T
//           B_in       = to_psd(M sum_j (gamma_nij / q_nij) z_ij z_ij^H / sum_j gamma_nij)
// Both steps evaluate q with the SAME B, so one pass over the unit mixture Z serves an iteration:
// k_cacgmm_pass leaves sum_j gamma, sum_j (gamma / q) z z^H and sum_j logsumexp_n (the loss of the
// parameters it was given) per (mixture, bin); the posterior goes to HBM only when asked for.
// ref: ssspy/bss/cacgmm.py:116-156 (unit input), :561-601, :629-738.
#include "common.hpp"
#include "herm_packed.hpp"
#include "ssspy_amd.h"

namespace ssspy {

constexpr int CACGMM_MAX_SOURCES = 16;
constexpr int CACGMM_THREADS = 256;

// Z = X / floor(||x||_2) per (bin, frame); X, Z (B, M, F, T).  grid: (ceil(F T / 256), B)
__global__ __launch_bounds__(256) void k_cacgmm_unit(const c128 *__restrict__ X, c128 *Z, int M,
                                                     long long FT, int floor_kind, double eps) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= FT) return;
  const long long base = (long long)blockIdx.y * M * FT + e;
  double s = 0.0;
  for (int m = 0; m < M; ++m) {
    const c128 x = X[base + m * FT];
    s += x.x * x.x + x.y * x.y;
  }
  const double d = apply_floor(sqrt(s), floor_kind, eps);
  for (int m = 0; m < M; ++m) {
    const c128 x = X[base + m * FT];
    Z[base + m * FT] = cmake(x.x / d, x.y / d);
  }
}

// LDS of the pass, in doubles: the frame tile of Z (t-major, rows padded to an odd number of c128 so
// that lanes on consecutive frames and lanes on consecutive channels both spread over the banks),
// the weights gamma / q of the tile (t-major, padded likewise), the N packed inverses, the N
// log alpha - log det B, and the slots of the closing reductions.
__host__ __device__ inline int cacgmm_zs(int M) { return M | 1; }
__host__ __device__ inline int cacgmm_ws(int N) { return N | 1; }
static inline size_t cacgmm_pass_lds(int M, int N, int tile) {
  const size_t mm = ((size_t)N * M * M + 1) & ~(size_t)1;
  return ((size_t)tile * cacgmm_zs(M) * 2 + (size_t)tile * cacgmm_ws(N) + mm + CACGMM_MAX_SOURCES +
          4 * (CACGMM_MAX_SOURCES + 1)) * sizeof(double);
}

// One workgroup per (bin, mixture) walks the frames in tiles of `tile` (<= 256).
//   phase 1: lane = frame.  z in registers (and to LDS), the N quadratic forms against the packed
//            inverses staged in LDS (every lane reads the same word: a broadcast), the softmax over
//            n in registers (the loop over n is unrolled to 16 and cut by the uniform n < N).
//   phase 2: lane = (row a of source n, frame group g): sum_t w_nt z_at conj(z_ct) for the M columns c
//            of its row, over the frames t = g, g + G, .. of the tile, G = 256 / (N M) groups; the
//            accumulators stay in registers across the tiles.
//   end:     the G groups are added in group order through LDS, the per-lane sum_t gamma and
//            sum_t logsumexp across the wave by shuffles and across the four waves in wave order.
// Every sum has a fixed order: no atomics, the same bits on every run.  Lanes past the last frame
// load nothing and contribute zero weights.
// binv (B, N, F, M^2) packed [M diagonal][re, im of the upper triangle, row-major], logp (B, N, F).
// sum_gamma (B, N, F), num (B, N, F, M, M) (both or neither), loss (B, F) = -sum_t lse / T, gamma
// (B, N, F, T): each may be NULL.  gamma_in (may be NULL): posteriors to take for the sums instead of
// the softmax of this pass (CACGMM.update_parameters after the posterior was assigned by hand).
template <int M>
__global__ __launch_bounds__(256) void k_cacgmm_pass(const c128 *__restrict__ Z,
                                                     const double *__restrict__ binv,
                                                     const double *__restrict__ logp, int N, int F,
                                                     int T, int tile, int floor_kind, double eps,
                                                     double *sum_gamma, c128 *num, double *loss,
                                                     double *gamma,
                                                     const double *__restrict__ gamma_in) {
  constexpr int MM = M * M;
  constexpr int NMAX = CACGMM_MAX_SOURCES;
  constexpr int ZS = M | 1;
  extern __shared__ double smem[];
  const int WS = N | 1;
  c128 *sZ = reinterpret_cast<c128 *>(smem);
  double *sW = smem + (size_t)tile * ZS * 2;
  double *sB = sW + (size_t)tile * WS;
  double *sLp = sB + (((size_t)N * MM + 1) & ~(size_t)1);
  double *sRed = sLp + NMAX;

  const int tid = threadIdx.x;
  const int f = blockIdx.x, b = blockIdx.y;
  const bool stats = num != nullptr;

  for (int e = tid; e < N * MM; e += CACGMM_THREADS) {
    const int n = e / MM;
    sB[e] = binv[(((long long)b * N + n) * F + f) * MM + (e - n * MM)];
  }
  if (tid < N) sLp[tid] = logp[((long long)b * N + tid) * F + f];

  // phase-2 role
  const int rows = N * M;
  const int G = CACGMM_THREADS / rows;
  const int g = tid / rows, r = tid - g * rows;
  const int rn = r / M, ra = r - rn * M;
  const bool worker = stats && g < G;
  c128 acc[M];
#pragma unroll
  for (int c = 0; c < M; ++c) acc[c] = cmake(0.0, 0.0);

  double sg[NMAX];
#pragma unroll
  for (int n = 0; n < NMAX; ++n) sg[n] = 0.0;
  double lse_acc = 0.0;
  __syncthreads();

  for (int t0 = 0; t0 < T; t0 += tile) {
    const int t = t0 + tid;
    const bool live = tid < tile && t < T;
    if (tid < tile) {
      c128 z[M];
#pragma unroll
      for (int a = 0; a < M; ++a) {
        z[a] = live ? Z[(((long long)b * M + a) * F + f) * T + t] : cmake(0.0, 0.0);
        if (stats) sZ[tid * ZS + a] = z[a];
      }
      double lg[NMAX], qv[NMAX];
      double vmax = 0.0;
#pragma unroll
      for (int n = 0; n < NMAX; ++n) {
        lg[n] = 0.0;
        qv[n] = 1.0;
        if (n < N) {
          const double *H = sB + n * MM;
          double q = 0.0, cross = 0.0;
#pragma unroll
          for (int a = 0; a < M; ++a) {
            q = fma(H[a], cabs2(z[a]), q);
            c128 u = cmake(0.0, 0.0);  // sum_{c > a} H_ac z_c
#pragma unroll
            for (int c = a + 1; c < M; ++c) {
              const int e = M + 2 * tri<M>(a, c);
              cfma(u, cmake(H[e], H[e + 1]), z[c]);
            }
            cross = fma(z[a].x, u.x, cross);
            cross = fma(z[a].y, u.y, cross);
          }
          q = fma(2.0, cross, q);
          q = q > 0.0 ? q : (q != q ? q : 0.0);  // numpy.maximum(q, 0): NaN stays
          q = apply_floor(q, floor_kind, eps);
          qv[n] = q;
          lg[n] = sLp[n] - (double)M * log(q);
          vmax = (n == 0 || lg[n] > vmax) ? lg[n] : vmax;
        }
      }
      double s = 0.0;
#pragma unroll
      for (int n = 0; n < NMAX; ++n)
        if (n < N) {
          lg[n] = exp(lg[n] - vmax);
          s += lg[n];
        }
      if (live) lse_acc += log(s) + vmax;
#pragma unroll
      for (int n = 0; n < NMAX; ++n)
        if (n < N) {
          const long long ge = (((long long)b * N + n) * F + f) * T + t;
          const double gm = live ? (gamma_in ? gamma_in[ge] : lg[n] / s) : 0.0;
          sg[n] += gm;
          if (gamma && live) gamma[ge] = gm;
          if (stats) sW[tid * WS + n] = live ? gm / qv[n] : 0.0;
        }
    }
    if (stats) {
      __syncthreads();
      if (worker) {
        const int tl = min(tile, T - t0);
        for (int tt = g; tt < tl; tt += G) {
          const double w = sW[tt * WS + rn];
          const c128 za = sZ[tt * ZS + ra];
          const c128 wa = cmake(w * za.x, w * za.y);
#pragma unroll
          for (int c = 0; c < M; ++c) {
            const c128 zc = sZ[tt * ZS + c];
            acc[c].x = fma(wa.x, zc.x, acc[c].x);
            acc[c].x = fma(wa.y, zc.y, acc[c].x);
            acc[c].y = fma(wa.y, zc.x, acc[c].y);
            acc[c].y = fma(-wa.x, zc.y, acc[c].y);
          }
        }
      }
      __syncthreads();
    }
  }

  if (stats) {
    // fold the G frame groups in group order through the tile's LDS, as many groups per round
    // as fit (at least one: a group has N M^2 <= 128 M values, the region tile (M | 1), tile >= 128)
    c128 *red = sZ;  // (the last barrier of the loop is behind every read of sZ)
    const int cap = tile * ZS;
    const int per = rows * M;
    const int fit = cap / per;
    c128 total[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) total[k] = cmake(0.0, 0.0);
    for (int g0 = 0; g0 < G; g0 += fit) {
      const int gn = min(fit, G - g0);
      if (worker && g >= g0 && g < g0 + gn) {
#pragma unroll
        for (int c = 0; c < M; ++c) red[((g - g0) * rows + r) * M + c] = acc[c];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int o = tid + k * CACGMM_THREADS;
        if (o < per)
          for (int gg = 0; gg < gn; ++gg) total[k] = cadd(total[k], red[gg * per + o]);
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int o = tid + k * CACGMM_THREADS;
      if (o < per) {
        const int n = o / MM;
        num[(((long long)b * N + n) * F + f) * MM + (o - n * MM)] = total[k];
      }
    }
  }

  // sum_t gamma_n and sum_t lse over the workgroup
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int n = 0; n < NMAX; ++n)
    if (n < N) {
      const double v = wave_sum(sg[n]);
      if (lane == 0) sRed[wave * (NMAX + 1) + n] = v;
    }
  {
    const double v = wave_sum(lse_acc);
    if (lane == 0) sRed[wave * (NMAX + 1) + NMAX] = v;
  }
  __syncthreads();
  if (tid <= NMAX && (tid < N || tid == NMAX)) {
    double v = 0.0;
    for (int w = 0; w < CACGMM_THREADS / 64; ++w) v += sRed[w * (NMAX + 1) + tid];
    if (tid < N) {
      if (sum_gamma) sum_gamma[((long long)b * N + tid) * F + f] = v;
    } else if (loss) {
      loss[(long long)b * F + f] = -(v / (double)T);
    }
  }
}

// alpha = sum_gamma / T;  num <- M (num / sum_gamma) in place.  One thread per matrix element.
__global__ __launch_bounds__(256) void k_cacgmm_scale(const double *__restrict__ sum_gamma, c128 *num,
                                                      double *mixing, long long n_mat, int M, int T) {
  const int MM = M * M;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_mat * MM) return;
  const long long idx = e / MM;
  const double s = sum_gamma[idx];
  const c128 v = num[e];
  num[e] = cmake((double)M * (v.x / s), (double)M * (v.y / s));
  if (e - idx * MM == 0) mixing[idx] = s / (double)T;
}

// The tail of the parameter step and normalize_covariance, a lane per matrix:
//   hermitise: B <- (B + B^H) / 2, the closing step of to_psd (the rebuilt P diag(lam) P^H of the
//              row-distributed eigensolvers is Hermitian only to the last bit);
//   normalize: B <- B / Re tr B (the trace is read before any element is rewritten).
// ref: ssspy/special/psd.py:66-69, ssspy/bss/cacgmm.py:207-222
__global__ __launch_bounds__(256) void k_cacgmm_normalize(c128 *cov, long long n_mat, int M,
                                                          int hermitise, int normalize) {
  const int MM = M * M;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_mat) return;
  c128 *C = cov + idx * MM;
  if (hermitise) {
    for (int a = 0; a < M; ++a) {
      C[a * M + a] = cmake(C[a * M + a].x, 0.0);
      for (int c = a + 1; c < M; ++c) {
        const c128 x = C[a * M + c], y = C[c * M + a];
        const c128 z = cmake(0.5 * (x.x + y.x), 0.5 * (x.y - y.y));
        C[a * M + c] = z;
        C[c * M + a] = cconj(z);
      }
    }
  }
  if (!normalize) return;
  double tr = 0.0;
  for (int a = 0; a < M; ++a) tr += C[a * M + a].x;
  for (int e = 0; e < MM; ++e) {
    const c128 v = C[e];
    C[e] = cmake(v.x / tr, v.y / tr);
  }
}

// B^-1 (packed) and log alpha - log det B per (mixture, source, bin); a lane per matrix, packed
// Hermitian storage (M^2 registers).  Only the upper triangle of B is read.  A pivot that is not
// positive bumps info[0] (numpy.linalg.inv raises LinAlgError on a singular matrix).
template <int M>
__global__ __launch_bounds__(64) void k_cacgmm_prepare(const c128 *__restrict__ cov,
                                                       const double *__restrict__ mixing,
                                                       double *binv, double *logp, long long n_mat,
                                                       int *info) {
  constexpr int MM = M * M;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_mat) return;
  HermP<M> A;
#pragma unroll
  for (int a = 0; a < M; ++a) {
    A.d[a] = cov[idx * MM + a * M + a].x;
#pragma unroll
    for (int c = a + 1; c < M; ++c) A.o[tri<M>(a, c)] = cov[idx * MM + a * M + c];
  }
  double logdet = 0.0;
  const bool ok = hp_chol_inverse<M>(A, logdet);
  if (!ok && info) atomicAdd(info, 1);
#pragma unroll
  for (int a = 0; a < M; ++a) binv[idx * MM + a] = A.d[a];
#pragma unroll
  for (int e = 0; e < (M * (M - 1)) / 2; ++e) {
    binv[idx * MM + M + 2 * e] = A.o[e].x;
    binv[idx * MM + M + 2 * e + 1] = A.o[e].y;
  }
  logp[idx] = log(mixing[idx]) - logdet;
}

// out[row] = sum_f terms[row * F + f]: lane-strided partial sums, then the block's in a fixed order
__global__ __launch_bounds__(256) void k_cacgmm_fold_loss(const double *__restrict__ terms,
                                                          double *out, int F) {
  __shared__ double scratch[4];
  const long long row = blockIdx.x;
  double s = 0.0;
  for (int f = threadIdx.x; f < F; f += blockDim.x) s += terms[row * F + f];
  const double total = block_sum(s, scratch);
  if (threadIdx.x == 0) out[row] = total;
}

// out[b,n,f,t] = gamma[b,n,f,t] X[b,ref,f,t].  grid: (ceil(F T / 256), N, B)
__global__ __launch_bounds__(256) void k_cacgmm_separate(const double *__restrict__ gamma,
                                                         const c128 *__restrict__ X, c128 *out,
                                                         int N, int M, long long FT, int ref) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= FT) return;
  const int n = blockIdx.y, b = blockIdx.z;
  const c128 x = X[((long long)b * M + ref) * FT + e];
  const double gm = gamma[((long long)b * N + n) * FT + e];
  out[((long long)b * N + n) * FT + e] = cmake(gm * x.x, gm * x.y);
}

static int cacgmm_check_sizes(int B, int M, int N, int F, int T) {
  SSSPY_REQUIRE(B > 0 && F > 0 && T > 0 && M > 0 && N > 0, "cacgmm: bad shape");
  if (M < 2 || M > SSSPY_MAX_SOURCES)
    return fail(SSSPY_ERR_UNSUPPORTED, "cacgmm: n_channels must be in [2, 8]");
  if (N > CACGMM_MAX_SOURCES)
    return fail(SSSPY_ERR_UNSUPPORTED, "cacgmm: n_sources must be in [1, 16]");
  SSSPY_REQUIRE(B <= 65535 && N <= 65535, "cacgmm: too many mixtures for one launch");
  return SSSPY_OK;
}

#define CACGMM_DISPATCH_M(M_, CALL)                                                       \
  switch (M_) {                                                                           \
    case 2: { constexpr int MC = 2; CALL; } break;                                        \
    case 3: { constexpr int MC = 3; CALL; } break;                                        \
    case 4: { constexpr int MC = 4; CALL; } break;                                        \
    case 5: { constexpr int MC = 5; CALL; } break;                                        \
    case 6: { constexpr int MC = 6; CALL; } break;                                        \
    case 7: { constexpr int MC = 7; CALL; } break;                                        \
    case 8: { constexpr int MC = 8; CALL; } break;                                        \
    default: return ::ssspy::fail(SSSPY_ERR_UNSUPPORTED, "cacgmm: n_channels must be in [2, 8]"); \
  }

}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_cacgmm_unit_input(const void *X, void *Z, int B, int M, int F, int T, int floor_kind,
                            double floor_eps, void *stream) {
  SSSPY_REQUIRE(X && Z, "cacgmm_unit_input: bad argument");
  if (int rc = cacgmm_check_sizes(B, M, 1, F, T)) return rc;
  const long long FT = (long long)F * T;
  hipLaunchKernelGGL(k_cacgmm_unit, dim3((unsigned)((FT + 255) / 256), B), dim3(256), 0,
                     as_stream(stream), (const c128 *)X, (c128 *)Z, M, FT, floor_kind, floor_eps);
  return check_launch("k_cacgmm_unit");
}

int ssspy_cacgmm_prepare(const void *covariance, const double *mixing, double *binv, double *logp,
                         int B, int N, int F, int M, int *info, void *stream) {
  SSSPY_REQUIRE(covariance && mixing && binv && logp, "cacgmm_prepare: bad argument");
  if (int rc = cacgmm_check_sizes(B, M, N, F, 1)) return rc;
  const long long n_mat = (long long)B * N * F;
  dim3 grid((unsigned)((n_mat + 63) / 64)), block(64);
  CACGMM_DISPATCH_M(M, hipLaunchKernelGGL((k_cacgmm_prepare<MC>), grid, block, 0, as_stream(stream),
                                          (const c128 *)covariance, mixing, binv, logp, n_mat, info));
  return check_launch("k_cacgmm_prepare");
}

int ssspy_cacgmm_frame_pass(const void *Z, const double *binv, const double *logp, int B, int M,
                            int N, int F, int T, int floor_kind, double floor_eps,
                            double *sum_gamma, void *num, double *loss, double *posterior,
                            const double *posterior_in, void *stream) {
  SSSPY_REQUIRE(Z && binv && logp, "cacgmm_frame_pass: bad argument");
  SSSPY_REQUIRE((sum_gamma != nullptr) == (num != nullptr),
                "cacgmm_frame_pass: sum_gamma and num come together");
  if (int rc = cacgmm_check_sizes(B, M, N, F, T)) return rc;
  SSSPY_REQUIRE(F <= 0x7fffffff / 2, "cacgmm_frame_pass: too many bins for one launch");
  // the frame tile: 256 frames when the workgroup's LDS stays within 64 KB, else 128
  int tile = CACGMM_THREADS;
  if (cacgmm_pass_lds(M, N, tile) > 64 * 1024) tile = 128;
  const size_t smem = cacgmm_pass_lds(M, N, tile);
  dim3 grid(F, B), block(CACGMM_THREADS);
  CACGMM_DISPATCH_M(M, {
    if (smem > 48 * 1024) {
      // (granted once per instantiation and device, not on every launch)
      static size_t granted[64] = {};
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
      if (smem > granted[dev]) {
        hipError_t e = hipFuncSetAttribute((const void *)k_cacgmm_pass<MC>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return fail(SSSPY_ERR_HIP, hipGetErrorString(e));
        granted[dev] = smem;
      }
    }
    hipLaunchKernelGGL((k_cacgmm_pass<MC>), grid, block, smem, as_stream(stream), (const c128 *)Z,
                       binv, logp, N, F, T, tile, floor_kind, floor_eps, sum_gamma, (c128 *)num, loss,
                       posterior, posterior_in);
  });
  return check_launch("k_cacgmm_pass");
}

int ssspy_cacgmm_parameter_step(const double *sum_gamma, void *num, double *mixing, void *covariance,
                                int B, int N, int F, int M, int T, int floor_kind, double floor_eps,
                                int normalize, void *stream) {
  SSSPY_REQUIRE(sum_gamma && num && mixing && covariance && num != covariance,
                "cacgmm_parameter_step: bad argument");
  if (int rc = cacgmm_check_sizes(B, M, N, F, T)) return rc;
  const long long n_mat = (long long)B * N * F, total = n_mat * M * M;
  hipLaunchKernelGGL(k_cacgmm_scale, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     as_stream(stream), sum_gamma, (c128 *)num, mixing, n_mat, M, T);
  if (int rc = check_launch("k_cacgmm_scale")) return rc;
  if (int rc = ssspy_to_psd(num, covariance, n_mat, M, floor_kind, floor_eps, stream)) return rc;
  hipLaunchKernelGGL(k_cacgmm_normalize, dim3((unsigned)((n_mat + 255) / 256)), dim3(256), 0,
                     as_stream(stream), (c128 *)covariance, n_mat, M, 1, normalize ? 1 : 0);
  return check_launch("k_cacgmm_normalize");
}

int ssspy_cacgmm_normalize(void *covariance, int B, int N, int F, int M, void *stream) {
  SSSPY_REQUIRE(covariance, "cacgmm_normalize: bad argument");
  if (int rc = cacgmm_check_sizes(B, M, N, F, 1)) return rc;
  const long long n_mat = (long long)B * N * F;
  hipLaunchKernelGGL(k_cacgmm_normalize, dim3((unsigned)((n_mat + 255) / 256)), dim3(256), 0,
                     as_stream(stream), (c128 *)covariance, n_mat, M, 0, 1);
  return check_launch("k_cacgmm_normalize");
}

int ssspy_cacgmm_fold_loss(const double *terms, double *out, long long rows, int F, void *stream) {
  SSSPY_REQUIRE(terms && out && rows > 0 && rows <= 0x7fffffff && F > 0,
                "cacgmm_fold_loss: bad argument");
  hipLaunchKernelGGL(k_cacgmm_fold_loss, dim3((unsigned)rows), dim3(256), 0, as_stream(stream),
                     terms, out, F);
  return check_launch("k_cacgmm_fold_loss");
}

int ssspy_cacgmm_separate(const double *posterior, const void *X, void *out, int B, int N, int M,
                          int F, int T, int reference_id, void *stream) {
  SSSPY_REQUIRE(posterior && X && out && reference_id >= 0 && reference_id < M,
                "cacgmm_separate: bad argument");
  SSSPY_REQUIRE(B > 0 && N > 0 && F > 0 && T > 0 && B <= 65535 && N <= 65535,
                "cacgmm_separate: bad shape");
  const long long FT = (long long)F * T;
  hipLaunchKernelGGL(k_cacgmm_separate, dim3((unsigned)((FT + 255) / 256), N, B), dim3(256), 0,
                     as_stream(stream), posterior, (const c128 *)X, (c128 *)out, N, M, FT,
                     reference_id);
  return check_launch("k_cacgmm_separate");
}

}  // extern "C"
