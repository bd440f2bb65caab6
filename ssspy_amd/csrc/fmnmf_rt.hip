// FastGaussMNMF with n_channels M and n_sources N at run time, up to SSSPY_RT_MAX_SOURCES (16) each:
// the shapes neither the MFMA-tile kernels (N, M <= 4, mnmf_kernels.hip) nor the compile-time-M walk
// (M <= 8, N <= 8, fmnmf_generic.hip) take -- M in 9..16, or N in 9..16 at any M.
//
// fmnmf_generic_update / _loss / _separate keep the orchestration (and the basis / activation
// contractions, which do not depend on M) and hand the M- and N-shaped work to the entry points at
// the end of this file:
//   k_walk_rt        the point passes of fmg::k_walk (traces, diagonaliser weights, loss data term,
//                    spatial sums, closed-form Wiener filter), one lane = one (bin, frame) point
//   k_diag_cov_rt    U_m = (1/T) sum_j x x^H / R~_m for all M weight sets in one pass on the f64
//                    matrix cores, the weights formed in LDS (no (B, M, F, T) array in HBM)
//   k_norm_scale_rt  the power normalisation (psi up to 16)
//   k_qinv_rt        Q^-1 per bin, a wave per bin, Gauss-Jordan in LDS
//   k_repair_rt      the Wiener filter through the eigen-decomposition of R (flagged bins, and the two
//                    stages of a host flooring callable); per-lane matrices in scratch, as their <= 8
//                    counterparts (k_separate<M, true>) keep them
//
// Per-point arrays (x, |Qx|^2, R~, lambda) have the compile-time bound 16 and predicated, unrolled
// loops, so every index is a constant and they stay in VGPRs.  Q and D of a bin sit in a wave-private
// LDS patch, zero-padded to 16 x 16, so the inner loops run in groups of four columns without a
// predicate per element.
//
// replaces: ssspy/bss/mnmf.py:1278-1303 (update_once), :1305-1417, :1449-1514, :1635-1675, :632-678,
//           :1219-1261 (loss), :1174-1217 (Wiener filter) for the shapes above.
#include "common.hpp"
#include "hermitian.hpp"
#include "rt_dense.hpp"
#include "ssspy_amd.h"

namespace ssspy {

namespace fmr {

constexpr int MX = SSSPY_RT_MAX_SOURCES;  // bound of M and N
constexpr int KT = 8;                      // activation rows per source the LDS tile holds
constexpr int WB = 8;                      // waves per workgroup (they share the activation tile)
// the modes of fmg::k_walk (fmnmf_generic.hip), same numbers
enum { MODE_TRACES = 0, MODE_WEIGHTS = 1, MODE_LOSS = 2, MODE_SEPARATE = 3, MODE_SPATIAL = 4 };
constexpr int SPTS = 8;   // points per round through the MODE_SPATIAL patch
constexpr int SROW = 50;  // a point's row there: lam[0..16), h[16..32), g[32..48), padding

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Q (row m, column a at q[m * MX + a]), D (d[n * MX + m]) and the basis row of one bin, zero beyond
// (M, M), (N, M) and (N, K); private to a wave
struct WaveBin {
  c128 q[MX * MX];
  double d[MX * MX];
  double t[MX * KT];
};

__device__ __forceinline__ void stage_bin(WaveBin &s, const c128 *__restrict__ Q,
                                          const double *__restrict__ Dsp,
                                          const double *__restrict__ basis, long long bin, int b,
                                          int N, int M, int F, int K, int i, int lane) {
  wave_lds_sync();  // (the previous bin's reads are done)
#pragma unroll
  for (int u = 0; u < MX * MX / 64; ++u) {
    const int e = u * 64 + lane, r = e / MX, c = e % MX;
    s.q[e] = (r < M && c < M) ? Q[bin * (M * M) + r * M + c] : cmake(0.0, 0.0);
    s.d[e] = (r < N && c < M) ? Dsp[bin * (N * M) + r * M + c] : 0.0;
  }
#pragma unroll
  for (int u = 0; u < MX * KT / 64; ++u) {
    const int e = u * 64 + lane, n = e / KT, k = e % KT;
    s.t[e] = (K <= KT && n < N && k < K) ? basis[(((long long)b * N + n) * F + i) * K + k] : 0.0;
  }
  wave_lds_sync();
}

// lambda_n = sum_k t_nik v_nkj at the lane's frame
__device__ __forceinline__ double lambda_one(const double *vt, const WaveBin &s,
                                             const double *__restrict__ act_b,
                                             const double *__restrict__ basis, int b, int n, int N,
                                             int F, int T, int K, int i, int j, int lane) {
  double l = 0.0;
  if (K <= KT) {
    for (int k = 0; k < K; ++k) l = fma(s.t[n * KT + k], vt[(n * K + k) * 64 + lane], l);
  } else {
    const double *tr = basis + (((long long)b * N + n) * F + i) * K;
    for (int k = 0; k < K; ++k) l = fma(tr[k], act_b[((long long)n * K + k) * T + j], l);
  }
  return l;
}

// lam[n] of every source (zero beyond N)
__device__ __forceinline__ void lambda_rt(double (&lam)[MX], const double *vt, const WaveBin &s,
                                          const double *__restrict__ act_b,
                                          const double *__restrict__ basis, int b, int N, int F,
                                          int T, int K, int i, int j, int lane) {
#pragma unroll
  for (int n = 0; n < MX; ++n)
    lam[n] = n < N ? lambda_one(vt, s, act_b, basis, b, n, N, F, T, K, i, j, lane) : 0.0;
}

// (Q x)_m of row m (x zero beyond M; the patch's columns beyond M are zero).  (A scheduling fence
// after each group of four columns: left alone, hipcc hoists the LDS reads of every row to the top
// and spills.)
__device__ __forceinline__ c128 qrow_x(const WaveBin &s, const c128 (&x)[MX], int m, int M) {
  c128 acc = cmake(0.0, 0.0);
#pragma unroll
  for (int a4 = 0; a4 < MX / 4; ++a4) {
    if (4 * a4 < M) {
#pragma unroll
      for (int a = 4 * a4; a < 4 * a4 + 4; ++a) cfma(acc, s.q[m * MX + a], x[a]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return acc;
}

// R~_m = sum_n lam_n d_nm (lam and the patch are zero beyond N)
__device__ __forceinline__ double rtilde(const WaveBin &s, const double (&lam)[MX], int m, int N) {
  double r = 0.0;
#pragma unroll
  for (int n4 = 0; n4 < MX / 4; ++n4)
    if (4 * n4 < N) {
#pragma unroll
      for (int n = 4 * n4; n < 4 * n4 + 4; ++n) r = fma(lam[n], s.d[n * MX + m], r);
    }
  return r;
}

// grid: (frame tiles of 64, bin groups, B), 64 WB threads: wave w walks bins
// [(blockIdx.y * WB + w) * bpw, + bpw) for the block's 64 frames (lane = frame).  Outputs as
// fmg::k_walk:
//   MODE_TRACES   out0, out1 (B,N,F,T): A_n = sum_m d_nm |q_m x|^2 / R~_m^2, Bt_n = sum_m d_nm / R~_m
//   MODE_WEIGHTS  out0 (B,M,F,T): 1 / R~_m
//   MODE_LOSS     out0: one slot per (workgroup, wave), [slot][B]
//   MODE_SPATIAL  out0: per frame tile the (num, den) sums of the spatial update,
//                 [tile][b][i][n * M + m][2]
//   MODE_SEPARATE Yout (B,N,F,T): the closed form R^-1 = Q^H diag(1 / rc) Q where the eigenvalue
//                 floor is provably idle (lambda_min(R) >= min rc / ||Q||_F^2 > eps); bins with a
//                 point where it may act are flagged in `redo` for k_repair_rt
// dynamic LDS: the activation tile vt[(n K + k) * 64 + lane] when K <= KT, else none.
template <int MODE>
__global__ __launch_bounds__(64 * WB, 1) void k_walk_rt(const c128 *__restrict__ X,
                                                     const c128 *__restrict__ Q,
                                                     const c128 *__restrict__ Qinv,
                                                     const double *__restrict__ Dsp,
                                                     const double *__restrict__ basis,
                                                     const double *__restrict__ act,
                                                     double *__restrict__ out0,
                                                     double *__restrict__ out1,
                                                     c128 *__restrict__ Yout, int N, int M, int F,
                                                     int T, int K, int bpw, int ref,
                                                     int floor_kind, double eps, int *redo) {
  extern __shared__ __attribute__((aligned(16))) double vt[];
  __shared__ WaveBin bins[WB];
  __shared__ double pts[MODE == MODE_SPATIAL ? WB * SPTS * SROW : 1];
  __shared__ c128 qref[MODE == MODE_SEPARATE ? WB * MX : 1];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.z;
  const int j_raw = blockIdx.x * 64 + lane;
  const bool valid = j_raw < T;
  const int j = valid ? j_raw : T - 1;
  const c128 *Xb = X + (long long)b * M * F * T;
  const double *act_b = act + (long long)b * N * K * T;
  if (K <= KT) {
    for (int e = threadIdx.x >> 6; e < N * K; e += WB) vt[e * 64 + lane] = act_b[(long long)e * T + j];
    __syncthreads();
  }
  WaveBin &s = bins[wave];
  const int i0 = (blockIdx.y * WB + wave) * bpw;
  const int i1 = min(i0 + bpw, F);
  double loss = 0.0;
#pragma unroll 1
  for (int i = i0; i < i1; ++i) {
    const long long bin = (long long)b * F + i;
    stage_bin(s, Q, Dsp, basis, bin, b, N, M, F, K, i, lane);
    // lambda, then R~ (lambda dies here but for the spatial and Wiener modes), then x and Q x: the
    // fences keep hipcc from hoisting the x loads over the first two phases (they spilled)
    double lam[MX], rc[MX];
    lambda_rt(lam, vt, s, act_b, basis, b, N, F, T, K, i, j, lane);
#pragma unroll
    for (int m = 0; m < MX; ++m) rc[m] = m < M ? rtilde(s, lam, m, N) : 1.0;
    __builtin_amdgcn_sched_barrier(0);
    c128 x[MX];
#pragma unroll
    for (int m = 0; m < MX; ++m) x[m] = m < M ? Xb[((long long)m * F + i) * T + j] : cmake(0.0, 0.0);
    if (MODE == MODE_SEPARATE) {
      double qf2 = 0.0;
#pragma unroll
      for (int u = 0; u < MX * MX / 64; ++u) qf2 += cabs2(s.q[u * 64 + lane]);
      qf2 = wave_sum(qf2);
      wave_lds_sync();
      if (lane < M) qref[wave * MX + lane] = Qinv[bin * (M * M) + ref * M + lane];
      wave_lds_sync();
      c128 sm[MX];  // s_m = q~[ref][m] (Q x)_m / R~_m
      double rcmin = 0.0;
#pragma unroll
      for (int m = 0; m < MX; ++m) {
        sm[m] = cmake(0.0, 0.0);
        if (m < M) {
          const double r = rc[m];
          rcmin = m == 0 ? r : (r < rcmin ? r : rcmin);
          const c128 y = qrow_x(s, x, m, M);
          const double g = 1.0 / r;
          sm[m] = cmul(qref[wave * MX + m], cmake(y.x * g, y.y * g));
        }
      }
      const bool closed = floor_kind != SSSPY_FLOOR_ADD && rcmin > eps * qf2 * 1.0000001;
      if (valid && !closed) redo[bin] = 1;  // (every writer stores the same value)
      if (valid && closed) {
        // (lambda_n again from the tile: kept alive from the top, it spilled)
#pragma unroll
        for (int n = 0; n < MX; ++n)
          if (n < N) {
            const double ln = lambda_one(vt, s, act_b, basis, b, n, N, F, T, K, i, j, lane);
            c128 o = cmake(0.0, 0.0);
#pragma unroll
            for (int m = 0; m < MX; ++m) {
              const double dv = s.d[n * MX + m];  // (zero beyond M)
              o.x = fma(dv, sm[m].x, o.x);
              o.y = fma(dv, sm[m].y, o.y);
            }
            Yout[(((long long)b * N + n) * F + i) * T + j] = cmake(ln * o.x, ln * o.y);
          }
      }
      continue;
    }
    double qx2[MX];
#pragma unroll
    for (int m = 0; m < MX; ++m) qx2[m] = m < M ? cabs2(qrow_x(s, x, m, M)) : 0.0;
    if (MODE == MODE_TRACES) {
      double g[MX], h[MX];
#pragma unroll
      for (int m = 0; m < MX; ++m) {
        g[m] = 1.0 / rc[m];
        h[m] = qx2[m] * g[m] * g[m];
      }
#pragma unroll
      for (int n = 0; n < MX; ++n) {
        if (n < N && valid) {
          double sa = 0.0, sb = 0.0;
#pragma unroll
          for (int m4 = 0; m4 < MX / 4; ++m4)
            if (4 * m4 < M) {
#pragma unroll
              for (int m = 4 * m4; m < 4 * m4 + 4; ++m) {
                sa = fma(s.d[n * MX + m], h[m], sa);  // (d is zero beyond M)
                sb = fma(s.d[n * MX + m], g[m], sb);
              }
            }
          const long long o = (((long long)b * N + n) * F + i) * T + j;
          out0[o] = sa;
          out1[o] = sb;
        }
      }
    } else if (MODE == MODE_WEIGHTS) {
      if (valid) {
#pragma unroll
        for (int m = 0; m < MX; ++m)
          if (m < M) out0[(((long long)b * M + m) * F + i) * T + j] = 1.0 / rc[m];
      }
    } else if (MODE == MODE_LOSS) {
      double term = 0.0;
#pragma unroll
      for (int m = 0; m < MX; ++m)
        if (m < M) term += qx2[m] / rc[m] + log(rc[m]);
      loss += valid ? term : 0.0;
    } else {  // MODE_SPATIAL
      // num[n][m] = sum_j lam_n h_m, den[n][m] = sum_j lam_n g_m over the wave's 64 frames: two
      // (16 x 64) x (64 x 16) products on the matrix core, the points through the wave's LDS patch
      // in operand layout, SPTS at a time (rows past N and columns past M are zero)
      double *pw = pts + wave * SPTS * SROW;
      double4_t an = {0.0, 0.0, 0.0, 0.0}, ad = {0.0, 0.0, 0.0, 0.0};
      const int kq = lane >> 4, ic = lane & 15;
#pragma unroll 1
      for (int round = 0; round < 64 / SPTS; ++round) {
        wave_lds_sync();
        if ((lane / SPTS) == round) {
          double *mine = pw + (lane % SPTS) * SROW;
#pragma unroll
          for (int n = 0; n < MX; ++n) mine[n] = valid ? lam[n] : 0.0;  // frames beyond T add nothing
#pragma unroll
          for (int m = 0; m < MX; ++m) {
            const double g = m < M ? 1.0 / rc[m] : 0.0;
            mine[16 + m] = qx2[m] * g * g;
            mine[32 + m] = g;
          }
        }
        wave_lds_sync();
#pragma unroll
        for (int t = 0; t < SPTS / 4; ++t) {
          const double *row = pw + (4 * t + kq) * SROW;
          const double lv = row[ic];
          an = mfma_f64(lv, row[16 + ic], an);
          ad = mfma_f64(lv, row[32 + ic], ad);
        }
      }
      // D: column ic (= m), rows kq + 4 reg (= n)
      if (ic < M) {
        double *dst = out0 + (((long long)blockIdx.x * gridDim.z + b) * F + i) * (N * M) * 2;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = kq + 4 * r;
          if (n < N) {
            dst[(n * M + ic) * 2] = an[r];
            dst[(n * M + ic) * 2 + 1] = ad[r];
          }
        }
      }
    }
  }
  if (MODE == MODE_LOSS) {
    loss = wave_sum(loss);
    if (lane == 0)
      out0[(((long long)blockIdx.y * gridDim.x + blockIdx.x) * WB + wave) * gridDim.z + b] =
          loss / (double)T;
  }
}

// ---- U[b, i, m] = (1/T) sum_j x x^H / R~_ijm for all M weight sets of a bin in one pass.
// grid (F, B), 256 threads.  Per slab of 64 frames the block parks x (frame-major, 16 channels,
// zero-padded) and the weights 1 / R~ of every set in LDS, the lambdas formed there too; then wave w
// owns the sets m = w, w + 4, w + 8, w + 12.  With x~ = [Re x ; Im x] a set is four 16 x 16 tiles
//   RR, RI, IR, II  (D = sum_j w_j x~_j x~_j^T),   U = (RR + II) + i (IR - RI),
// each lane holds x_{lane & 15} of frame lane >> 4 of a 4-frame step -- the same element is its A
// (scaled by the weight) and its B operand -- and a step is 4 v_mfma_f64_16x16x4 per set.
constexpr int CW = 4;    // waves of k_diag_cov_rt
constexpr int CSL = 64;  // frames per slab
__global__ __launch_bounds__(64 * CW, 2) void k_diag_cov_rt(const c128 *__restrict__ X,
                                                         const double *__restrict__ Dsp,
                                                         const double *__restrict__ basis,
                                                         const double *__restrict__ act,
                                                         c128 *__restrict__ U, int N, int M, int F,
                                                         int T, int K) {
  __shared__ c128 xs[CSL][MX];       // 16 KB
  __shared__ double ws[MX][CSL];     // 8 KB: 1 / R~_m per frame (zero past T)
  __shared__ double ls[MX][CSL];     // 8 KB: lambda_n per frame
  __shared__ double dd[MX * MX];     // d[n * MX + m]
  const int i = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long bin = (long long)b * F + i;
  for (int e = threadIdx.x; e < MX * MX; e += blockDim.x) {
    const int n = e / MX, m = e % MX;
    dd[e] = (n < N && m < M) ? Dsp[bin * (N * M) + n * M + m] : 0.0;
  }
  const c128 *Xb = X + (long long)b * M * F * T + (long long)i * T;
  const double *act_b = act + (long long)b * N * K * T;
  double4_t acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int j0 = 0; j0 < T; j0 += CSL) {
    __syncthreads();  // (the previous slab's reads are done; dd is in)
    // x of the slab, frame-major: thread (channel group, frame)
    for (int e = threadIdx.x; e < MX * CSL; e += blockDim.x) {
      const int m = e / CSL, f = e % CSL;
      xs[f][m] = (m < M && j0 + f < T) ? Xb[(long long)m * F * T + j0 + f] : cmake(0.0, 0.0);
    }
    // lambda_n of the slab's frames: wave w takes n = w, w + 4, ...
    {
      const int j = min(j0 + lane, T - 1);
      for (int n = wave; n < N; n += CW) {
        const double *tr = basis + (((long long)b * N + n) * F + i) * K;
        double l = 0.0;
        for (int k = 0; k < K; ++k) l = fma(tr[k], act_b[((long long)n * K + k) * T + j], l);
        ls[n][lane] = l;
      }
    }
    __syncthreads();
    // 1 / R~_m: wave w takes m = w, w + 4, ...
    for (int m = wave; m < M; m += CW) {
      double r = 0.0;
      for (int n = 0; n < N; ++n) r = fma(ls[n][lane], dd[n * MX + m], r);
      ws[m][lane] = j0 + lane < T ? 1.0 / r : 0.0;
    }
    __syncthreads();
    const int a = lane & 15, kq = lane >> 4;
#pragma unroll 2
    for (int f0 = 0; f0 < CSL; f0 += 4) {
      const c128 xv = xs[f0 + kq][a];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int m = wave + CW * u;
        if (m < M) {
          const double w = ws[m][f0 + kq];
          const double ar = w * xv.x, ai = w * xv.y;
          acc[u][0] = mfma_f64(ar, xv.x, acc[u][0]);  // RR
          acc[u][1] = mfma_f64(ar, xv.y, acc[u][1]);  // RI
          acc[u][2] = mfma_f64(ai, xv.x, acc[u][2]);  // IR
          acc[u][3] = mfma_f64(ai, xv.y, acc[u][3]);  // II
        }
      }
    }
  }
  // D: column c = lane & 15, rows a = (lane >> 4) + 4 reg
  const int c = lane & 15, kq = lane >> 4;
  const double inv_t = 1.0 / (double)T;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int m = wave + CW * u;
    if (m < M && c < M) {
      c128 *Um = U + (bin * M + m) * (M * M);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = kq + 4 * r;
        if (a < M)
          Um[a * M + c] = cmake((acc[u][0][r] + acc[u][3][r]) * inv_t,
                                (acc[u][2][r] - acc[u][1][r]) * inv_t);
      }
    }
  }
}

// psi_m = floor(sqrt(mean_i q[i][m])); Q[:,m,:] /= psi_m; D[:,:,m] /= psi_m^2.  grid (ceil(F/64), B)
// (fmg::k_norm_scale with psi up to 16)
__global__ __launch_bounds__(256) void k_norm_scale_rt(c128 *Q, double *Dsp,
                                                       const double *__restrict__ qbuf, int N, int M,
                                                       int F, int floor_kind, double eps) {
  __shared__ double part[256];
  __shared__ double psi[MX];
  const int b = blockIdx.y;
  const double *qb = qbuf + (long long)b * F * M;
  const int rows = 256 / M, r = threadIdx.x / M, mch = threadIdx.x % M;
  double local = 0.0;
  if (r < rows)
    for (int i = r; i < F; i += rows) local += qb[(long long)i * M + mch];
  part[threadIdx.x] = local;
  __syncthreads();
  if (threadIdx.x < M) {
    double total = 0.0;
    for (int q = 0; q < rows; ++q) total += part[q * M + threadIdx.x];
    double v = total / (double)F;
    v = v < 0.0 ? 0.0 : v;
    psi[threadIdx.x] = apply_floor(sqrt(v), floor_kind, eps);
  }
  __syncthreads();
  const int i0 = blockIdx.x * 64;
  const int nb = min(64, F - i0);
  c128 *Qb = Q + ((long long)b * F + i0) * M * M;
  for (int e = threadIdx.x; e < nb * M * M; e += blockDim.x) {
    const int m = (e / M) % M;
    const c128 v = Qb[e];
    Qb[e] = cmake(v.x / psi[m], v.y / psi[m]);
  }
  double *Db = Dsp + ((long long)b * F + i0) * N * M;
  for (int e = threadIdx.x; e < nb * N * M; e += blockDim.x) {
    const int m = e % M;
    Db[e] = Db[e] / (psi[m] * psi[m]);
  }
}

// Qinv = Q^-1 per bin: a wave per bin, Gauss-Jordan on [Q | I] in LDS with partial pivoting (largest
// |re| + |im| of the column, the first one on ties, as rt_lu_solve).  grid B F, 64 threads.
__global__ __launch_bounds__(64) void k_qinv_rt(const c128 *__restrict__ Q, c128 *__restrict__ Qinv,
                                                int M, int *info) {
  __shared__ c128 a[MX][2 * MX];
  __shared__ c128 rowk[2 * MX];
  __shared__ c128 fac[MX];
  __shared__ int piv;
  const long long bin = blockIdx.x;
  const int lane = threadIdx.x, W = 2 * M;
  for (int e = lane; e < M * W; e += 64) {
    const int r = e / W, c = e % W;
    a[r][c] = c < M ? Q[bin * (M * M) + r * M + c] : cmake(c - M == r ? 1.0 : 0.0, 0.0);
  }
  __syncthreads();
  bool ok = true;
  for (int k = 0; k < M; ++k) {
    if (lane == 0) {
      int p = k;
      double best = cabs1(a[k][k]);
      for (int r = k + 1; r < M; ++r) {
        const double v = cabs1(a[r][k]);
        if (v > best) {
          best = v;
          p = r;
        }
      }
      piv = p;
    }
    __syncthreads();
    const int p = piv;
    if (p != k) {
      for (int c = lane; c < W; c += 64) {
        const c128 t = a[k][c];
        a[k][c] = a[p][c];
        a[p][c] = t;
      }
    }
    __syncthreads();
    const c128 pv = a[k][k];
    ok = ok && (pv.x != 0.0 || pv.y != 0.0);
    const c128 inv = crecip(pv);
    for (int c = lane; c < W; c += 64) rowk[c] = cmul(a[k][c], inv);
    if (lane < M) fac[lane] = a[lane][k];
    __syncthreads();
    for (int e = lane; e < M * W; e += 64) {
      const int r = e / W, c = e % W;
      if (r == k) {
        a[r][c] = rowk[c];
      } else {
        c128 v = a[r][c];
        cfms(v, fac[r], rowk[c]);
        a[r][c] = v;
      }
    }
    __syncthreads();
  }
  for (int e = lane; e < M * M; e += 64) Qinv[bin * (M * M) + e] = a[e / M][M + e % M];
  if (!ok && lane == 0 && info) atomicAdd(info, 1);
}

// The Wiener filter through R = Q~ diag(rc) Q~^H, Q~ = Q^-1, and its eigen-decomposition (to_psd;
// ref: ssspy/bss/mnmf.py:1174-1217): grid (F, B), 64 threads along frames.
//   EIG 0  bins flagged by k_walk_rt<MODE_SEPARATE> only; a point takes the closed form where the
//          floor is provably idle and the Jacobi eigen-floor elsewhere
//   EIG 1  every point: ascending eigenvalues lam_io (B, F, T, M) and eigenvectors P_io
//          (B, F, T, M, M) to HBM for a host flooring callable
//   EIG 2  every point: Y from the floored eigenvalues and the stored eigenvectors
// (the M x M working set of a point lives in the lane's scratch memory: it is indexed at run time)
template <int EIG>
__global__ __launch_bounds__(64) void k_repair_rt(const c128 *__restrict__ X,
                                                  const c128 *__restrict__ Q,
                                                  const c128 *__restrict__ Qinv,
                                                  const double *__restrict__ Dsp,
                                                  const double *__restrict__ basis,
                                                  const double *__restrict__ act, c128 *Y, int N,
                                                  int M, int F, int T, int K, int ref,
                                                  int floor_kind, double eps,
                                                  const int *__restrict__ redo, double *lam_io,
                                                  c128 *P_io) {
  const int i = blockIdx.x, b = blockIdx.y;
  const long long bin = (long long)b * F + i;
  if (EIG == 0 && !redo[bin]) return;
  __shared__ c128 qt[MX * MX];
  __shared__ c128 qsrc[MX * MX];
  __shared__ double dd[MX * MX];
  for (int e = threadIdx.x; e < M * M; e += blockDim.x) {
    qt[e] = Qinv[bin * (M * M) + e];
    qsrc[e] = Q[bin * (M * M) + e];
  }
  for (int e = threadIdx.x; e < N * M; e += blockDim.x) dd[e] = Dsp[bin * (N * M) + e];
  __syncthreads();
  double qf2 = 0.0;
  for (int e = 0; e < M * M; ++e) qf2 += cabs2(qsrc[e]);
  // every lane walks the same number of rounds (jacobi ends its sweeps on a wave vote)
  for (int j0 = 0; j0 < T; j0 += 64) {
    const bool valid = j0 + (int)threadIdx.x < T;
    const int j = valid ? j0 + threadIdx.x : T - 1;
    double lam[MX], rc[MX];
    c128 x[MX], sm[MX];
    for (int n = 0; n < N; ++n) {
      double r = 0.0;
      const double *tr = basis + (((long long)b * N + n) * F + i) * K;
      const double *Vn = act + ((long long)b * N + n) * K * T;
      for (int k = 0; k < K; ++k) r = fma(tr[k], Vn[(long long)k * T + j], r);
      lam[n] = r;
    }
    double rcmin = 0.0;
    for (int m = 0; m < M; ++m) {
      double r = 0.0;
      for (int n = 0; n < N; ++n) r = fma(lam[n], dd[n * M + m], r);
      rc[m] = r;
      rcmin = m == 0 ? r : (r < rcmin ? r : rcmin);
      x[m] = X[(((long long)b * M + m) * F + i) * T + j];
    }
    const bool closed = EIG == 0 && floor_kind != SSSPY_FLOOR_ADD && rcmin > eps * qf2 * 1.0000001;
    if (closed) {
      for (int m = 0; m < M; ++m) {
        c128 y = cmake(0.0, 0.0);
        for (int a = 0; a < M; ++a) cfma(y, qsrc[m * M + a], x[a]);
        const double g = 1.0 / rc[m];
        sm[m] = cmake(y.x * g, y.y * g);
      }
    }
    c128 A[MX * MX], P[MX * MX];
    double evs[MX];
    const long long point = bin * T + j;
    if (EIG == 2) {
      for (int k = 0; k < M; ++k) {
        evs[k] = lam_io[point * M + k];
        for (int a = 0; a < M; ++a) P[a * M + k] = P_io[(point * M + a) * M + k];
      }
    } else {
      for (int a = 0; a < M; ++a)
        for (int c2 = a; c2 < M; ++c2) {
          c128 s = cmake(0.0, 0.0);
          for (int m = 0; m < M; ++m) {
            const c128 zz = cmulc(qt[a * M + m], qt[c2 * M + m]);
            s.x = fma(rc[m], zz.x, s.x);
            s.y = fma(rc[m], zz.y, s.y);
          }
          if (a == c2) s.y = 0.0;
          A[a * M + c2] = s;
          A[c2 * M + a] = cconj(s);
        }
      jacobi(Runtime{M}, A, P);
      for (int k = 0; k < M; ++k) evs[k] = apply_floor(A[k * M + k].x, floor_kind, eps);
    }
    if (EIG == 1) {
      if (valid) {
        // ascending order (rank of every eigenvalue, ties by index)
        for (int k = 0; k < M; ++k) {
          int rank = 0;
          for (int l = 0; l < M; ++l)
            rank += (A[l * M + l].x < A[k * M + k].x || (A[l * M + l].x == A[k * M + k].x && l < k))
                        ? 1 : 0;
          lam_io[point * M + rank] = A[k * M + k].x;
          for (int a = 0; a < M; ++a) P_io[(point * M + a) * M + rank] = P[a * M + k];
        }
      }
      continue;
    }
    if (!closed) {
      c128 z[MX];
      for (int a = 0; a < M; ++a) z[a] = cmake(0.0, 0.0);
      for (int k = 0; k < M; ++k) {
        c128 proj = cmake(0.0, 0.0);  // p_k^H x
        for (int a = 0; a < M; ++a) {
          const c128 pk = P[a * M + k];
          proj.x += pk.x * x[a].x + pk.y * x[a].y;
          proj.y += pk.x * x[a].y - pk.y * x[a].x;
        }
        const double ev = evs[k];
        proj = cmake(proj.x / ev, proj.y / ev);
        for (int a = 0; a < M; ++a) cfma(z[a], P[a * M + k], proj);
      }
      for (int m = 0; m < M; ++m) {
        c128 s = cmake(0.0, 0.0);
        for (int c2 = 0; c2 < M; ++c2) {
          const c128 qv = qt[c2 * M + m];
          s.x += qv.x * z[c2].x + qv.y * z[c2].y;
          s.y += qv.x * z[c2].y - qv.y * z[c2].x;
        }
        sm[m] = s;
      }
    }
    if (!valid) continue;
    for (int m = 0; m < M; ++m) sm[m] = cmul(qt[ref * M + m], sm[m]);
    for (int n = 0; n < N; ++n) {
      c128 y = cmake(0.0, 0.0);
      for (int m = 0; m < M; ++m) {
        const double wgt = lam[n] * dd[n * M + m];
        y.x = fma(wgt, sm[m].x, y.x);
        y.y = fma(wgt, sm[m].y, y.y);
      }
      Y[(((long long)b * N + n) * F + i) * T + j] = y;
    }
  }
}

struct WalkPlan {
  int gx, gy, bpw;  // frame tiles, bin groups, bins per wave
};
// bins per wave so that the launch has about 256 workgroups of WB waves, at most 16
static inline WalkPlan walk_plan(int B, int F, int T) {
  WalkPlan p;
  p.gx = (T + 63) / 64;
  const int most = (F + WB - 1) / WB;
  int gy = (256 + p.gx * B - 1) / (p.gx * B);
  gy = gy < 1 ? 1 : (gy > most ? most : gy);
  p.bpw = (F + WB * gy - 1) / (WB * gy);
  if (p.bpw > 16) p.bpw = 16;
  p.gy = (F + WB * p.bpw - 1) / (WB * p.bpw);
  return p;
}

static inline size_t walk_lds(int N, int K) { return K <= KT ? (size_t)N * K * 64 * sizeof(double) : 0; }

template <int MODE>
static int launch(const void *X, const void *Q, const void *Qinv, const double *D,
                  const double *basis, const double *act, double *out0, double *out1, void *Y,
                  int B, int N, int M, int F, int T, int K, int ref, int floor_kind, double eps,
                  int *redo, hipStream_t st) {
  const WalkPlan p = walk_plan(B, F, T);
  const size_t lds = walk_lds(N, K);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void *)k_walk_rt<MODE>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(SSSPY_ERR_HIP, hipGetErrorString(e));
  }
  hipLaunchKernelGGL((k_walk_rt<MODE>), dim3(p.gx, p.gy, B), dim3(64 * WB), lds, st,
                     (const c128 *)X, (const c128 *)Q, (const c128 *)Qinv, D, basis, act, out0, out1,
                     (c128 *)Y, N, M, F, T, K, p.bpw, ref, floor_kind, eps, redo);
  return check_launch("fmnmf_rt walk");
}

}  // namespace fmr

// ---- entry points for fmnmf_generic.hip
bool fmnmf_rt_shape(int N, int M) {
  return N >= 1 && M >= 2 && N <= SSSPY_RT_MAX_SOURCES && M <= SSSPY_RT_MAX_SOURCES &&
         (N > SSSPY_MAX_SOURCES || M > SSSPY_MAX_SOURCES);
}

int fmnmf_rt_walk(int mode, const void *X, const void *Q, const void *Qinv, const double *D,
                  const double *basis, const double *act, double *out0, double *out1, void *Y,
                  int B, int N, int M, int F, int T, int K, int ref, int floor_kind, double eps,
                  int *redo, hipStream_t st) {
  using namespace fmr;
  if (!fmnmf_rt_shape(N, M))
    return fail(SSSPY_ERR_UNSUPPORTED, "FastMNMF: n_sources and n_channels must be at most 16");
#define FMR_LAUNCH(MD)                                                                              \
  case MD:                                                                                          \
    return launch<MD>(X, Q, Qinv, D, basis, act, out0, out1, Y, B, N, M, F, T, K, ref, floor_kind, \
                      eps, redo, st);
  switch (mode) {
    FMR_LAUNCH(MODE_TRACES)
    FMR_LAUNCH(MODE_WEIGHTS)
    FMR_LAUNCH(MODE_LOSS)
    FMR_LAUNCH(MODE_SEPARATE)
    FMR_LAUNCH(MODE_SPATIAL)
    default: return fail(SSSPY_ERR_INTERNAL, "fmnmf_rt_walk: bad mode");
  }
#undef FMR_LAUNCH
}

int fmnmf_rt_loss_slots(int B, int F, int T) {
  const fmr::WalkPlan p = fmr::walk_plan(B, F, T);
  return p.gx * p.gy * fmr::WB;
}

int fmnmf_rt_diagonalizer_covariance(const void *X, const double *D, const double *basis,
                                     const double *act, void *U, int B, int N, int M, int F, int T,
                                     int K, hipStream_t st) {
  if (!fmnmf_rt_shape(N, M))
    return fail(SSSPY_ERR_UNSUPPORTED, "FastMNMF: n_sources and n_channels must be at most 16");
  hipLaunchKernelGGL(fmr::k_diag_cov_rt, dim3(F, B), dim3(64 * fmr::CW), 0, st, (const c128 *)X, D,
                     basis, act, (c128 *)U, N, M, F, T, K);
  return check_launch("fmnmf_rt diagonalizer covariance");
}

int fmnmf_rt_norm_scale(void *Q, double *D, const double *qbuf, int B, int N, int M, int F,
                        int floor_kind, double eps, hipStream_t st) {
  hipLaunchKernelGGL(fmr::k_norm_scale_rt, dim3((F + 63) / 64, B), dim3(256), 0, st, (c128 *)Q, D,
                     qbuf, N, M, F, floor_kind, eps);
  return check_launch("fmnmf_rt norm_scale");
}

// redo: B F ints of scratch (bins the closed-form walk hands to the repair launch)
int fmnmf_rt_separate(const void *X, const void *Q, void *Qinv, const double *D,
                      const double *basis, const double *act, void *Y, int B, int N, int M, int F,
                      int T, int K, int ref, int floor_kind, double eps, int *info, int *redo,
                      hipStream_t st) {
  if (!fmnmf_rt_shape(N, M))
    return fail(SSSPY_ERR_UNSUPPORTED, "FastMNMF: n_sources and n_channels must be at most 16");
  const long long nbins = (long long)B * F;
  hipError_t e = hipMemsetAsync(redo, 0, (size_t)nbins * sizeof(int), st);
  if (e != hipSuccess) return fail(SSSPY_ERR_HIP, hipGetErrorString(e));
  hipLaunchKernelGGL(fmr::k_qinv_rt, dim3((unsigned)nbins), dim3(64), 0, st, (const c128 *)Q,
                     (c128 *)Qinv, M, info);
  int rc = check_launch("fmnmf_rt qinv");
  if (rc) return rc;
  rc = fmr::launch<fmr::MODE_SEPARATE>(X, Q, Qinv, D, basis, act, nullptr, nullptr, Y, B, N, M, F,
                                       T, K, ref, floor_kind, eps, redo, st);
  if (rc) return rc;
  hipLaunchKernelGGL((fmr::k_repair_rt<0>), dim3(F, B), dim3(64), 0, st, (const c128 *)X,
                     (const c128 *)Q, (const c128 *)Qinv, D, basis, act, (c128 *)Y, N, M, F, T, K,
                     ref, floor_kind, eps, (const int *)redo, (double *)nullptr, (c128 *)nullptr);
  return check_launch("fmnmf_rt separate repair");
}

// stage 1: Q^-1 and the ascending eigenvalues lam (B,F,T,M) / eigenvectors P (B,F,T,M,M) of every
// point; stage 2: Y from the (host-floored) lam and P
int fmnmf_rt_separate_eig(const void *X, const void *Q, void *Qinv, const double *D,
                          const double *basis, const double *act, void *Y, int B, int N, int M,
                          int F, int T, int K, int ref, int stage, double *lam, void *P, int *info,
                          hipStream_t st) {
  if (!fmnmf_rt_shape(N, M))
    return fail(SSSPY_ERR_UNSUPPORTED, "FastMNMF: n_sources and n_channels must be at most 16");
  const long long nbins = (long long)B * F;
  if (stage == 1) {
    hipLaunchKernelGGL(fmr::k_qinv_rt, dim3((unsigned)nbins), dim3(64), 0, st, (const c128 *)Q,
                       (c128 *)Qinv, M, info);
    hipLaunchKernelGGL((fmr::k_repair_rt<1>), dim3(F, B), dim3(64), 0, st, (const c128 *)X,
                       (const c128 *)Q, (const c128 *)Qinv, D, basis, act, (c128 *)Y, N, M, F, T, K,
                       ref, SSSPY_FLOOR_NONE, 0.0, (const int *)nullptr, lam, (c128 *)P);
  } else {
    hipLaunchKernelGGL((fmr::k_repair_rt<2>), dim3(F, B), dim3(64), 0, st, (const c128 *)X,
                       (const c128 *)Q, (const c128 *)Qinv, D, basis, act, (c128 *)Y, N, M, F, T, K,
                       ref, SSSPY_FLOOR_NONE, 0.0, (const int *)nullptr, lam, (c128 *)P);
  }
  return check_launch("fmnmf_rt separate (eigen stages)");
}

}  // namespace ssspy
