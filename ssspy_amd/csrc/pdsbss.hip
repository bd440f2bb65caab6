// Primal-dual splitting BSS (PDSBSS / MaskingPDSBSS) and the proximal operator of -log|det|.
// ref: ssspy/bss/pdsbss.py:197-219, :396-412; ssspy/linalg/prox.py.
//
// An iteration is three passes over X (B,N,F,T), W (B,F,N,N) and the dual variable (B,Q,N,F,T):
//   (a) k_pds_contract:    XY_i = (sum_q dual_q)_i X_i^H per bin, a contraction over penalties and frames
//   (b) k_prox_neg_logdet, fused form: Wt = prox_{-mu1 log|det|}(W - mu1 mu2 XY), W2 = 2 Wt - W,
//       W <- relaxed (the same kernel serves ssspy_prox_neg_logdet on its own)
//   (c) k_pds_dual_step:   per penalty Z = dual_q + W2 x, Yt = Z - prox_q(Z, 1 / mu2), dual_q <- relaxed
// Z is never stored: the pass that needs it forms it again from X, W2 and dual_q.  The group norm of
// l21 stays inside a lane (over sources), inside the workgroup of a bin (over frames) or comes from
// k_pds_bin_norms (over bins: partial sums per chunk of bins, added in chunk order).
// fp64 / complex128, no atomics, every sum in a fixed order: two runs give the same bits.
#include "common.hpp"
#include "pds_common.hpp"
#include "prox_svd.hpp"

namespace ssspy {

namespace {

constexpr int RM = SSSPY_RT_MAX_SOURCES;
constexpr int PDS_MAX_CHUNKS = FOLD_GROUP;  // (one level of k_fold_slabs: no scratch)
// a `kind` of k_pds_dual_step past the public SSSPY_PROX_* ones: Z to zout, the dual untouched
// (ssspy_pdsbss_form_z; ssspy_pdsbss_dual_step refuses it)
constexpr int PDS_KIND_FORM_Z = SSSPY_PROX_GIVEN + 1;

// ---- prox of -mu log|det| for n matrices, a lane per matrix on private memory.  NT: the size at
// compile time (1..8) or 0 for the size at run time (9..16).  A lane past the end works on the last
// matrix (every lane is in the wave votes) and writes nothing.
//   W2 == NULL: out = prox(X)
//   W2 != NULL (the filter step; X is W, out may be W): A = W - cxy XY, Wt = prox(A),
//     W2 = 2 Wt - W, out = relax Wt + (1 - relax) W
template <int NT>
__global__ __launch_bounds__(64) void k_prox_neg_logdet(const c128 *X, const c128 *__restrict__ XY,
                                                        c128 *out, c128 *W2, long long n, int n_rt,
                                                        double mu, double cxy, double relax) {
  constexpr int NM = NT > 0 ? NT : RM;
  const int N = NT > 0 ? NT : n_rt;
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = lane < n;
  const long long base = (live ? lane : n - 1) * N * N;
  c128 A[NM * NM], V[NM * NM];
  double sv[NM];
  for (int e = 0; e < N * N; ++e) {
    c128 a = X[base + e];
    if (W2) {
      const c128 xy = XY[base + e];
      a = cmake(a.x - cxy * xy.x, a.y - cxy * xy.y);
    }
    A[e] = a;
  }
  prox_neg_logdet_lane(A, V, sv, N, mu);
  if (!live) return;
  for (int r = 0; r < N; ++r)
    for (int c = 0; c < N; ++c) {
      const c128 wt = prox_entry(A, V, N, r, c);
      const long long e = base + r * N + c;
      if (W2) {
        const c128 w = X[e];
        W2[e] = cmake(2.0 * wt.x - w.x, 2.0 * wt.y - w.y);
        out[e] = cmake(relax * wt.x + (1.0 - relax) * w.x, relax * wt.y + (1.0 - relax) * w.y);
      } else {
        out[e] = wt;
      }
    }
}

static int launch_prox(const c128 *X, const c128 *XY, c128 *out, c128 *W2, long long n, int N,
                       double mu, double cxy, double relax, hipStream_t st) {
  const dim3 grid((unsigned)((n + 63) / 64)), block(64);
#define SSSPY_PROX_CASE(NN)                                                                     \
  case NN:                                                                                      \
    hipLaunchKernelGGL((k_prox_neg_logdet<NN>), grid, block, 0, st, X, XY, out, W2, n, N, mu, cxy, \
                       relax);                                                                  \
    break;
  switch (N) {
    SSSPY_PROX_CASE(1)
    SSSPY_PROX_CASE(2)
    SSSPY_PROX_CASE(3)
    SSSPY_PROX_CASE(4)
    SSSPY_PROX_CASE(5)
    SSSPY_PROX_CASE(6)
    SSSPY_PROX_CASE(7)
    SSSPY_PROX_CASE(8)
    default:
      hipLaunchKernelGGL((k_prox_neg_logdet<0>), grid, block, 0, st, X, XY, out, W2, n, N, mu, cxy,
                         relax);
  }
#undef SSSPY_PROX_CASE
  return check_launch("k_prox_neg_logdet");
}

// ---- (a) XY[b,i,n,m] = sum_j (sum_q dual[b,q,n,i,j]) conj(X[b,m,i,j]).  grid (F, B), 256 threads.
// G: the source count rounded up to a power of two.  Thread (n, jl) = (tid / FL, tid % FL), FL = 256 / G,
// walks frames jl, jl + FL, ... of row n with N accumulators; the frame lanes of a row are added by a
// butterfly inside a wave and over the waves of a row in wave order.
template <int G>
__global__ __launch_bounds__(PDS_THREADS) void k_pds_contract(const c128 *__restrict__ dual,
                                                              const c128 *__restrict__ X, c128 *XY,
                                                              int Q, int N, int F, int T) {
  constexpr int FL = PDS_THREADS / G;
  constexpr int S = FL < 64 ? FL : 64;    // frame lanes of a row inside one wave
  constexpr int WPR = FL > 64 ? FL / 64 : 1;  // waves per row
  __shared__ c128 Ps[G * WPR * G];
  const int tid = threadIdx.x, n = tid / FL, jl = tid % FL;
  const int i = blockIdx.x, b = blockIdx.y;
  const bool src = n < N;
  const long long FT = (long long)F * T;
  const c128 *__restrict__ Xb = X + ((long long)b * N * F + i) * T;  // row m at Xb + m FT
  const c128 *__restrict__ Db = dual + (long long)b * Q * N * FT + ((long long)(src ? n : 0) * F + i) * T;
  c128 acc[G];
#pragma unroll
  for (int m = 0; m < G; ++m) acc[m] = cmake(0.0, 0.0);
  if (src) {
    for (int j = jl; j < T; j += FL) {
      c128 d = Db[j];
      for (int q = 1; q < Q; ++q) d = cadd(d, Db[(long long)q * N * FT + j]);
#pragma unroll
      for (int m = 0; m < G; ++m)
        if (m < N) {
          const c128 x = Xb[m * FT + j];
          // acc += d conj(x)
          acc[m].x = fma(d.x, x.x, acc[m].x);
          acc[m].x = fma(d.y, x.y, acc[m].x);
          acc[m].y = fma(d.y, x.x, acc[m].y);
          acc[m].y = fma(-d.x, x.y, acc[m].y);
        }
    }
  }
#pragma unroll
  for (int off = S / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int m = 0; m < G; ++m) {
      acc[m].x += __shfl_xor(acc[m].x, off, 64);
      acc[m].y += __shfl_xor(acc[m].y, off, 64);
    }
  }
  if (jl % 64 == 0) {
    const int w = jl / 64;
#pragma unroll
    for (int m = 0; m < G; ++m) Ps[(n * WPR + w) * G + m] = acc[m];
  }
  __syncthreads();
  if (tid < N * N) {
    const int r = tid / N, m = tid % N;
    c128 s = Ps[(r * WPR) * G + m];
#pragma unroll
    for (int w = 1; w < WPR; ++w) s = cadd(s, Ps[(r * WPR + w) * G + m]);
    XY[(((long long)b * F + i) * N + r) * N + m] = s;
  }
}

// ---- the group norms of l21 over bins: part[c,b,n,j] = sum over the bins of chunk c of |Z|^2, in
// bin order.  grid (ceil(T / 256), C, B); a thread owns one frame.  No barriers.
template <int G>
__global__ __launch_bounds__(PDS_THREADS) void k_pds_bin_norms(const c128 *__restrict__ X,
                                                               const c128 *__restrict__ W2,
                                                               const c128 *__restrict__ dual,
                                                               long long dual_bstride, int N, int F,
                                                               int T, int FC, double *part) {
  const int j = blockIdx.x * PDS_THREADS + threadIdx.x;
  const int c = blockIdx.y, b = blockIdx.z, B = gridDim.z;
  if (j >= T) return;
  const long long FT = (long long)F * T;
  double r[G];
#pragma unroll
  for (int n = 0; n < G; ++n) r[n] = 0.0;
  const int i_end = min(F, (c + 1) * FC);
  for (int i = c * FC; i < i_end; ++i) {
    const c128 *__restrict__ Xb = X + ((long long)b * N * F + i) * T;
    const c128 *Db = dual + (long long)b * dual_bstride + (long long)i * T;
    const c128 *__restrict__ Wn = W2 + ((long long)b * F + i) * (N * N);
    c128 z[G];
    pds_form_z<G>(z, Xb, Db, Wn, N, FT, j);
#pragma unroll
    for (int n = 0; n < G; ++n) r[n] += cabs2(z[n]);
  }
#pragma unroll
  for (int n = 0; n < G; ++n)
    if (n < N) part[(((long long)c * B + b) * N + n) * T + j] = r[n];
}

// max(1 - step / max(norm, step), 0): the factor of l1 / l21 (ref: ssspy/linalg/prox.py:6-33)
__device__ __forceinline__ double pds_shrink(double norm, double step) {
  norm = norm < step ? step : norm;
  const double s = 1.0 - step / norm;
  return s < 0.0 ? 0.0 : s;  // (NaN propagates, as through np.maximum)
}

// ---- (c) one penalty's dual step.  grid (F, B), 256 threads; thread j walks frames j, j + 256, ...
// with the N rows of Z in registers.
//   kind L1 / L21_SOURCES / L21_BINS (r2 (B,N,T) from k_pds_bin_norms) / L21_FRAMES (the norm of a
//   row of the bin: a first walk and a block sum in wave order) / MASK (aux (B,N,F,T): Yt = Z - aux Z)
//   / GIVEN (aux is Yt, formed on the host) / PDS_KIND_FORM_Z (Z to zout, the dual untouched).
template <int G>
__global__ __launch_bounds__(PDS_THREADS) void k_pds_dual_step(
    const c128 *__restrict__ X, const c128 *__restrict__ W2, c128 *dual, long long dual_bstride, int N,
    int F, int T, int kind, double step, double relax, const double *__restrict__ r2,
    const c128 *__restrict__ aux, c128 *zout) {
  __shared__ c128 Ws[G * G];
  __shared__ double Rs[PDS_THREADS / 64][G];
  __shared__ double Rn[G];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x, b = blockIdx.y;
  const long long FT = (long long)F * T;
  const c128 *__restrict__ Xb = X + ((long long)b * N * F + i) * T;
  c128 *Db = dual + (long long)b * dual_bstride + (long long)i * T;
  const long long aux_off = ((long long)b * N * F + i) * T;  // row n at + n FT
  if (tid < N * N) Ws[tid] = W2[((long long)b * F + i) * (N * N) + tid];
  __syncthreads();
  if (kind == SSSPY_PROX_L21_FRAMES) {
    double r[G];
#pragma unroll
    for (int n = 0; n < G; ++n) r[n] = 0.0;
    for (int j = tid; j < T; j += PDS_THREADS) {
      c128 z[G];
      pds_form_z<G>(z, Xb, Db, Ws, N, FT, j);
#pragma unroll
      for (int n = 0; n < G; ++n) r[n] += cabs2(z[n]);
    }
#pragma unroll
    for (int n = 0; n < G; ++n) {
      const double s = wave_sum(r[n]);
      if (lane == 0) Rs[wave][n] = s;
    }
    __syncthreads();
    if (tid < G) {
      double s = Rs[0][tid];
#pragma unroll
      for (int w = 1; w < PDS_THREADS / 64; ++w) s += Rs[w][tid];
      Rn[tid] = s;
    }
    __syncthreads();
  }
  for (int j = tid; j < T; j += PDS_THREADS) {
    c128 z[G];
    if (kind != SSSPY_PROX_GIVEN) pds_form_z<G>(z, Xb, Db, Ws, N, FT, j);
    if (kind == PDS_KIND_FORM_Z) {
#pragma unroll
      for (int n = 0; n < G; ++n)
        if (n < N) zout[aux_off + n * FT + j] = z[n];
      continue;
    }
    double all2 = 0.0;
    if (kind == SSSPY_PROX_L21_SOURCES) {
#pragma unroll
      for (int n = 0; n < G; ++n) all2 += cabs2(z[n]);  // (rows past N are zero)
    }
#pragma unroll
    for (int n = 0; n < G; ++n) {
      if (n < N) {
        c128 yt;
        if (kind == SSSPY_PROX_GIVEN) {
          yt = aux[aux_off + n * FT + j];
        } else if (kind == SSSPY_PROX_MASK) {
          yt = csub(z[n], cmul(aux[aux_off + n * FT + j], z[n]));
        } else {
          double norm2;
          if (kind == SSSPY_PROX_L1) norm2 = cabs2(z[n]);
          else if (kind == SSSPY_PROX_L21_SOURCES) norm2 = all2;
          else if (kind == SSSPY_PROX_L21_BINS) norm2 = r2[((long long)b * N + n) * T + j];
          else norm2 = Rn[n];
          const double s = pds_shrink(sqrt(norm2), step);
          yt = cmake(z[n].x - s * z[n].x, z[n].y - s * z[n].y);
        }
        const c128 d = Db[n * FT + j];
        Db[n * FT + j] = cmake(relax * yt.x + (1.0 - relax) * d.x, relax * yt.y + (1.0 - relax) * d.y);
      }
    }
  }
}

// bins per chunk and chunks of the l21-over-bins norm pass
static void pds_chunks(int F, int &FC, int &C) {
  const int want = F < PDS_MAX_CHUNKS ? F : PDS_MAX_CHUNKS;
  FC = (F + want - 1) / want;
  C = (F + FC - 1) / FC;
}

}  // namespace

}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_prox_neg_logdet(const void *X, void *out, long long n, int N, double step_size,
                          void *stream) {
  SSSPY_REQUIRE(X && out && n > 0, "prox_neg_logdet: bad argument");
  if (N < 1 || N > SSSPY_RT_MAX_SOURCES)
    return fail(SSSPY_ERR_UNSUPPORTED, "prox_neg_logdet: the size must be in [1, 16]");
  return launch_prox((const c128 *)X, nullptr, (c128 *)out, nullptr, n, N, step_size, 0.0, 1.0,
                     as_stream(stream));
}

int ssspy_pdsbss_contract(const void *dual, const void *X, void *XY, int B, int Q, int N, int F,
                          int T, void *stream) {
  SSSPY_REQUIRE(dual && X && XY && Q > 0 && B > 0 && F > 0 && T > 0, "pdsbss_contract: bad argument");
  if (!pds_shape_ok(B, N, F, T))
    return fail(SSSPY_ERR_UNSUPPORTED, "pdsbss_contract: 1..16 sources, up to 65535 mixtures");
  SSSPY_PDS_DISPATCH_G(N, hipLaunchKernelGGL((k_pds_contract<GG>), dim3((unsigned)F, (unsigned)B),
                                             dim3(PDS_THREADS), 0, as_stream(stream),
                                             (const c128 *)dual, (const c128 *)X, (c128 *)XY, Q, N, F,
                                             T));
  return check_launch("k_pds_contract");
}

int ssspy_pdsbss_filter_step(void *W, const void *XY, void *W2, int B, int F, int N, double mu1,
                             double mu2, double relaxation, void *stream) {
  SSSPY_REQUIRE(W && XY && W2 && W != W2 && B > 0 && F > 0, "pdsbss_filter_step: bad argument");
  if (N < 1 || N > SSSPY_RT_MAX_SOURCES)
    return fail(SSSPY_ERR_UNSUPPORTED, "pdsbss_filter_step: 1..16 sources");
  return launch_prox((const c128 *)W, (const c128 *)XY, (c128 *)W, (c128 *)W2, (long long)B * F, N,
                     mu1, mu1 * mu2, relaxation, as_stream(stream));
}

size_t ssspy_pdsbss_bin_norms_workspace_bytes(int B, int N, int F, int T) {
  if (!pds_shape_ok(B, N, F, T)) return 0;
  int FC, C;
  pds_chunks(F, FC, C);
  return (size_t)C * B * N * T * sizeof(double);
}

int ssspy_pdsbss_bin_norms(const void *X, const void *W2, const void *dual_q,
                           long long dual_batch_stride, double *r2, int B, int N, int F, int T,
                           void *workspace, size_t workspace_bytes, void *stream) {
  SSSPY_REQUIRE(X && W2 && dual_q && r2 && workspace && B > 0 && F > 0 && T > 0,
                "pdsbss_bin_norms: bad argument");
  if (!pds_shape_ok(B, N, F, T))
    return fail(SSSPY_ERR_UNSUPPORTED, "pdsbss_bin_norms: 1..16 sources, up to 65535 mixtures");
  SSSPY_REQUIRE(dual_batch_stride >= (long long)N * F * T, "pdsbss_bin_norms: bad dual stride");
  SSSPY_REQUIRE(workspace_bytes >= ssspy_pdsbss_bin_norms_workspace_bytes(B, N, F, T),
                "pdsbss_bin_norms: workspace too small");
  int FC, C;
  pds_chunks(F, FC, C);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)((T + PDS_THREADS - 1) / PDS_THREADS), (unsigned)C, (unsigned)B);
  SSSPY_PDS_DISPATCH_G(N, hipLaunchKernelGGL((k_pds_bin_norms<GG>), grid, dim3(PDS_THREADS), 0, st,
                                             (const c128 *)X, (const c128 *)W2, (const c128 *)dual_q,
                                             dual_batch_stride, N, F, T, FC, (double *)workspace));
  const int rc = check_launch("k_pds_bin_norms");
  if (rc != SSSPY_OK) return rc;
  return launch_fold_slabs((const double *)workspace, nullptr, r2, (long long)B * N * T, C, st);
}

int ssspy_pdsbss_dual_step(const void *X, const void *W2, void *dual_q, long long dual_batch_stride,
                           int kind, double step_size, double relaxation, const double *r2,
                           const void *aux, int B, int N, int F, int T, void *stream) {
  SSSPY_REQUIRE(X && W2 && dual_q && B > 0 && F > 0 && T > 0, "pdsbss_dual_step: bad argument");
  SSSPY_REQUIRE(kind >= SSSPY_PROX_L1 && kind <= SSSPY_PROX_GIVEN, "pdsbss_dual_step: bad kind");
  SSSPY_REQUIRE(kind != SSSPY_PROX_L21_BINS || r2, "pdsbss_dual_step: l21 over bins needs r2");
  SSSPY_REQUIRE((kind != SSSPY_PROX_MASK && kind != SSSPY_PROX_GIVEN) || aux,
                "pdsbss_dual_step: this kind needs aux");
  if (!pds_shape_ok(B, N, F, T))
    return fail(SSSPY_ERR_UNSUPPORTED, "pdsbss_dual_step: 1..16 sources, up to 65535 mixtures");
  SSSPY_REQUIRE(dual_batch_stride >= (long long)N * F * T, "pdsbss_dual_step: bad dual stride");
  SSSPY_PDS_DISPATCH_G(N, hipLaunchKernelGGL((k_pds_dual_step<GG>), dim3((unsigned)F, (unsigned)B),
                                             dim3(PDS_THREADS), 0, as_stream(stream), (const c128 *)X,
                                             (const c128 *)W2, (c128 *)dual_q, dual_batch_stride, N, F,
                                             T, kind, step_size, relaxation, r2, (const c128 *)aux,
                                             (c128 *)nullptr));
  return check_launch("k_pds_dual_step");
}

int ssspy_pdsbss_form_z(const void *X, const void *W2, const void *dual_q,
                        long long dual_batch_stride, void *Z, int B, int N, int F, int T,
                        void *stream) {
  SSSPY_REQUIRE(X && W2 && dual_q && Z && Z != dual_q && B > 0 && F > 0 && T > 0,
                "pdsbss_form_z: bad argument");
  if (!pds_shape_ok(B, N, F, T))
    return fail(SSSPY_ERR_UNSUPPORTED, "pdsbss_form_z: 1..16 sources, up to 65535 mixtures");
  SSSPY_REQUIRE(dual_batch_stride >= (long long)N * F * T, "pdsbss_form_z: bad dual stride");
  SSSPY_PDS_DISPATCH_G(N, hipLaunchKernelGGL((k_pds_dual_step<GG>), dim3((unsigned)F, (unsigned)B),
                                             dim3(PDS_THREADS), 0, as_stream(stream), (const c128 *)X,
                                             (const c128 *)W2, (c128 *)dual_q, dual_batch_stride, N, F,
                                             T, PDS_KIND_FORM_Z, 0.0, 1.0,
                                             (const double *)nullptr, (const c128 *)nullptr,
                                             (c128 *)Z));
  return check_launch("k_pds_dual_step");
}

}  // extern "C"
