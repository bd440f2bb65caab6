// Primal-dual splitting BSS (PDSBSS / MaskingPDSBSS) and the proximal operator of -log|det|.
// ref: ssspy/bss/pdsbss.py:197-219, :396-412; ssspy/linalg/prox.py.
//
// An iteration is three passes over X (B,N,F,T), W (B,F,N,N) and the dual variable (B,Q,N,F,T):
//   (a) k_prox_contract:   XY_i = (sum_q dual_q)_i X_i^H per bin, a contraction over penalties and frames
//   (b) k_prox_neg_logdet, fused form: Wt = prox_{-mu1 log|det|}(W - mu1 mu2 XY), W2 = 2 Wt - W,
//       W <- relaxed (the same kernel serves ssspy_prox_neg_logdet on its own)
//   (c) k_pds_dual_step:   per penalty Z = dual_q + W2 x, Yt = Z - prox_q(Z, 1 / mu2), dual_q <- relaxed
// Z is never stored: the pass that needs it forms it again from X, W2 and dual_q.  The group norm of
// l21 stays inside a lane (over sources), inside the workgroup of a bin (over frames) or comes from
// k_pds_bin_norms (over bins: partial sums per chunk of bins, added in chunk order).
// (a) is the contraction of prox_passes.hpp with this family's operand.
#include "common.hpp"
#include "prox_passes.hpp"
#include "prox_svd.hpp"

namespace ssspy {

namespace {

constexpr int RM = SSSPY_RT_MAX_SOURCES;

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
  SSSPY_DISPATCH_N(N, hipLaunchKernelGGL((k_prox_neg_logdet<NN>), grid, block, 0, st, X, XY, out, W2, n,
                                         N, mu, cxy, relax));
  return check_launch("k_prox_neg_logdet");
}

// the operand of (a): d = sum_q dual_q, the penalties added in order
struct PdsOperand {
  const c128 *__restrict__ dual;
  __device__ __forceinline__ c128 at(long long off, int j, int Q, long long NFT) const {
    c128 d = dual[off + j];
    for (int q = 1; q < Q; ++q) d = cadd(d, dual[off + q * NFT + j]);
    return d;
  }
};

// ---- the group norms of l21 over bins: part[c,b,n,j] = sum over the bins of chunk c of |Z|^2, in
// bin order.  grid (ceil(T / 256), C, B); a thread owns one frame.  No barriers.
template <int G>
__global__ __launch_bounds__(PROX_THREADS) void k_pds_bin_norms(const c128 *__restrict__ X,
                                                               const c128 *__restrict__ W2,
                                                               const c128 *__restrict__ dual,
                                                               long long dual_bstride, int N, int F,
                                                               int T, int FC, double *part) {
  const int j = blockIdx.x * PROX_THREADS + threadIdx.x;
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

// ---- (c) one penalty's dual step.  grid (F, B), 256 threads; thread j walks frames j, j + 256, ...
// with the N rows of Z in registers.
//   kind L1 / L21_SOURCES / L21_BINS (r2 (B,N,T) from k_pds_bin_norms) / L21_FRAMES (the norm of a
//   row of the bin: a first walk and a block sum in wave order) / MASK (aux (B,N,F,T): Yt = Z - aux Z)
//   / GIVEN (aux is Yt, formed on the host) / PROX_KIND_FORM_Z (Z to zout, the dual untouched).
template <int G>
__global__ __launch_bounds__(PROX_THREADS) void k_pds_dual_step(
    const c128 *__restrict__ X, const c128 *__restrict__ W2, c128 *dual, long long dual_bstride, int N,
    int F, int T, int kind, double step, double relax, const double *__restrict__ r2,
    const c128 *__restrict__ aux, c128 *zout) {
  __shared__ c128 Ws[G * G];
  __shared__ double Rs[PROX_THREADS / 64][G];
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
    for (int j = tid; j < T; j += PROX_THREADS) {
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
      for (int w = 1; w < PROX_THREADS / 64; ++w) s += Rs[w][tid];
      Rn[tid] = s;
    }
    __syncthreads();
  }
  for (int j = tid; j < T; j += PROX_THREADS) {
    c128 z[G];
    if (kind != SSSPY_PROX_GIVEN) pds_form_z<G>(z, Xb, Db, Ws, N, FT, j);
    if (kind == PROX_KIND_FORM_Z) {
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
          const double s = prox_shrink(sqrt(norm2), step);
          yt = cmake(z[n].x - s * z[n].x, z[n].y - s * z[n].y);
        }
        const c128 d = Db[n * FT + j];
        Db[n * FT + j] = cmake(relax * yt.x + (1.0 - relax) * d.x, relax * yt.y + (1.0 - relax) * d.y);
      }
    }
  }
}

static int launch_dual_step(const void *X, const void *W2, void *dual_q, long long bstride, int kind,
                            double step, double relax, const double *r2, const void *aux, void *zout,
                            int B, int N, int F, int T, hipStream_t st) {
  SSSPY_PROX_DISPATCH_G(N, hipLaunchKernelGGL((k_pds_dual_step<GG>), dim3((unsigned)F, (unsigned)B),
                                              dim3(PROX_THREADS), 0, st, (const c128 *)X,
                                              (const c128 *)W2, (c128 *)dual_q, bstride, N, F, T, kind,
                                              step, relax, r2, (const c128 *)aux, (c128 *)zout));
  return check_launch("k_pds_dual_step");
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
  const int rc = prox_check_args("pdsbss_contract", dual && X && XY && Q > 0, B, N, F, T);
  if (rc != SSSPY_OK) return rc;
  const PdsOperand op = {(const c128 *)dual};
  SSSPY_PROX_DISPATCH_G(N, hipLaunchKernelGGL((k_prox_contract<GG, PdsOperand>),
                                              dim3((unsigned)F, (unsigned)B), dim3(PROX_THREADS), 0,
                                              as_stream(stream), op, (const c128 *)X, (c128 *)XY, Q, N,
                                              F, T));
  return check_launch("k_prox_contract");
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
  if (!prox_shape_ok(B, N, F, T)) return 0;
  int FC, C;
  prox_chunks(F, FC, C);
  return (size_t)C * B * N * T * sizeof(double);
}

int ssspy_pdsbss_bin_norms(const void *X, const void *W2, const void *dual_q,
                           long long dual_batch_stride, double *r2, int B, int N, int F, int T,
                           void *workspace, size_t workspace_bytes, void *stream) {
  int rc = prox_check_args("pdsbss_bin_norms", X && W2 && dual_q && r2 && workspace, B, N, F, T,
                           {"dual", dual_batch_stride});
  if (rc != SSSPY_OK) return rc;
  SSSPY_REQUIRE(workspace_bytes >= ssspy_pdsbss_bin_norms_workspace_bytes(B, N, F, T),
                "pdsbss_bin_norms: workspace too small");
  int FC, C;
  prox_chunks(F, FC, C);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)((T + PROX_THREADS - 1) / PROX_THREADS), (unsigned)C, (unsigned)B);
  SSSPY_PROX_DISPATCH_G(N, hipLaunchKernelGGL((k_pds_bin_norms<GG>), grid, dim3(PROX_THREADS), 0, st,
                                              (const c128 *)X, (const c128 *)W2, (const c128 *)dual_q,
                                              dual_batch_stride, N, F, T, FC, (double *)workspace));
  rc = check_launch("k_pds_bin_norms");
  if (rc != SSSPY_OK) return rc;
  return launch_fold_slabs((const double *)workspace, nullptr, r2, (long long)B * N * T, C, st);
}

int ssspy_pdsbss_dual_step(const void *X, const void *W2, void *dual_q, long long dual_batch_stride,
                           int kind, double step_size, double relaxation, const double *r2,
                           const void *aux, int B, int N, int F, int T, void *stream) {
  const int rc = prox_check_args("pdsbss_dual_step", X && W2 && dual_q, B, N, F, T,
                                 {"dual", dual_batch_stride}, {"aux", kind, r2, aux});
  if (rc != SSSPY_OK) return rc;
  return launch_dual_step(X, W2, dual_q, dual_batch_stride, kind, step_size, relaxation, r2, aux,
                          nullptr, B, N, F, T, as_stream(stream));
}

int ssspy_pdsbss_form_z(const void *X, const void *W2, const void *dual_q,
                        long long dual_batch_stride, void *Z, int B, int N, int F, int T,
                        void *stream) {
  const int rc = prox_check_args("pdsbss_form_z", X && W2 && dual_q && Z && Z != dual_q, B, N, F, T,
                                 {"dual", dual_batch_stride});
  if (rc != SSSPY_OK) return rc;
  return launch_dual_step(X, W2, (void *)dual_q, dual_batch_stride, PROX_KIND_FORM_Z, 0.0, 1.0, nullptr,
                          nullptr, Z, B, N, F, T, as_stream(stream));
}

}  // extern "C"
