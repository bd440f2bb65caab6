// Blind source separation by the alternating direction method of multipliers (ADMMBSS /
// MaskingADMMBSS).  ref: ssspy/bss/admmbss.py:220-257, :415-442.
//
// The state is W (B,F,N,N), auxiliary1 / dual1 (B,F,N,N) and auxiliary2 / dual2 (B,Q,N,F,T).
// Once per call:
//   k_prox_contract (operand X) + k_admm_invert: Ainv_i = (Q conj(X_i) X_i^T + I)^-1, Hermitian positive
//   definite and constant over the iterations (the reference rebuilds and solves it every iteration)
// An iteration is three passes:
//   (a) k_prox_contract:    R_i = (sum_q (auxiliary2_q - dual2_q))_i X_i^H per bin
//   (b) k_admm_filter_step: W = Ainv (auxiliary1 - dual1 + R), U = relax W + (1 - relax) auxiliary1,
//       auxiliary1 <- prox_{-log|det| / rho}(U + dual1), dual1 <- dual1 + U - auxiliary1; a lane per bin
//   (c) k_admm_aux_step:    per penalty Z = relax W x + (1 - relax) auxiliary2_q + dual2_q,
//       auxiliary2_q <- prox_q(Z, 1 / rho), dual2_q <- Z - auxiliary2_q
// Z is never stored: the pass that needs it forms it again (k_admm_bin_norms for l21 over bins, the
// first walk of l21 over frames).  The contraction is that of prox_passes.hpp with this family's operand.
#include "common.hpp"
#include "prox_passes.hpp"
#include "prox_svd.hpp"

namespace ssspy {

namespace {

constexpr int RM = SSSPY_RT_MAX_SOURCES;

// ---- A = Q conj(Gm) + I -> A^-1 in place for n matrices, a lane per matrix on private memory, with
// Gm[r][c] = sum_j x_r conj(x_c) from k_prox_contract: A = L L^H (Cholesky on the lower triangle),
// M = L^-1, A^-1 = M^H M.  NT as in k_prox_neg_logdet.  No votes: a lane past the end leaves.
template <int NT>
__global__ __launch_bounds__(64) void k_admm_invert(c128 *GA, long long n, int n_rt, double Qd) {
  constexpr int NM = NT > 0 ? NT : RM;
  const int N = NT > 0 ? NT : n_rt;
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  c128 *g = GA + lane * N * N;
  c128 L[NM * NM], M[NM * NM];
  for (int r = 0; r < N; ++r)
    for (int c = 0; c <= r; ++c) {
      const c128 v = g[r * N + c];
      L[r * N + c] = cmake(fma(Qd, v.x, r == c ? 1.0 : 0.0), r == c ? 0.0 : -Qd * v.y);
    }
  for (int j = 0; j < N; ++j) {
    double d = L[j * N + j].x;
    for (int k = 0; k < j; ++k) d -= cabs2(L[j * N + k]);
    const double ljj = sqrt(d), inv = 1.0 / ljj;
    L[j * N + j] = cmake(ljj, 0.0);
    for (int i = j + 1; i < N; ++i) {
      c128 s = L[i * N + j];
      for (int k = 0; k < j; ++k) cfms(s, L[i * N + k], cconj(L[j * N + k]));
      L[i * N + j] = cscale(s, inv);
    }
  }
  for (int j = 0; j < N; ++j) {
    M[j * N + j] = cmake(1.0 / L[j * N + j].x, 0.0);
    for (int i = j + 1; i < N; ++i) {
      c128 s = cmake(0.0, 0.0);
      for (int k = j; k < i; ++k) cfma(s, L[i * N + k], M[k * N + j]);
      const double inv = -1.0 / L[i * N + i].x;
      M[i * N + j] = cscale(s, inv);
    }
  }
  for (int r = 0; r < N; ++r)
    for (int c = 0; c <= r; ++c) {
      c128 s = cmake(0.0, 0.0);
      for (int k = r; k < N; ++k) cfma(s, cconj(M[k * N + r]), M[k * N + c]);
      g[r * N + c] = r == c ? cmake(s.x, 0.0) : s;
      if (r != c) g[c * N + r] = cconj(s);
    }
}

// ---- (b) the filter step for n bins, a lane per bin on private memory.  A lane past the end takes a
// zero matrix through the Jacobi (every lane is in its wave votes) and touches no memory.  U + dual1 waits in
// dual1's own memory while the Jacobi destroys the private copy: dual1 <- (U + dual1) - auxiliary1.
// An all-zero argument (the first iteration from the zero state) leaves prox_neg_logdet_lane as
// sqrt(1 / rho) I: the completion of the vanishing columns picks e_0, e_1, ... in order and V = I.
template <int NT>
__global__ __launch_bounds__(64) void k_admm_filter_step(const c128 *__restrict__ Ainv,
                                                         const c128 *__restrict__ R, c128 *W,
                                                         c128 *aux1, c128 *dual1, long long n, int n_rt,
                                                         double mu, double relax) {
  constexpr int NM = NT > 0 ? NT : RM;
  const int N = NT > 0 ? NT : n_rt;
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = lane < n;
  const long long base = lane * N * N;
  c128 A[NM * NM], V[NM * NM];
  double sv[NM];
  if (live) {
    // the right-hand side auxiliary1 - dual1 + R
    for (int e = 0; e < N * N; ++e) V[e] = cadd(csub(aux1[base + e], dual1[base + e]), R[base + e]);
    for (int r = 0; r < N; ++r)
      for (int c = 0; c < N; ++c) {
        c128 s = cmake(0.0, 0.0);
        for (int k = 0; k < N; ++k) cfma(s, Ainv[base + r * N + k], V[k * N + c]);
        A[r * N + c] = s;
      }
    const double om = 1.0 - relax;
    for (int e = 0; e < N * N; ++e) {
      const c128 w = A[e], v = aux1[base + e], y = dual1[base + e];
      const c128 u = cmake(relax * w.x + om * v.x, relax * w.y + om * v.y);
      A[e] = cadd(u, y);
      W[base + e] = w;
      dual1[base + e] = A[e];
    }
  } else {
    for (int e = 0; e < N * N; ++e) A[e] = cmake(0.0, 0.0);  // (no rotation: votes at once)
  }
  prox_neg_logdet_lane(A, V, sv, N, mu);
  if (!live) return;
  for (int r = 0; r < N; ++r)
    for (int c = 0; c < N; ++c) {
      const c128 v = prox_entry(A, V, N, r, c);
      const long long e = base + r * N + c;
      aux1[e] = v;
      dual1[e] = csub(dual1[e], v);
    }
}

// the operand of the contraction: d = sum_q (P_q - S_q), the penalties added in order, or d = P
// (Q = 1) where S is NULL (the Gram matrix of the mixture with P = X)
struct AdmmOperand {
  const c128 *__restrict__ P, *__restrict__ S;
  __device__ __forceinline__ c128 at(long long off, int j, int Q, long long NFT) const {
    c128 d = P[off + j];
    if (S) {
      d = csub(d, S[off + j]);
      for (int q = 1; q < Q; ++q) {
        const long long e = off + q * NFT + j;
        d = cadd(d, csub(P[e], S[e]));
      }
    }
    return d;
  }
};

// ---- the group norms of l21 over bins: part[c,b,n,j] = sum over the bins of chunk c of |Z|^2, in
// bin order.  grid (ceil(T / 256), C, B); a thread owns one frame.  No barriers.
template <int G>
__global__ __launch_bounds__(PROX_THREADS) void k_admm_bin_norms(
    const c128 *__restrict__ X, const c128 *__restrict__ W, const c128 *__restrict__ aux2,
    const c128 *__restrict__ dual2, long long bstride, int N, int F, int T, int FC, double relax,
    double *part) {
  const int j = blockIdx.x * PROX_THREADS + threadIdx.x;
  const int c = blockIdx.y, b = blockIdx.z, B = gridDim.z;
  if (j >= T) return;
  const long long FT = (long long)F * T;
  const bool mix = relax != 1.0;
  double r[G];
#pragma unroll
  for (int n = 0; n < G; ++n) r[n] = 0.0;
  const int i_end = min(F, (c + 1) * FC);
  for (int i = c * FC; i < i_end; ++i) {
    const c128 *__restrict__ Xb = X + ((long long)b * N * F + i) * T;
    const long long so = (long long)b * bstride + (long long)i * T;
    const c128 *__restrict__ Wn = W + ((long long)b * F + i) * (N * N);
    c128 z[G];
    admm_form_z<G>(z, Xb, aux2 + so, dual2 + so, Wn, N, FT, j, relax, mix);
#pragma unroll
    for (int n = 0; n < G; ++n) r[n] += cabs2(z[n]);
  }
#pragma unroll
  for (int n = 0; n < G; ++n)
    if (n < N) part[(((long long)c * B + b) * N + n) * T + j] = r[n];
}

// ---- (c) one penalty's auxiliary step.  grid (F, B), 256 threads; thread j walks frames j, j + 256,
// ... with the N rows of Z in registers; a thread reads the N entries of auxiliary2_q / dual2_q of its
// frame before it writes them.
//   kind L1 / L21_SOURCES / L21_BINS (r2 (B,N,T) from k_admm_bin_norms) / L21_FRAMES (the norm of a
//   row of the bin: a first walk and a block sum in wave order) / MASK (given (B,N,F,T): the mask,
//   auxiliary2_q <- given Z) / GIVEN (given is prox(Z), formed on the host) / PROX_KIND_FORM_Z (Z to
//   zout, the state untouched).
template <int G>
__global__ __launch_bounds__(PROX_THREADS) void k_admm_aux_step(
    const c128 *__restrict__ X, const c128 *__restrict__ W, c128 *aux2, c128 *dual2, long long bstride,
    int N, int F, int T, int kind, double step, double relax, const double *__restrict__ r2,
    const c128 *__restrict__ given, c128 *zout) {
  __shared__ c128 Ws[G * G];
  __shared__ double Rs[PROX_THREADS / 64][G];
  __shared__ double Rn[G];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x, b = blockIdx.y;
  const long long FT = (long long)F * T;
  const bool mix = relax != 1.0;
  const c128 *__restrict__ Xb = X + ((long long)b * N * F + i) * T;
  const long long so = (long long)b * bstride + (long long)i * T;
  c128 *Ab = aux2 + so, *Db = dual2 + so;
  const long long given_off = ((long long)b * N * F + i) * T;  // row n at + n FT
  if (tid < N * N) Ws[tid] = W[((long long)b * F + i) * (N * N) + tid];
  __syncthreads();
  if (kind == SSSPY_PROX_L21_FRAMES) {
    double r[G];
#pragma unroll
    for (int n = 0; n < G; ++n) r[n] = 0.0;
    for (int j = tid; j < T; j += PROX_THREADS) {
      c128 z[G];
      admm_form_z<G>(z, Xb, Ab, Db, Ws, N, FT, j, relax, mix);
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
    admm_form_z<G>(z, Xb, Ab, Db, Ws, N, FT, j, relax, mix);
    if (kind == PROX_KIND_FORM_Z) {
#pragma unroll
      for (int n = 0; n < G; ++n)
        if (n < N) zout[given_off + n * FT + j] = z[n];
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
        c128 v;
        if (kind == SSSPY_PROX_GIVEN) {
          v = given[given_off + n * FT + j];
        } else if (kind == SSSPY_PROX_MASK) {
          v = cmul(given[given_off + n * FT + j], z[n]);
        } else {
          double norm2;
          if (kind == SSSPY_PROX_L1) norm2 = cabs2(z[n]);
          else if (kind == SSSPY_PROX_L21_SOURCES) norm2 = all2;
          else if (kind == SSSPY_PROX_L21_BINS) norm2 = r2[((long long)b * N + n) * T + j];
          else norm2 = Rn[n];
          v = cscale(z[n], prox_shrink(sqrt(norm2), step));
        }
        Ab[n * FT + j] = v;
        Db[n * FT + j] = csub(z[n], v);
      }
    }
  }
}

static int launch_contract(const c128 *P, const c128 *S, const c128 *X, c128 *R, int B, int Q, int N,
                           int F, int T, hipStream_t st) {
  const AdmmOperand op = {P, S};
  SSSPY_PROX_DISPATCH_G(N, hipLaunchKernelGGL((k_prox_contract<GG, AdmmOperand>),
                                              dim3((unsigned)F, (unsigned)B), dim3(PROX_THREADS), 0, st,
                                              op, X, R, Q, N, F, T));
  return check_launch("k_prox_contract");
}

static int launch_aux_step(const void *X, const void *W, void *aux2_q, void *dual2_q, long long bstride,
                           int kind, double step, double relax, const double *r2, const void *given,
                           void *zout, int B, int N, int F, int T, hipStream_t st) {
  SSSPY_PROX_DISPATCH_G(N, hipLaunchKernelGGL((k_admm_aux_step<GG>), dim3((unsigned)F, (unsigned)B),
                                              dim3(PROX_THREADS), 0, st, (const c128 *)X,
                                              (const c128 *)W, (c128 *)aux2_q, (c128 *)dual2_q, bstride,
                                              N, F, T, kind, step, relax, r2, (const c128 *)given,
                                              (c128 *)zout));
  return check_launch("k_admm_aux_step");
}

}  // namespace

}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_admmbss_gram_inverse(const void *X, void *Ainv, int B, int Q, int N, int F, int T,
                               void *stream) {
  int rc = prox_check_args("admmbss_gram_inverse", X && Ainv && Q > 0, B, N, F, T);
  if (rc != SSSPY_OK) return rc;
  hipStream_t st = as_stream(stream);
  rc = launch_contract((const c128 *)X, nullptr, (const c128 *)X, (c128 *)Ainv, B, 1, N, F, T, st);
  if (rc != SSSPY_OK) return rc;
  const long long n = (long long)B * F;
  const dim3 grid((unsigned)((n + 63) / 64)), block(64);
  SSSPY_DISPATCH_N(N, hipLaunchKernelGGL((k_admm_invert<NN>), grid, block, 0, st, (c128 *)Ainv, n, N,
                                         (double)Q));
  return check_launch("k_admm_invert");
}

int ssspy_admmbss_contract(const void *aux2, const void *dual2, const void *X, void *R, int B, int Q,
                           int N, int F, int T, void *stream) {
  const int rc = prox_check_args("admmbss_contract", aux2 && dual2 && X && R && Q > 0, B, N, F, T);
  if (rc != SSSPY_OK) return rc;
  return launch_contract((const c128 *)aux2, (const c128 *)dual2, (const c128 *)X, (c128 *)R, B, Q, N,
                         F, T, as_stream(stream));
}

int ssspy_admmbss_filter_step(const void *Ainv, const void *R, void *W, void *aux1, void *dual1, int B,
                              int F, int N, double rho, double relaxation, void *stream) {
  SSSPY_REQUIRE(Ainv && R && W && aux1 && dual1 && aux1 != dual1 && W != aux1 && W != dual1 && B > 0 &&
                    F > 0,
                "admmbss_filter_step: bad argument");
  if (N < 1 || N > SSSPY_RT_MAX_SOURCES)
    return fail(SSSPY_ERR_UNSUPPORTED, "admmbss_filter_step: 1..16 sources");
  const long long n = (long long)B * F;
  const dim3 grid((unsigned)((n + 63) / 64)), block(64);
  SSSPY_DISPATCH_N(N, hipLaunchKernelGGL((k_admm_filter_step<NN>), grid, block, 0, as_stream(stream),
                                         (const c128 *)Ainv, (const c128 *)R, (c128 *)W, (c128 *)aux1,
                                         (c128 *)dual1, n, N, 1.0 / rho, relaxation));
  return check_launch("k_admm_filter_step");
}

size_t ssspy_admmbss_bin_norms_workspace_bytes(int B, int N, int F, int T) {
  if (!prox_shape_ok(B, N, F, T)) return 0;
  int FC, C;
  prox_chunks(F, FC, C);
  return (size_t)C * B * N * T * sizeof(double);
}

int ssspy_admmbss_bin_norms(const void *X, const void *W, const void *aux2_q, const void *dual2_q,
                            long long batch_stride, double relaxation, double *r2, int B, int N, int F,
                            int T, void *workspace, size_t workspace_bytes, void *stream) {
  int rc = prox_check_args("admmbss_bin_norms", X && W && aux2_q && dual2_q && r2 && workspace, B, N, F,
                           T, {"batch", batch_stride});
  if (rc != SSSPY_OK) return rc;
  SSSPY_REQUIRE(workspace_bytes >= ssspy_admmbss_bin_norms_workspace_bytes(B, N, F, T),
                "admmbss_bin_norms: workspace too small");
  int FC, C;
  prox_chunks(F, FC, C);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)((T + PROX_THREADS - 1) / PROX_THREADS), (unsigned)C, (unsigned)B);
  SSSPY_PROX_DISPATCH_G(N, hipLaunchKernelGGL((k_admm_bin_norms<GG>), grid, dim3(PROX_THREADS), 0, st,
                                              (const c128 *)X, (const c128 *)W, (const c128 *)aux2_q,
                                              (const c128 *)dual2_q, batch_stride, N, F, T, FC,
                                              relaxation, (double *)workspace));
  rc = check_launch("k_admm_bin_norms");
  if (rc != SSSPY_OK) return rc;
  return launch_fold_slabs((const double *)workspace, nullptr, r2, (long long)B * N * T, C, st);
}

int ssspy_admmbss_aux_step(const void *X, const void *W, void *aux2_q, void *dual2_q,
                           long long batch_stride, int kind, double step_size, double relaxation,
                           const double *r2, const void *given, int B, int N, int F, int T,
                           void *stream) {
  const int rc = prox_check_args("admmbss_aux_step", X && W && aux2_q && dual2_q && aux2_q != dual2_q,
                                 B, N, F, T, {"batch", batch_stride}, {"given", kind, r2, given});
  if (rc != SSSPY_OK) return rc;
  return launch_aux_step(X, W, aux2_q, dual2_q, batch_stride, kind, step_size, relaxation, r2, given,
                         nullptr, B, N, F, T, as_stream(stream));
}

int ssspy_admmbss_form_z(const void *X, const void *W, const void *aux2_q, const void *dual2_q,
                         long long batch_stride, double relaxation, void *Z, int B, int N, int F,
                         int T, void *stream) {
  const int rc = prox_check_args(
      "admmbss_form_z", X && W && aux2_q && dual2_q && Z && Z != aux2_q && Z != dual2_q, B, N, F, T,
      {"batch", batch_stride});
  if (rc != SSSPY_OK) return rc;
  return launch_aux_step(X, W, (void *)aux2_q, (void *)dual2_q, batch_stride, PROX_KIND_FORM_Z, 0.0,
                         relaxation, nullptr, nullptr, Z, B, N, F, T, as_stream(stream));
}

}  // extern "C"
