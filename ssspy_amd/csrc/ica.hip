// Time-domain ICA (GradICA, NaturalGradICA, FastICA; ref: ssspy/bss/ica.py) on real fp64 waveforms.
//
// Three kernels:
//  * k_ica_stats: one pass over X (B,N,T).  A workgroup of four waves owns one chunk of ICA_CHUNK
//    samples of one mixture; lanes take consecutive samples, so every channel row is read with
//    coalesced 8-byte loads.  W is workgroup-uniform (its index depends on blockIdx and loop counters
//    only: scalar loads, SGPR operands of the FMAs).  Each lane forms y = W x, applies the
//    nonlinearity in registers and adds phi(y_n) r_m (r = y or x), G(y_n) and phi'(y_n) to its
//    accumulators; y and phi never reach memory.  Lane -> wave (xor butterfly) -> workgroup (waves in
//    order through LDS) -> one record per (mixture, chunk).  The chunk is a constant, so the set of
//    records, the order they are added in and every bit of the result are the same on every run.
//    2..8 sources: the count at compile time, all rows in one lane (at most 64 + 16 accumulators);
//    9..16: the count at run time, the rows of phi in groups of four over grid z (64 + 8
//    accumulators; every group forms all of y again -- correct, not tuned).
//  * k_ica_step: one wave per mixture adds the records in chunk order, divides by T and updates W.
//  * k_ica_separate: Y = W X.
//
// Algorithmic bytes of the statistics pass: 8 N T read per mixture (X once), (N N + 2 N) 8 written per
// 2048 samples.  fp64, no atomics on doubles.
#include "common.hpp"

namespace ssspy {
namespace {

constexpr int ICA_BLOCK = 256;
constexpr int ICA_ITEMS = 8;
constexpr int ICA_CHUNK = ICA_BLOCK * ICA_ITEMS;  // 2048 samples per record
constexpr int ICA_RT_ROWS = 4;
constexpr int ICA_MAX_N = 16;
constexpr int ICA_MAX_REC = ICA_MAX_N * ICA_MAX_N + 2 * ICA_MAX_N;

// G, phi, phi' of one sample.  The forms are the overflow-safe ones of the named NumPy functions in
// bss/ica.py: equal to log(1 + exp(y)), 1 / (1 + exp(-y)), log(cosh(y)) wherever those neither
// overflow nor underflow, finite where they do.  NaN goes through all three.
__device__ __forceinline__ void ica_terms(int kind, double y, double &g, double &phi, double &dphi) {
  if (kind == SSSPY_ICA_LAPLACE) {
    g = fabs(y);
    phi = (y != y) ? y : (double)((y > 0.0) - (y < 0.0));  // sign(0) = 0, as NumPy's
    dphi = 0.0;
  } else if (kind == SSSPY_ICA_LOGISTIC) {
    const double e = exp(-fabs(y));  // in [0, 1]
    const double d = 1.0 / (1.0 + e);
    g = ((y > 0.0) ? y : 0.0) + log1p(e);
    phi = (y >= 0.0) ? d : e * d;
    dphi = e * d * d;
  } else if (kind == SSSPY_ICA_LOGCOSH) {
    const double a = fabs(y);
    const double th = tanh(y);
    g = a + log1p(exp(-2.0 * a)) - 0.693147180559945309417232121458;
    phi = th;
    dphi = 1.0 - th * th;
  } else {  // SSSPY_ICA_IDENTITY
    g = 0.0;
    phi = y;
    dphi = 0.0;
  }
}

// NN: the number of sources at compile time, or 0: at run time (<= ICA_MAX_N).  R: rows of phi per
// workgroup (R == NN: all of them, grid z = 1).
template <int NN, int R>
__global__ __launch_bounds__(ICA_BLOCK) void k_ica_stats(
    const double *__restrict__ X, const double *__restrict__ W, const double *__restrict__ phi_in,
    const double *__restrict__ dphi_in, double *__restrict__ ws, int n_rt, long long T, int kind,
    int right_x) {
  constexpr int NM = NN ? NN : ICA_MAX_N;
  constexpr int NVAL = R * NM + 2 * R;
  const int N = NN ? NN : n_rt;
  const int b = blockIdx.y;
  const int r0 = (NN && R == NN) ? 0 : (int)blockIdx.z * R;
  const long long chunk = blockIdx.x, chunks = gridDim.x;
  const double *Xb = X + (long long)b * N * T;
  const double *Wb = W + (long long)b * N * N;

  double acc[R][NM], accg[R], accd[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    accg[r] = accd[r] = 0.0;
#pragma unroll
    for (int m = 0; m < NM; ++m) acc[r][m] = 0.0;
  }

  const long long t0 = chunk * ICA_CHUNK + threadIdx.x;
  // (the run-time form is not to be unrolled over the samples: it is at 256 VGPRs with one)
#pragma unroll(NN ? ICA_ITEMS : 1)
  for (int i = 0; i < ICA_ITEMS; ++i) {
    const long long t = t0 + (long long)i * ICA_BLOCK;
    if (t < T) {
      double x[NM], rt[NM];
#pragma unroll
      for (int k = 0; k < NM; ++k) x[k] = (k < N) ? Xb[(long long)k * T + t] : 0.0;
      if (right_x) {
#pragma unroll
        for (int m = 0; m < NM; ++m) rt[m] = x[m];
      } else {
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          double s = 0.0;
          if (m < N) {
#pragma unroll
            for (int k = 0; k < NM; ++k)
              if (k < N) s = fma(Wb[m * N + k], x[k], s);
          }
          rt[m] = s;
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int n = r0 + r;
        if (n < N) {
          double g, phi, dphi;
          if (kind == SSSPY_ICA_GIVEN) {
            const long long at = ((long long)b * N + n) * T + t;
            phi = phi_in[at];
            dphi = dphi_in ? dphi_in[at] : 0.0;
            g = 0.0;
          } else {
            double y = 0.0;
#pragma unroll
            for (int k = 0; k < NM; ++k)
              if (k < N) y = fma(Wb[n * N + k], x[k], y);
            ica_terms(kind, y, g, phi, dphi);
          }
#pragma unroll
          for (int m = 0; m < NM; ++m)
            if (m < N) acc[r][m] = fma(phi, rt[m], acc[r][m]);
          accg[r] += g;
          accd[r] += dphi;
        }
      }
    }
  }

  // lane -> wave -> workgroup, in a fixed order
  __shared__ double red[ICA_BLOCK / 64][NVAL];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const double v = wave_sum(acc[r][m]);
      if (lane == 0) red[wave][r * NM + m] = v;
    }
    const double vg = wave_sum(accg[r]), vd = wave_sum(accd[r]);
    if (lane == 0) {
      red[wave][R * NM + r] = vg;
      red[wave][R * NM + R + r] = vd;
    }
  }
  __syncthreads();
  const int e = threadIdx.x;
  if (e < NVAL) {
    double s = red[0][e];
#pragma unroll
    for (int w = 1; w < ICA_BLOCK / 64; ++w) s += red[w][e];
    double *rec = ws + ((long long)b * chunks + chunk) * (long long)(N * N + 2 * N);
    if (e < R * NM) {
      const int n = r0 + e / NM, m = e % NM;
      if (n < N && m < N) rec[n * N + m] = s;
    } else if (e < R * NM + R) {
      const int n = r0 + (e - R * NM);
      if (n < N) rec[N * N + n] = s;
    } else {
      const int n = r0 + (e - R * NM - R);
      if (n < N) rec[N * N + N + n] = s;
    }
  }
}

// One wave per mixture.  The matrices live in LDS (N <= 16); the wave is the whole workgroup, so
// __syncthreads() orders its LDS traffic.
__global__ __launch_bounds__(64) void k_ica_step(const double *__restrict__ ws, double *W, int N,
                                                 long long T, int chunks, int algorithm,
                                                 int holonomic, double step_size, double *loss_data,
                                                 double *logdet, double *means, int *info) {
  __shared__ double S[ICA_MAX_REC];
  __shared__ double Wo[ICA_MAX_N * ICA_MAX_N], A[ICA_MAX_N * ICA_MAX_N];
  __shared__ double D[ICA_MAX_N * ICA_MAX_N], Z[ICA_MAX_N * ICA_MAX_N];
  __shared__ int P[ICA_MAX_N];
  const int lane = threadIdx.x, b = blockIdx.x;
  const int NNv = N * N, rec = NNv + 2 * N;
  double *Wb = W + (long long)b * NNv;
  const double *wsb = ws + (long long)b * chunks * rec;

  for (int e = lane; e < rec; e += 64) {
    const double s = ordered_sum<double>(wsb + e, rec, chunks) / (double)T;
    S[e] = s;
    if (means) means[(long long)b * rec + e] = s;
  }
  for (int e = lane; e < NNv; e += 64) Wo[e] = A[e] = Wb[e];
  __syncthreads();

  if (loss_data && lane == 0) {
    double s = 0.0;
    for (int n = 0; n < N; ++n) s += S[NNv + n];
    loss_data[b] = s;
  }

  // P A = L U of the state the records were formed from: log|det W|, and the solve of GradICA
  bool singular = false;
  if (algorithm == SSSPY_ICA_GRAD || logdet) {
    for (int k = 0; k < N; ++k) {
      int p = k;
      double best = fabs(A[k * N + k]);
      for (int i = k + 1; i < N; ++i) {
        const double v = fabs(A[i * N + k]);
        if (v > best) {
          best = v;
          p = i;
        }
      }
      if (lane == 0) P[k] = p;
      __syncthreads();
      if (p != k && lane < N) {
        const double u = A[k * N + lane];
        A[k * N + lane] = A[p * N + lane];
        A[p * N + lane] = u;
      }
      __syncthreads();
      if (best == 0.0) {  // (uniform) an exactly zero pivot: numpy.linalg.inv raises here
        singular = true;
        continue;
      }
      const double pivot = A[k * N + k];
      if (lane > k && lane < N) A[lane * N + k] /= pivot;
      __syncthreads();
      const int m = N - k - 1;
      for (int e = lane; e < m * m; e += 64) {
        const int i = k + 1 + e / m, j = k + 1 + e % m;
        A[i * N + j] = fma(-A[i * N + k], A[k * N + j], A[i * N + j]);
      }
      __syncthreads();
    }
    if (logdet && lane == 0) {
      double s = 0.0;
      for (int k = 0; k < N; ++k) s += log(fabs(A[k * N + k]));
      logdet[b] = s;
    }
  }

  if (algorithm == SSSPY_ICA_GRAD || algorithm == SSSPY_ICA_NATURAL_GRAD) {
    // D = PhiY - I (holonomic) or PhiY off the diagonal
    for (int e = lane; e < NNv; e += 64) {
      const bool diag = (e / N) == (e % N);
      D[e] = holonomic ? (diag ? S[e] - 1.0 : S[e]) : (diag ? 0.0 : S[e]);
    }
    __syncthreads();
    if (algorithm == SSSPY_ICA_NATURAL_GRAD) {
      for (int e = lane; e < NNv; e += 64) {
        const int i = e / N, j = e % N;
        double s = 0.0;
        for (int k = 0; k < N; ++k) s = fma(D[i * N + k], Wo[k * N + j], s);
        Wb[e] = Wo[e] - step_size * s;
      }
    } else if (singular) {
      if (lane == 0) atomicAdd(info, 1);
    } else if (lane < N) {
      // delta = D W^-T: row j of delta solves W v = (row j of D)^T; lane j owns row j of Z
      double *v = Z + lane * N;
      for (int i = 0; i < N; ++i) v[i] = D[lane * N + i];
      for (int k = 0; k < N; ++k) {
        const int p = P[k];
        if (p != k) {
          const double u = v[k];
          v[k] = v[p];
          v[p] = u;
        }
      }
      for (int i = 1; i < N; ++i) {
        double s = v[i];
        for (int k = 0; k < i; ++k) s = fma(-A[i * N + k], v[k], s);
        v[i] = s;
      }
      for (int i = N - 1; i >= 0; --i) {
        double s = v[i];
        for (int k = i + 1; k < N; ++k) s = fma(-A[i * N + k], v[k], s);
        v[i] = s / A[i * N + i];
      }
      for (int i = 0; i < N; ++i) Wb[lane * N + i] = Wo[lane * N + i] - step_size * v[i];
    }
  } else if (algorithm == SSSPY_ICA_FAST) {
    // row n: w <- E[phi'] w_n - E[phi z] from the OLD row, classical Gram-Schmidt against the rows
    // already updated (D holds them), unit norm.  A zero norm gives nan, as in the reference.
    for (int n = 0; n < N; ++n) {
      double w = 0.0;
      if (lane < N) w = S[NNv + N + n] * Wo[n * N + lane] - S[n * N + lane];
      if (lane < N) Z[lane] = w;
      __syncthreads();
      if (n > 0) {
        double corr = 0.0;
        for (int q = 0; q < n; ++q) {
          double scale = 0.0;
          for (int m = 0; m < N; ++m) scale += D[q * N + m] * Z[m];
          if (lane < N) corr += scale * D[q * N + lane];
        }
        w -= corr;
        __syncthreads();
        if (lane < N) Z[lane] = w;
        __syncthreads();
      }
      double norm2 = 0.0;
      for (int m = 0; m < N; ++m) norm2 += Z[m] * Z[m];
      if (lane < N) D[n * N + lane] = w / sqrt(norm2);
      __syncthreads();
    }
    for (int e = lane; e < NNv; e += 64) Wb[e] = D[e];
  }
}

template <int NN>
__global__ __launch_bounds__(ICA_BLOCK) void k_ica_separate(const double *__restrict__ X,
                                                            const double *__restrict__ W,
                                                            double *__restrict__ Y, int n_rt,
                                                            long long T) {
  constexpr int NM = NN ? NN : ICA_MAX_N;
  const int N = NN ? NN : n_rt;
  const int b = blockIdx.y;
  const long long t = (long long)blockIdx.x * ICA_BLOCK + threadIdx.x;
  if (t >= T) return;
  const double *Xb = X + (long long)b * N * T;
  const double *Wb = W + (long long)b * N * N;
  double *Yb = Y + (long long)b * N * T;
  double x[NM];
#pragma unroll
  for (int k = 0; k < NM; ++k) x[k] = (k < N) ? Xb[(long long)k * T + t] : 0.0;
#pragma unroll
  for (int n = 0; n < NM; ++n) {
    if (n < N) {
      double y = 0.0;
#pragma unroll
      for (int k = 0; k < NM; ++k)
        if (k < N) y = fma(Wb[n * N + k], x[k], y);
      Yb[(long long)n * T + t] = y;
    }
  }
}

inline long long ica_chunks(long long T) { return (T + ICA_CHUNK - 1) / ICA_CHUNK; }

inline int ica_shape_ok(int B, int N, long long T, const char *what) {
  if (B <= 0 || T <= 0) return fail(SSSPY_ERR_BADARG, what);
  if (N < 2 || N > ICA_MAX_N)
    return fail(SSSPY_ERR_UNSUPPORTED, "ICA takes 2 to 16 sources");
  if (B > 65535) return fail(SSSPY_ERR_UNSUPPORTED, "ICA takes up to 65535 mixtures per call");
  if (ica_chunks(T) > 2147483647LL) return fail(SSSPY_ERR_UNSUPPORTED, "ICA: n_samples too large");
  return SSSPY_OK;
}

}  // namespace
}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_ica_chunk_samples(int N, long long T) {
  (void)N;
  (void)T;
  return ICA_CHUNK;
}

size_t ssspy_ica_workspace_bytes(int B, int N, long long T) {
  if (B <= 0 || N < 2 || N > ICA_MAX_N || T <= 0) return 0;
  return (size_t)B * (size_t)ica_chunks(T) * (size_t)(N * N + 2 * N) * sizeof(double);
}

#define ICA_STATS_CASE(NN_)                                                                       \
  case NN_:                                                                                       \
    hipLaunchKernelGGL((k_ica_stats<NN_, NN_>), dim3((unsigned)chunks, B, 1), dim3(ICA_BLOCK), 0, \
                       st, X, W, phi, dphi, (double *)ws, N, T, kind, right);                     \
    break;

int ssspy_ica_stats(const double *X, const double *W, const double *phi, const double *dphi,
                    void *ws, size_t ws_bytes, int B, int N, long long T, int kind, int right,
                    void *stream) {
  SSSPY_REQUIRE(X && W && ws, "ica_stats: null pointer");
  const int rc = ica_shape_ok(B, N, T, "ica_stats: bad shape");
  if (rc != SSSPY_OK) return rc;
  SSSPY_REQUIRE(kind >= SSSPY_ICA_LAPLACE && kind <= SSSPY_ICA_GIVEN, "ica_stats: bad kind");
  SSSPY_REQUIRE(right == SSSPY_ICA_RIGHT_Y || right == SSSPY_ICA_RIGHT_X, "ica_stats: bad right");
  SSSPY_REQUIRE(kind != SSSPY_ICA_GIVEN || phi, "ica_stats: SSSPY_ICA_GIVEN needs phi");
  SSSPY_REQUIRE(ws_bytes >= ssspy_ica_workspace_bytes(B, N, T), "ica_stats: workspace too small");
  hipStream_t st = as_stream(stream);
  const long long chunks = ica_chunks(T);
  switch (N) {
    ICA_STATS_CASE(2)
    ICA_STATS_CASE(3)
    ICA_STATS_CASE(4)
    ICA_STATS_CASE(5)
    ICA_STATS_CASE(6)
    ICA_STATS_CASE(7)
    ICA_STATS_CASE(8)
    default:
      hipLaunchKernelGGL((k_ica_stats<0, ICA_RT_ROWS>),
                         dim3((unsigned)chunks, B, (N + ICA_RT_ROWS - 1) / ICA_RT_ROWS),
                         dim3(ICA_BLOCK), 0, st, X, W, phi, dphi, (double *)ws, N, T, kind, right);
  }
  return check_launch("k_ica_stats");
}

int ssspy_ica_step(const void *ws, size_t ws_bytes, double *W, int B, int N, long long T,
                   int algorithm, int holonomic, double step_size, double *loss_data,
                   double *logdet, double *means, int *info, void *stream) {
  SSSPY_REQUIRE(ws && W, "ica_step: null pointer");
  const int rc = ica_shape_ok(B, N, T, "ica_step: bad shape");
  if (rc != SSSPY_OK) return rc;
  SSSPY_REQUIRE(algorithm >= SSSPY_ICA_FOLD_ONLY && algorithm <= SSSPY_ICA_FAST,
                "ica_step: bad algorithm");
  SSSPY_REQUIRE(algorithm != SSSPY_ICA_GRAD || info, "ica_step: SSSPY_ICA_GRAD needs info");
  SSSPY_REQUIRE(ws_bytes >= ssspy_ica_workspace_bytes(B, N, T), "ica_step: workspace too small");
  hipLaunchKernelGGL(k_ica_step, dim3(B), dim3(64), 0, as_stream(stream), (const double *)ws, W, N, T,
                     (int)ica_chunks(T), algorithm, holonomic, step_size, loss_data, logdet, means,
                     info);
  return check_launch("k_ica_step");
}

#define ICA_SEPARATE_CASE(NN_)                                                                    \
  case NN_:                                                                                       \
    hipLaunchKernelGGL((k_ica_separate<NN_>), grid, dim3(ICA_BLOCK), 0, st, X, W, Y, N, T);       \
    break;

int ssspy_ica_separate(const double *X, const double *W, double *Y, int B, int N, long long T,
                       void *stream) {
  SSSPY_REQUIRE(X && W && Y, "ica_separate: null pointer");
  const int rc = ica_shape_ok(B, N, T, "ica_separate: bad shape");
  if (rc != SSSPY_OK) return rc;
  SSSPY_REQUIRE((T + ICA_BLOCK - 1) / ICA_BLOCK <= 2147483647LL, "ica_separate: n_samples too large");
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)((T + ICA_BLOCK - 1) / ICA_BLOCK), B, 1);
  switch (N) {
    ICA_SEPARATE_CASE(2)
    ICA_SEPARATE_CASE(3)
    ICA_SEPARATE_CASE(4)
    ICA_SEPARATE_CASE(5)
    ICA_SEPARATE_CASE(6)
    ICA_SEPARATE_CASE(7)
    ICA_SEPARATE_CASE(8)
    default:
      hipLaunchKernelGGL((k_ica_separate<0>), grid, dim3(ICA_BLOCK), 0, st, X, W, Y, N, T);
  }
  return check_launch("k_ica_separate");
}

}  // extern "C"
