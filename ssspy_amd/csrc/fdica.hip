// Frequency-domain ICA (GradFDICA / NaturalGradFDICA / AuxFDICA-IP1 with the Laplace model): the
// elementwise weight of the per-iteration path and the bin-resident iteration kernel.
// ref: ssspy/bss/fdica.py:598-650, :793-843, :1065-1116.
//
// The bins of FDICA never talk to each other: the n_iter iterations of one (mixture, bin) are a
// closed problem on its N x T slab of the mixture.  k_fdica_steps gives a workgroup one (mixture, bin),
// keeps the slab in LDS when it fits (else re-reads it from global memory every step), keeps W on
// chip and runs every step inside one launch: the estimate, the weights and the covariances never
// exist in HBM.
//
// All three algorithms use the same statistics.  The Laplace score is phi(y) = y / floor(|y|) and the
// auxiliary weight 2 / floor(2 |y|): one real weight per (source, frame), so with
// U_n = mean_j weight_nj x_j x_j^H   (N Hermitian N x N matrices)
// IP1 sweeps on U_n directly and row n of P = mean_j phi(y) y^H is (w_n U_n) W^H, as in
// ssspy_iva_grad_step.
#include "common.hpp"
#include "rows_lu.hpp"

namespace ssspy {

constexpr int FDICA_THREADS = 256;
// The slab of a resident bin, N * T * 16 bytes, at most this: with the 6 KiB of statistics and filters
// below a workgroup stays under the 64 KiB of LDS that need no opt-in, and two workgroups fit a CU.
constexpr int FDICA_X_LDS_BYTES = 48 * 1024;
constexpr int FDICA_ROUTED_SOURCES = 4;  // (ssspy_fdica_route: above, the per-iteration operators)

// index of (p, q), p <= q, in the row-major upper triangle of an N x N matrix
template <int N>
__device__ __forceinline__ constexpr int tri(int p, int q) {
  return p * N - p * (p - 1) / 2 + (q - p);
}

// entry (p, q) of the Hermitian matrix whose upper triangle is U
template <int N>
__device__ __forceinline__ c128 herm_at(const c128 *U, int p, int q) {
  return p <= q ? U[tri<N>(p, q)] : cconj(U[tri<N>(q, p)]);
}

// Forward elimination of A z = rhs with partial pivoting, a G-lane group per matrix: lane r owns row
// r of A and of the NR right-hand sides (the layout of k_ip1_rows / k_grad_step_rows: the pivot is the
// largest |re| + |im| among the rows not yet used, the lowest row on ties).  Leaves the pivot owners
// (`plane`), the inverted pivots and the step at which a row was used (`order`); returns false on a
// zero pivot; ld = log|det A|.
template <int N, int G, int NR>
__device__ __forceinline__ bool rows_lu_forward(c128 (&a)[N], c128 (&rhs)[NR], int r, bool row,
                                                int &order, int (&plane)[N], c128 (&pinv)[N],
                                                double &ld) {
  bool ok = true;
  order = row ? -1 : N;
  ld = 0.0;
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
    c128 prow[N], prhs[NR];
#pragma unroll
    for (int c = k; c < N; ++c) prow[c] = shfl_c(a[c], bl, G);
#pragma unroll
    for (int c = 0; c < NR; ++c) prhs[c] = shfl_c(rhs[c], bl, G);
    const c128 piv = prow[k];
    ok = ok && (piv.x != 0.0 || piv.y != 0.0);
    ld += 0.5 * log(cabs2(piv));
    pinv[k] = crecip(piv);
    if (order < 0) {  // still unused: eliminate column k
      const c128 f = cmul(a[k], pinv[k]);
#pragma unroll
      for (int c = k + 1; c < N; ++c) cfms(a[c], f, prow[c]);
#pragma unroll
      for (int c = 0; c < NR; ++c) cfms(rhs[c], f, prhs[c]);
    }
  }
  return ok;
}

// ---- the weight of the per-iteration path: score form 1 / floor(|y|), auxiliary form
// 2 / floor(2 |y|), on Y (B, S, F, T) (the whole estimate, or a pair of its rows for IP2).
// `contrast`: sum_s mean_j 2 |y_sij| of (mixture b, bin i) at contrast[i * stride + b], to be added
// over the bins in slot order (ssspy_fold_scalar_slots); no atomics.  grid: (F, B)
__global__ __launch_bounds__(256) void k_fdica_weight(const c128 *__restrict__ Y, double *weight,
                                                      int S, int F, int T, int aux, int floor_kind,
                                                      double eps, double *contrast,
                                                      long long stride) {
  __shared__ double scratch[4];
  const int i = blockIdx.x, b = blockIdx.y;
  double g = 0.0;
  for (int s = 0; s < S; ++s) {
    const long long row = (((long long)b * S + s) * F + i) * T;
    for (int j = threadIdx.x; j < T; j += 256) {
      const double a = sqrt(cabs2(Y[row + j]));
      if (weight)
        weight[row + j] = aux ? 2.0 / apply_floor(2.0 * a, floor_kind, eps)
                              : 1.0 / apply_floor(a, floor_kind, eps);
      g += 2.0 * a;
    }
  }
  if (contrast) {  // (uniform: every thread reaches the barriers of block_sum)
    const double total = block_sum(g, scratch);
    if (threadIdx.x == 0) contrast[(long long)i * stride + b] = total / (double)T;
  }
}

// ---- the bin-resident iteration.  grid: (F, B), 256 threads; dynamic LDS: the slab when RESIDENT.
// Thread (jl, n) = (tid / G, tid % G) walks frames jl, jl + 256 / G, ... for source n: y = w_n x_j,
// the weight, and the N (N + 1) / 2 entries of its share of U_n -- no lane holds more than one
// covariance.  The shares are added over the lanes of a wave by a butterfly and over the four waves
// in wave order: a fixed order, the same bits on every run.  Wave 0 then updates the filter, lane r
// of every G-lane group owning row r (the groups compute the same thing; group 0 stores).
//   loss (may be NULL): step s leaves the contrast term sum_n mean_j 2 |y| of the state it STARTS
//   from at loss[i * slot_stride + s * B + b] and log|det W_i| of that state in `logdet` likewise;
//   a last walk without statistics leaves entry n_steps of the final state.
template <int N, bool RESIDENT>
__global__ __launch_bounds__(FDICA_THREADS) void k_fdica_steps(
    const c128 *__restrict__ X, c128 *W, int B, int F, int T, int algorithm, int holonomic,
    double eta, int floor_kind, double eps, int n_steps, double *loss, double *logdet,
    long long slot_stride, int *info) {
  constexpr int G = rows_group<N>();
  constexpr int FL = FDICA_THREADS / G;
  constexpr int NH = N * (N + 1) / 2;
  extern __shared__ c128 Xs[];
  __shared__ c128 Ws[N * N];
  __shared__ c128 Us[N * NH];
  __shared__ double Gs[N];
  const int tid = threadIdx.x, n = tid % G, jl = tid / G;
  const int lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x, b = blockIdx.y;
  const bool src = n < N;
  const int nn = src ? n : N - 1;  // (idle lanes shadow the last source, never store)
  const long long row_stride = (long long)F * T;
  const c128 *__restrict__ Xb = X + ((long long)b * N * F + i) * T;  // row c at Xb + c * row_stride
  c128 *Wb = W + ((long long)b * F + i) * (N * N);
  if (RESIDENT) {
    for (int c = 0; c < N; ++c)
      for (int j = tid; j < T; j += FDICA_THREADS) Xs[c * T + j] = Xb[c * row_stride + j];
  }
  if (tid < N * N) Ws[tid] = Wb[tid];
  __syncthreads();
  const double inv_t = 1.0 / (double)T;
  const bool aux = algorithm == SSSPY_FDICA_AUX_IP1;
  const int walks = loss ? n_steps + 1 : n_steps;
  bool ok = true;
#pragma unroll 1
  for (int s = 0; s < walks; ++s) {
    const bool last = s == n_steps;  // the final state: contrast only
    c128 w[N];
#pragma unroll
    for (int c = 0; c < N; ++c) w[c] = Ws[nn * N + c];
    c128 acc[NH];
#pragma unroll
    for (int k = 0; k < NH; ++k) acc[k] = cmake(0.0, 0.0);
    double g = 0.0;
#pragma unroll 1
    for (int j = jl; j < T; j += FL) {
      c128 x[N];
#pragma unroll
      for (int c = 0; c < N; ++c) x[c] = RESIDENT ? Xs[c * T + j] : Xb[c * row_stride + j];
      c128 y = cmake(0.0, 0.0);
#pragma unroll
      for (int c = 0; c < N; ++c) cfma(y, w[c], x[c]);
      const double a = sqrt(cabs2(y));
      g += 2.0 * a;
      if (!last) {
        const double phi = aux ? 2.0 / apply_floor(2.0 * a, floor_kind, eps)
                               : 1.0 / apply_floor(a, floor_kind, eps);
#pragma unroll
        for (int p = 0; p < N; ++p) {
          const c128 px = cscale(x[p], phi);
#pragma unroll
          for (int q = p; q < N; ++q) cfmac(acc[tri<N>(p, q)], px, x[q]);
        }
      }
    }
    // over the frame lanes of a wave (lanes of one source sit G apart)
#pragma unroll
    for (int off = G; off < 64; off <<= 1) {
      g += __shfl_xor(g, off, 64);
      if (!last) {
#pragma unroll
        for (int k = 0; k < NH; ++k) {
          acc[k].x += __shfl_xor(acc[k].x, off, 64);
          acc[k].y += __shfl_xor(acc[k].y, off, 64);
        }
      }
    }
    // over the waves, in wave order
#pragma unroll 1
    for (int wv = 0; wv < FDICA_THREADS / 64; ++wv) {
      if (wave == wv && lane < G && src) {
        Gs[n] = wv == 0 ? g : Gs[n] + g;
        if (!last) {
#pragma unroll
          for (int k = 0; k < NH; ++k) {
            c128 v = acc[k];
            if (wv > 0) v = cadd(Us[n * NH + k], v);
            if (wv == FDICA_THREADS / 64 - 1) v = cscale(v, inv_t);
            Us[n * NH + k] = v;
          }
        }
      }
      __syncthreads();
    }
    if (wave == 0) {
      const int r = n;  // my row
      const long long slot = (long long)i * slot_stride + (long long)s * B + b;
      if (loss && tid == 0) {
        double total = 0.0;
#pragma unroll
        for (int m = 0; m < N; ++m) total += Gs[m];
        loss[slot] = total * inv_t;
      }
      if (logdet) {
        c128 a[N], dummy[1];
        int order, plane[N];
        c128 pinv[N];
        double ld;
#pragma unroll
        for (int c = 0; c < N; ++c) a[c] = w[c];
        dummy[0] = cmake(0.0, 0.0);
        rows_lu_forward<N, G, 1>(a, dummy, r, src, order, plane, pinv, ld);
        if (tid == 0) logdet[slot] = ld;
      }
      if (!last && aux) {
        // IP1: w_n <- (W U_n)^-1 e_n / sqrt(w_n^H U_n w_n), n = 0 .. N - 1 (rows of W are w_n^H)
#pragma unroll 1
        for (int n2 = 0; n2 < N; ++n2) {
          const c128 *Un = Us + n2 * NH;
          c128 a[N];
#pragma unroll
          for (int c = 0; c < N; ++c) a[c] = cmake(0.0, 0.0);
#pragma unroll
          for (int m = 0; m < N; ++m)
#pragma unroll
            for (int c = 0; c < N; ++c) cfma(a[c], w[m], herm_at<N>(Un, m, c));
          c128 rhs[1];
          rhs[0] = cmake(r == n2 ? 1.0 : 0.0, 0.0);
          int order, plane[N];
          c128 pinv[N];
          double ld;
          ok = rows_lu_forward<N, G, 1>(a, rhs, r, src, order, plane, pinv, ld) && ok;
          c128 v[N];
#pragma unroll
          for (int k = N - 1; k >= 0; --k) {
            // the owner of pivot k has folded the unknowns above k into its right-hand side already
            const c128 mine = cmul(rhs[0], pinv[k]);
            v[k] = shfl_c(mine, plane[k], G);
            if (order < k) cfms(rhs[0], a[k], v[k]);
          }
          // Re(v^H U_n v): lane r takes row r, summed in row order on every lane
          double q = 0.0;
#pragma unroll
          for (int p = 0; p < N; ++p) {
            if (p == nn) {
              c128 t = cmake(0.0, 0.0);
#pragma unroll
              for (int c = 0; c < N; ++c) cfma(t, herm_at<N>(Un, p, c), v[c]);
              q = v[p].x * t.x + v[p].y * t.y;
            }
          }
          q = src ? q : 0.0;
          double qf = 0.0;
#pragma unroll
          for (int c = 0; c < N; ++c) qf += __shfl(q, c, G);
          qf = qf < 0.0 ? 0.0 : qf;  // np.maximum(., 0): NaN propagates
          const double d = apply_floor(sqrt(qf), floor_kind, eps);
          if (r == n2) {
#pragma unroll
            for (int c = 0; c < N; ++c) w[c] = cmake(v[c].x / d, -v[c].y / d);
          }
        }
      } else if (!last) {
        // row r of P = (w_r U_r) W^H, D = P - I (holonomic) or offdiag(P)
        const c128 *Ur = Us + nn * NH;
        c128 t[N], P[N], delta[N];
#pragma unroll
        for (int c = 0; c < N; ++c) t[c] = delta[c] = cmake(0.0, 0.0);
#pragma unroll
        for (int m = 0; m < N; ++m)
#pragma unroll
          for (int c = 0; c < N; ++c) cfma(t[c], w[m], herm_at<N>(Ur, m, c));
        const bool natural = algorithm == SSSPY_FDICA_NATURAL_GRAD;
#pragma unroll
        for (int m = 0; m < N; ++m) {
          c128 wm[N];  // row m of W
#pragma unroll
          for (int c = 0; c < N; ++c) wm[c] = shfl_c(w[c], m, G);
          c128 pm = cmake(0.0, 0.0);
          // (cfmac, where grad_iva.hip has cfma(., ., cconj(.)): the imaginary terms in the other
          //  order, different bits)
#pragma unroll
          for (int c = 0; c < N; ++c) cfmac(pm, t[c], wm[c]);
          if (m == nn) pm = holonomic ? cmake(pm.x - 1.0, pm.y) : cmake(0.0, 0.0);
          P[m] = pm;
          if (natural) {  // W <- W - eta D W
#pragma unroll
            for (int c = 0; c < N; ++c) cfma(delta[c], pm, wm[c]);
          }
        }
        if (!natural) {
          // W <- W - eta D W^-H: Z = D W^-H solves W Z^H = D^H
          c128 a[N], rhs[N];
#pragma unroll
          for (int c = 0; c < N; ++c) a[c] = w[c];
#pragma unroll
          for (int c = 0; c < N; ++c) {
            rhs[c] = cmake(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < N; ++k) {
              const c128 v = shfl_c(P[k], c, G);  // D[c][k]
              if (k == nn) rhs[c] = cconj(v);
            }
          }
          int order, plane[N];
          c128 pinv[N];
          double ld;
          ok = rows_lu_forward<N, G, N>(a, rhs, r, src, order, plane, pinv, ld) && ok;
#pragma unroll
          for (int k = N - 1; k >= 0; --k) {
#pragma unroll
            for (int c = 0; c < N; ++c) {
              const c128 mine = cmul(rhs[c], pinv[k]);
              const c128 z = shfl_c(mine, plane[k], G);  // Z^H[k][c]
              if (order < k) cfms(rhs[c], a[k], z);
              if (c == nn) delta[k] = cconj(z);
            }
          }
        }
#pragma unroll
        for (int c = 0; c < N; ++c) w[c] = cmake(w[c].x - eta * delta[c].x, w[c].y - eta * delta[c].y);
      }
      if (!last && lane < G && src) {
#pragma unroll
        for (int c = 0; c < N; ++c) Ws[r * N + c] = w[c];
      }
    }
    __syncthreads();
  }
  if (tid < N * N) Wb[tid] = Ws[tid];
  if (!ok && info && tid == 0) atomicAdd(info, 1);
}

static bool fdica_resident(int N, int T) {
  return (long long)N * T * (long long)sizeof(c128) <= FDICA_X_LDS_BYTES;
}

template <int N>
static int launch_fdica_steps(const c128 *X, c128 *W, int B, int F, int T, int algorithm,
                              int holonomic, double eta, int floor_kind, double eps, int n_steps,
                              double *loss, double *logdet, long long slot_stride, int *info,
                              hipStream_t st) {
  const dim3 grid((unsigned)F, (unsigned)B), block(FDICA_THREADS);
  if (fdica_resident(N, T))
    hipLaunchKernelGGL((k_fdica_steps<N, true>), grid, block, (size_t)N * T * sizeof(c128), st, X, W,
                       B, F, T, algorithm, holonomic, eta, floor_kind, eps, n_steps, loss, logdet,
                       slot_stride, info);
  else
    hipLaunchKernelGGL((k_fdica_steps<N, false>), grid, block, 0, st, X, W, B, F, T, algorithm,
                       holonomic, eta, floor_kind, eps, n_steps, loss, logdet, slot_stride, info);
  return check_launch("k_fdica_steps");
}

}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_fdica_weight(const void *Y, double *weight, int B, int S, int F, int T, int aux_form,
                       int floor_kind, double floor_eps, double *contrast,
                       long long contrast_stride, void *stream) {
  SSSPY_REQUIRE(Y && (weight || contrast) && B > 0 && B <= 65535 && S > 0 && F > 0 && T > 0,
                "fdica_weight: bad argument");
  SSSPY_REQUIRE(!contrast || contrast_stride >= B, "fdica_weight: bad contrast stride");
  hipLaunchKernelGGL(k_fdica_weight, dim3((unsigned)F, (unsigned)B), dim3(256), 0, as_stream(stream),
                     (const c128 *)Y, weight, S, F, T, aux_form ? 1 : 0, floor_kind, floor_eps,
                     contrast, contrast_stride);
  return check_launch("k_fdica_weight");
}

int ssspy_fdica_route(int B, int N, int F, int T, int algorithm) {
  if (B <= 0 || N < 1 || F <= 0 || T <= 0 || algorithm < SSSPY_FDICA_GRAD ||
      algorithm > SSSPY_FDICA_AUX_IP2)
    return -1;
  // Measured (profiles/fdica.txt): at 2..4 sources an iteration in the kernel takes 0.23 .. 0.9 of the
  // per-iteration operators' time, resident or streaming; at 6 and 8 sources (the 8-lane groups:
  // 256 VGPRs + AGPRs, one wave per SIMD) 1.3 .. 4.9 times as long on either route.  So 5..8 sources
  // take the operators; the kernel stays callable there (ssspy_fdica_steps) but nothing routes to it.
  if (N < 2 || N > FDICA_ROUTED_SOURCES || B > 65535 || algorithm == SSSPY_FDICA_AUX_IP2)
    return SSSPY_FDICA_ROUTE_COMPOSED;
  return fdica_resident(N, T) ? SSSPY_FDICA_ROUTE_RESIDENT : SSSPY_FDICA_ROUTE_STREAMING;
}

int ssspy_fdica_steps(const void *X, void *W, int B, int N, int F, int T, int algorithm,
                      int holonomic, double step_size, int floor_kind, double floor_eps,
                      int n_steps, double *loss_data, double *logdet, long long slot_stride,
                      int *info, void *stream) {
  SSSPY_REQUIRE(X && W && X != W && B > 0 && F > 0 && T > 0 && n_steps >= 1,
                "fdica_steps: bad argument");
  SSSPY_REQUIRE((!loss_data && !logdet) ||
                    (loss_data && logdet && slot_stride >= ((long long)n_steps + 1) * B),
                "fdica_steps: loss_data and logdet come together, slot_stride >= (n_steps + 1) B");
  if (N < 2 || N > SSSPY_MAX_SOURCES || B > 65535 || algorithm < SSSPY_FDICA_GRAD ||
      algorithm > SSSPY_FDICA_AUX_IP1)
    return fail(SSSPY_ERR_UNSUPPORTED,
                "fdica_steps: 2..8 sources, up to 65535 mixtures, gradient, natural gradient or IP1");
  DISPATCH_N(N, return launch_fdica_steps<NN>((const c128 *)X, (c128 *)W, B, F, T, algorithm,
                                              holonomic ? 1 : 0, step_size, floor_kind, floor_eps,
                                              n_steps, loss_data, logdet, slot_stride, info,
                                              as_stream(stream)));
  return SSSPY_OK;
}

}  // extern "C"
