// FastIVA / FasterIVA (fixed-point IVA on the whitened mixture) and the whitening / PCA filter.
//   FastIVA:   w_in <- mean_j phi_nj (w_in - y*_inj z_ij) - (mean_j psi_nj |y_inj|^2) w_in, then
//              W_i <- (W_i W_i^H)^-1/2 W_i                       (ssspy/bss/iva.py:1182-1207)
//   FasterIVA: row n of W_i <- conj of the principal eigenvector of U_in = mean_j phi_nj z z^H, then
//              the same orthonormalisation                        (ssspy/bss/iva.py:1383-1400)
//   whiten / pca: P_i = Lambda^-1/2 V^H resp. V^H of C_i = V Lambda V^H
//                                                  (ssspy/transform/whiten.py, ssspy/transform/pca.py)
// mean_j phi_nj y*_inj z_ij = U_in w_in, so FastIVA needs no N covariances per bin: one pass over
// Z leaves c_in = sum_j phi_nj y*_inj z_ij (an M-vector), b_in = sum_j psi_nj |y_inj|^2 and
// a_n = sum_j phi_nj; y = W z lives in registers only.
// fp64 / complex128, no fp64 atomics, every sum in a fixed order: the same bits on every run.
//
// One source for every source count: NC > 0 compiles the count in (2..8: the working set of a lane
// is indexed by constants and sits in registers; Jacobi unrolled up to 6 x 6, rolled for 7, 8 as in
// hermitian.hpp), NC == 0 takes it at run time (9..16, matrices in the lane's private memory as in
// grad_iva.hip -- correct, not tuned).
#include "common.hpp"
#include "hermitian.hpp"
#include "rt_dense.hpp"

namespace ssspy {

namespace {

template <int NC>
constexpr int fi_cap() {
  return NC ? NC : RTN;
}
// sources a block of the statistics pass takes
template <int NC>
constexpr int fi_group() {
  return NC == 0 ? RTN : (NC <= 4 ? NC : (NC <= 6 ? 3 : 2));
}

// The dimension descriptor (hermitian.hpp) of a source count, for the routines on the flat row-major
// matrices of a lane; the Jacobi sweeps are rolled (a call, the matrix in private memory) at 7 and 8.
// Every lane of the wave must be in a call of jacobi (the sweep loop ends on a wave vote).
template <int NC>
__device__ __forceinline__ auto fi_dim(int N) {
  if constexpr (NC == 0) return Runtime{N};
  else return Fixed<NC>{};
}
template <int NC>
__device__ __forceinline__ auto fi_jacobi_dim(int N) {
  if constexpr (NC == 0) return Runtime{N};
  else return Fixed<NC, (NC > 6)>{};
}

// W <- (W W^H)^-1/2 W, the unitary polar factor u v^H of W = u s v^H (ssspy/bss/iva.py:1204-1205,
// :1397-1398).  false: W W^H is singular to working precision (smallest eigenvalue not above 1e-14 of
// the largest) or not finite -- the reference's SVD returns some unitary matrix there, here the
// caller counts the bin in info[0].
constexpr double FI_SINGULAR = 1e-14;

template <int NC>
__device__ __forceinline__ bool fi_orthonormalize(c128 *W, int N) {
  constexpr int C = fi_cap<NC>();
  c128 G[C * C], P[C * C], S[C * C];
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = r; c < N; ++c) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < N; ++k) cfma(s, W[r * N + k], cconj(W[c * N + k]));
      if (r == c) s.y = 0.0;
      G[r * N + c] = s;
      G[c * N + r] = cconj(s);
    }
  jacobi(fi_jacobi_dim<NC>(N), G, P);
  double w[C];
  double lmin = G[0].x, lmax = G[0].x;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double lam = G[k * N + k].x;
    lmin = lam < lmin ? lam : lmin;
    lmax = lam > lmax ? lam : lmax;
    w[k] = lam > 0.0 ? 1.0 / sqrt(lam) : 0.0;
  }
  // (spelt so that a NaN anywhere fails it)
  const bool ok = (lmin > FI_SINGULAR * lmax) && (lmax < 1.79e308) && (lmin == lmin);
#pragma unroll
  for (int a = 0; a < N; ++a)
#pragma unroll
    for (int b = a; b < N; ++b) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const c128 t = cmulc(P[a * N + k], P[b * N + k]);
        s.x = fma(w[k], t.x, s.x);
        s.y = fma(w[k], t.y, s.y);
      }
      if (a == b) s.y = 0.0;
      S[a * N + b] = s;
      S[b * N + a] = cconj(s);
    }
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < N; ++k) cfma(s, S[r * N + k], W[k * N + c]);
      G[r * N + c] = s;
    }
  // One Newton-Schulz step, V <- V - (V V^H - I) V / 2.  Forming W W^H squares the conditioning of
  // W, so V V^H is I only to eps cond(W W^H) (4e-11 at 1e6); the step squares that distance.
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = r; c < N; ++c) {
      c128 s = cmake(r == c ? -1.0 : 0.0, 0.0);
#pragma unroll
      for (int k = 0; k < N; ++k) cfma(s, G[r * N + k], cconj(G[c * N + k]));
      if (r == c) s.y = 0.0;
      S[r * N + c] = s;
      S[c * N + r] = cconj(s);
    }
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < N; ++k) cfma(s, S[r * N + k], G[k * N + c]);
      W[r * N + c] = cmake(fma(-0.5, s.x, G[r * N + c].x), fma(-0.5, s.y, G[r * N + c].y));
    }
  return ok;
}

// a lane past the end works on the last item (every lane is in the wave votes of the Jacobi sweeps)
// and writes nothing
struct FiLane {
  long long idx;
  bool live;
};
__device__ __forceinline__ FiLane fi_lane(long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  return FiLane{i < n ? i : n - 1, i < n};
}

// ---- phi = G'(r) / floor(2 r), psi = (2 phi - G''(r)) / floor(2 r) from the frame powers and the
// closures' values on the norms (ssspy/bss/iva.py:1187-1188, :1196, :1390-1391)
__global__ __launch_bounds__(256) void k_fast_weights(const double *__restrict__ r2,
                                                      const double *__restrict__ g1,
                                                      const double *__restrict__ g2, double *phi,
                                                      double *psi, long long total, int floor_kind,
                                                      double eps) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const double d = apply_floor(2.0 * sqrt(r2[e]), floor_kind, eps);
  const double p = g1[e] / d;
  phi[e] = p;
  if (psi) psi[e] = (2.0 * p - (g2 ? g2[e] : 0.0)) / d;
}

// ---- the statistics pass of FastIVA.  The bin-major tile of cov_core.hpp: lane = q * 16 + c, c a
// bin of a tile of 16 consecutive bins, q one of 4 frame sub-groups; in a step lane (c, q) owns the 4
// consecutive frames j0 + 4 q + {0..3} of bin i0 + c, 64 contiguous bytes of every channel row.  A
// lane accumulates the statistics of ONE bin over its frames privately; the four waves of a block
// take a quarter of the frames each.  Folds: q by two shuffles, the waves through LDS in wave order.
// The filters of the tile are staged in LDS as [element][bin] (compiled counts; at run time they are
// read through the cache).  Frames past the end contribute phi = psi = 0 on a clamped address.
// From 5 compiled sources on a block takes a group of NS sources (blockIdx.z; 3 at 5, 6 sources, 2 at
// 7, 8): all N x N complex accumulators of a lane plus the filter rows the compiler keeps beside them
// spilled 208 .. 1588 bytes per lane inside the frame loop; a group's NS x N do not spill, at the
// price of reading Z once per group (2 .. 4 times, the groups of a tile running side by side).
// grid: (ceil(F / 16), B, ceil(N / NS)), 256 threads; dynamic LDS: fast_stats_lds_bytes()
template <int NC>
__global__ __launch_bounds__(256) void k_fast_stats(const c128 *__restrict__ Z,
                                                    const c128 *__restrict__ W,
                                                    const double *__restrict__ phi,
                                                    const double *__restrict__ psi, c128 *cst,
                                                    double *bst, double *ast, int N_, int F, int T) {
  constexpr int C = fi_cap<NC>();
  constexpr int NS = fi_group<NC>();
  const int N = NC ? NC : N_;
  const int n0 = blockIdx.z * NS;           // first source of this block's group
  const int ns = min(NS, N - n0);           // sources in it
  extern __shared__ double fi_lds[];
  double *Wl = fi_lds;                                  // [2 N N][16] (compiled counts only)
  double *fold = fi_lds + (NC ? 2 * N * N * 16 : 0);    // [4 waves][2 N + 2][16]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int b = blockIdx.y;
  const int i0 = blockIdx.x * 16;
  const int ic = min(i0 + c, F - 1);
  if constexpr (NC != 0) {
    for (int e = threadIdx.x; e < N * N * 16; e += 256) {
      const int cb = e & 15, el = e >> 4;
      const c128 w = W[((long long)b * F + min(i0 + cb, F - 1)) * (N * N) + el];
      Wl[(2 * el) * 16 + cb] = w.x;
      Wl[(2 * el + 1) * 16 + cb] = w.y;
    }
    __syncthreads();
  }
  const c128 *Wg = W + ((long long)b * F + ic) * (long long)(N * N);
  const int Tq = (T + 3) >> 2;
  const int jb = wave * Tq, je = min(T, jb + Tq);
  c128 acc[NS * C];
  double bb[NS], aa[NS];
#pragma unroll
  for (int e = 0; e < NS * C; ++e) acc[e] = cmake(0.0, 0.0);
#pragma unroll
  for (int k = 0; k < NS; ++k) bb[k] = aa[k] = 0.0;
  for (int j0 = jb; j0 < je; j0 += 16) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + 4 * q + u;
      const bool valid = j < je;
      const int jc = min(j, T - 1);
      c128 z[C];
#pragma unroll
      for (int m = 0; m < N; ++m) z[m] = Z[(((long long)b * N + m) * F + ic) * T + jc];
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        // (a group's sources past the last one repeat it with zero weights and store nothing)
        const bool mine = k < ns;
        const int n = n0 + (mine ? k : ns - 1);
        c128 y = cmake(0.0, 0.0);
#pragma unroll
        for (int m = 0; m < N; ++m) {
          c128 w;
          if constexpr (NC != 0)
            w = cmake(Wl[(2 * (n * N + m)) * 16 + c], Wl[(2 * (n * N + m) + 1) * 16 + c]);
          else
            w = Wg[n * N + m];
          cfma(y, w, z[m]);
        }
        const long long e = ((long long)b * N + n) * T + jc;
        const double p = (valid && mine) ? phi[e] : 0.0;
        const double s = (valid && mine && psi) ? psi[e] : 0.0;
        aa[k] += p;
        bb[k] = fma(s, cabs2(y), bb[k]);
        const c128 t = cmake(p * y.x, -p * y.y);  // phi y*
#pragma unroll
        for (int m = 0; m < N; ++m) cfma(acc[k * C + m], t, z[m]);
      }
    }
  }
  // the four frame sub-groups of a bin
#pragma unroll
  for (int k = 0; k < NS; ++k) {
#pragma unroll
    for (int m = 0; m < N; ++m) {
      double vx = acc[k * C + m].x, vy = acc[k * C + m].y;
      vx += __shfl_xor(vx, 16, 64);
      vx += __shfl_xor(vx, 32, 64);
      vy += __shfl_xor(vy, 16, 64);
      vy += __shfl_xor(vy, 32, 64);
      acc[k * C + m] = cmake(vx, vy);
    }
    double v = bb[k];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    bb[k] = v;
    v = aa[k];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    aa[k] = v;
  }
  // the waves, one source at a time: [wave][value][bin], values 2 N of c_n, then b_n, a_n
  const int V = 2 * N + 2;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    if (k >= ns) break;  // (uniform over the block)
    const int n = n0 + k;
    __syncthreads();
    if (q == 0) {
      double *mine = fold + (size_t)wave * V * 16;
#pragma unroll
      for (int m = 0; m < N; ++m) {
        mine[(2 * m) * 16 + c] = acc[k * C + m].x;
        mine[(2 * m + 1) * 16 + c] = acc[k * C + m].y;
      }
      mine[(2 * N) * 16 + c] = bb[k];
      mine[(2 * N + 1) * 16 + c] = aa[k];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < V * 16; t += 256) {
      const int cb = t & 15, v = t >> 4;
      const int bin = i0 + cb;
      if (bin >= F) continue;
      const double s = ((fold[(0 * V + v) * 16 + cb] + fold[(1 * V + v) * 16 + cb]) +
                        fold[(2 * V + v) * 16 + cb]) + fold[(3 * V + v) * 16 + cb];
      const long long row = ((long long)b * F + bin) * N + n;
      if (v < 2 * N) ((double *)cst)[row * N * 2 + v] = s;
      else if (v == 2 * N) bst[row] = s;
      else ast[row] = s;
    }
  }
}

static size_t fast_stats_lds_bytes(int N, bool staged) {
  return ((staged ? (size_t)2 * N * N * 16 : 0) + (size_t)4 * (2 * N + 2) * 16) * sizeof(double);
}

// ---- per-bin steps, a lane per bin.  cst != nullptr: the FastIVA update from the moments first
//   row n of W <- ((a_n - b_n) / T) w_n - conj(c_n) / T
// (w_in of the reference is column n of W_i^H, so the row is its conjugate), then the rows are
// orthonormalised.  cst == nullptr: the orthonormalisation alone.
template <int NC>
__global__ __launch_bounds__(64) void k_fast_step(c128 *W, const c128 *__restrict__ cst,
                                                  const double *__restrict__ bst,
                                                  const double *__restrict__ ast, long long nbins,
                                                  int N_, double inv_T, int *info) {
  constexpr int C = fi_cap<NC>();
  const int N = NC ? NC : N_;
  const FiLane ln = fi_lane(nbins);
  c128 Wm[C * C];
#pragma unroll
  for (int e = 0; e < N * N; ++e) Wm[e] = W[ln.idx * (N * N) + e];
  if (cst) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
      const double s = (ast[ln.idx * N + n] - bst[ln.idx * N + n]) * inv_T;
#pragma unroll
      for (int m = 0; m < N; ++m) {
        const c128 cc = cst[(ln.idx * N + n) * N + m];
        Wm[n * N + m] = cmake(fma(s, Wm[n * N + m].x, -inv_T * cc.x),
                              fma(s, Wm[n * N + m].y, inv_T * cc.y));
      }
    }
  }
  const bool ok = fi_orthonormalize<NC>(Wm, N);
  if (!ln.live) return;
#pragma unroll
  for (int e = 0; e < N * N; ++e) W[ln.idx * (N * N) + e] = Wm[e];
  if (!ok && info) atomicAdd(info, 1);
}

// ---- FasterIVA, a lane per (bin, source): row n of W_i <- conj of the eigenvector of the largest
// eigenvalue of U_in (the first one on ties).  The phase of the eigenvector is the decomposition's,
// as with LAPACK arbitrary: it moves row n by a unit factor, which the orthonormalisation keeps and
// every quantity the algorithm defines (norms, loss, restored output) is blind to.
template <int NC>
__global__ __launch_bounds__(64) void k_principal_rows(c128 *W, const c128 *__restrict__ U,
                                                       long long nrows, int N_, int *info) {
  constexpr int C = fi_cap<NC>();
  const int N = NC ? NC : N_;
  const FiLane ln = fi_lane(nrows);
  c128 A[C * C], P[C * C];
#pragma unroll
  for (int e = 0; e < N * N; ++e) A[e] = U[ln.idx * (N * N) + e];
  hermitize(fi_dim<NC>(N), A);
  jacobi(fi_jacobi_dim<NC>(N), A, P);
  int best = 0;
  double lbest = A[0].x;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double lam = A[k * N + k].x;
    finite = finite && (fabs(lam) < 1.79e308);
    if (lam > lbest) {
      lbest = lam;
      best = k;
    }
  }
  if (!ln.live) return;
#pragma unroll
  for (int m = 0; m < N; ++m) {
    c128 v = cmake(0.0, 0.0);
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (k == best) v = P[m * N + k];
    W[ln.idx * N + m] = cconj(v);
  }
  if (!finite && info) atomicAdd(info, 1);
}

// ---- whitening / PCA filter, a lane per bin: C = V Lambda V^H (eigenvalues ascending, ties by
// index), row k of P = scale_k conj(column k of V):
//   mode 0 (whiten): scale = Lambda^-1/2, ascending          (ssspy/transform/whiten.py:55-61)
//   mode 1 (pca, ascend=False): scale = 1, ascending         (ssspy/transform/pca.py:57-64)
//   mode 2 (pca, ascend=True):  scale = 1, descending
// A non-finite eigenvalue, or for whiten one that is not positive, bumps info[0] (the reference
// returns inf / nan there).
template <int NC>
__global__ __launch_bounds__(64) void k_whitening_filter(const c128 *__restrict__ Cm, c128 *Pout,
                                                         long long nbins, int N_, int mode,
                                                         int *info) {
  constexpr int C = fi_cap<NC>();
  const int N = NC ? NC : N_;
  const FiLane ln = fi_lane(nbins);
  c128 A[C * C], P[C * C];
#pragma unroll
  for (int e = 0; e < N * N; ++e) A[e] = Cm[ln.idx * (N * N) + e];
  hermitize(fi_dim<NC>(N), A);
  jacobi(fi_jacobi_dim<NC>(N), A, P);
  if (!ln.live) return;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double lk = A[k * N + k].x;
    int rank = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double lj = A[j * N + j].x;
      rank += (lj < lk || (lj == lk && j < k)) ? 1 : 0;
    }
    ok = ok && (fabs(lk) < 1.79e308) && (mode != 0 || lk > 0.0);
    const double scale = mode == 0 ? 1.0 / sqrt(lk) : 1.0;
    const int row = mode == 2 ? N - 1 - rank : rank;
#pragma unroll
    for (int m = 0; m < N; ++m) {
      const c128 v = P[m * N + k];
      Pout[ln.idx * (N * N) + row * N + m] = cmake(scale * v.x, -scale * v.y);
    }
  }
  if (!ok && info) atomicAdd(info, 1);
}

// switch on a run-time source count: 2..8 compiled in, 9..16 at run time
#define FI_DISPATCH(N_, CALL)                      \
  switch (N_) {                                    \
    case 2: { constexpr int NN = 2; CALL; } break; \
    case 3: { constexpr int NN = 3; CALL; } break; \
    case 4: { constexpr int NN = 4; CALL; } break; \
    case 5: { constexpr int NN = 5; CALL; } break; \
    case 6: { constexpr int NN = 6; CALL; } break; \
    case 7: { constexpr int NN = 7; CALL; } break; \
    case 8: { constexpr int NN = 8; CALL; } break; \
    default: { constexpr int NN = 0; CALL; } break; \
  }

inline dim3 fi_lanes(long long n) { return dim3((unsigned)((n + 63) / 64)); }

int fi_check_sources(int N, const char *what) {
  if (N < 2 || N > SSSPY_RT_MAX_SOURCES) {
    std::snprintf(g_last_error, sizeof(g_last_error), "%s: 2 to %d sources, got %d", what,
                  SSSPY_RT_MAX_SOURCES, N);
    return SSSPY_ERR_UNSUPPORTED;
  }
  return SSSPY_OK;
}

}  // namespace

}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_fast_iva_weights(const double *r2, const double *d_contrast, const double *dd_contrast,
                           double *phi, double *psi, int B, int N, int T, int floor_kind,
                           double floor_eps, void *stream) {
  SSSPY_REQUIRE(r2 && d_contrast && phi && B > 0 && N > 0 && T > 0, "fast_iva_weights: bad argument");
  const long long total = (long long)B * N * T;
  hipLaunchKernelGGL(k_fast_weights, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     as_stream(stream), r2, d_contrast, dd_contrast, phi, psi, total, floor_kind,
                     floor_eps);
  return check_launch("k_fast_weights");
}

int ssspy_fast_iva_stats(const void *Z, const void *W, const double *phi, const double *psi,
                         void *c, double *b, double *a, int B, int N, int F, int T, void *stream) {
  SSSPY_REQUIRE(Z && W && phi && psi && c && b && a && B > 0 && B <= 65535 && F > 0 && T > 0,
                "fast_iva_stats: bad argument");
  if (int rc = fi_check_sources(N, "fast_iva_stats")) return rc;
  FI_DISPATCH(N, const dim3 grid((unsigned)((F + 15) / 16), (unsigned)B,
                                 (unsigned)((N + fi_group<NN>() - 1) / fi_group<NN>()));
              const dim3 block(256);
              hipLaunchKernelGGL((k_fast_stats<NN>), grid, block,
                                    fast_stats_lds_bytes(N, NN != 0), as_stream(stream),
                                    (const c128 *)Z, (const c128 *)W, phi, psi, (c128 *)c, b, a, N,
                                    F, T));
  return check_launch("k_fast_stats");
}

int ssspy_fast_iva_step(void *W, const void *c, const double *b, const double *a, int B, int F,
                        int N, int T, int *info, void *stream) {
  SSSPY_REQUIRE(W && c && b && a && B > 0 && F > 0 && T > 0, "fast_iva_step: bad argument");
  if (int rc = fi_check_sources(N, "fast_iva_step")) return rc;
  const long long nbins = (long long)B * F;
  FI_DISPATCH(N, hipLaunchKernelGGL((k_fast_step<NN>), fi_lanes(nbins), dim3(64), 0,
                                    as_stream(stream), (c128 *)W, (const c128 *)c, b, a, nbins, N,
                                    1.0 / (double)T, info));
  return check_launch("k_fast_step");
}

int ssspy_orthonormalize_rows(void *W, int B, int F, int N, int *info, void *stream) {
  SSSPY_REQUIRE(W && B > 0 && F > 0, "orthonormalize_rows: bad argument");
  if (int rc = fi_check_sources(N, "orthonormalize_rows")) return rc;
  const long long nbins = (long long)B * F;
  FI_DISPATCH(N, hipLaunchKernelGGL((k_fast_step<NN>), fi_lanes(nbins), dim3(64), 0,
                                    as_stream(stream), (c128 *)W, (const c128 *)nullptr,
                                    (const double *)nullptr, (const double *)nullptr, nbins, N, 0.0,
                                    info));
  return check_launch("k_fast_step (orthonormalize)");
}

int ssspy_faster_iva_step(void *W, const void *U, int B, int F, int N, int *info, void *stream) {
  SSSPY_REQUIRE(W && U && W != U && B > 0 && F > 0, "faster_iva_step: bad argument");
  if (int rc = fi_check_sources(N, "faster_iva_step")) return rc;
  const long long nrows = (long long)B * F * N;
  FI_DISPATCH(N, hipLaunchKernelGGL((k_principal_rows<NN>), fi_lanes(nrows), dim3(64), 0,
                                    as_stream(stream), (c128 *)W, (const c128 *)U, nrows, N, info));
  if (int rc = check_launch("k_principal_rows")) return rc;
  return ssspy_orthonormalize_rows(W, B, F, N, info, stream);
}

int ssspy_whitening_filter(const void *C, void *P, int B, int F, int N, int mode, int *info,
                           void *stream) {
  SSSPY_REQUIRE(C && P && C != P && B > 0 && F > 0 && mode >= 0 && mode <= 2,
                "whitening_filter: bad argument");
  if (int rc = fi_check_sources(N, "whitening_filter")) return rc;
  const long long nbins = (long long)B * F;
  FI_DISPATCH(N, hipLaunchKernelGGL((k_whitening_filter<NN>), fi_lanes(nbins), dim3(64), 0,
                                    as_stream(stream), (const c128 *)C, (c128 *)P, nbins, N, mode,
                                    info));
  return check_launch("k_whitening_filter");
}

}  // extern "C"
