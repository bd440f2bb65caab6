// Mask-based beamformers (MVDR, GEV, MWF): the bin-resident kernel.
//   Souden, Benesty, Affes, "On optimal frequency-domain multichannel linear filtering for noise
//   reduction", IEEE TASLP 18(2), 2010 (MVDR, eq. 18, and the speech-distortion-weighted MWF, eq. 16);
//   Warsitz, Haeb-Umbach, "Blind acoustic beamforming based on generalized eigenvalue decomposition",
//   IEEE TASLP 15(5), 2007 (GEV, eq. 12, and the blind analytic normalisation, eq. 30);
//   Higuchi et al., ICASSP 2016 / Heymann et al., ICASSP 2016 (masks as covariance weights).
//
// Per bin, with x_t in C^M the frame, m_nt >= 0 the mask of source n and u_nt its noise weight (the
// noise mask, or 1 - m_nt formed here):
//   S_n = sum_t m_nt x_t x_t^H, a_n = sum_t m_nt, N_n = sum_t u_nt x_t x_t^H, b_n = sum_t u_nt
//   Phi_s = S_n / max(a_n, eps), Phi_v = N_n / max(b_n, eps) + loading (tr(N_n / max(b_n, eps)) / M) I
//   MVDR  A = Phi_v^-1 Phi_s (Cholesky), w = A e_ref / max(Re tr A, eps)
//   MWF   w = (Phi_s + mu Phi_v)^-1 Phi_s e_ref
//   GEV   Phi_v = L L^H, C = L^-1 Phi_s L^-H, v its principal unit eigenvector (Jacobi), w0 = L^-H v,
//         a = L v; w = w0 conj(a_ref) ("reference") or w0 p ||a|| / sqrt(M), p = conj(a_ref) / |a_ref|
//         ("ban"; p = 1 where a_ref = 0)
//   y_nt = w_n^H x_t; the filter is stored as the row w_n^H (demix_filter[f, n, :]).
// A Phi_s that is zero in every entry (an all-zero mask) gives w = 0.
//
// The bins never talk to each other (the model of csrc/wpe.hip): a workgroup of 256 threads owns one
// (mixture, bin).  The frames go in tiles of BF_TILE through LDS; every thread owns up to NPT fixed
// (source, signal-or-noise, packed-triangle entry) sums -- at most 2 * 16 * 36 = 1152 over 256 threads
// -- and the sum of the weights of each, and walks the frames of a tile in frame order: no atomics,
// the same bits on every run and on both routes.  Then lane n of the first wave solves source n on
// matrices in LDS (the run-time-size routines of hermitian.hpp: nothing M x M in private memory), and
// the apply walk writes Y: thread tt, frame t0 + tt.
//
// LDS (dynamic; 160 KiB per CU decide the bounds), c128 = 16 bytes:
//   slab    RESIDENT: the bin's M rows of T frames, row stride T | 1 (odd: the rows of one frame fall
//           into different banks), where 16 M T <= BF_SLAB_LDS_BYTES = 48 KiB (the rule of wpe.hip): at
//           most 49280 bytes.  Otherwise one tile, M rows of stride 257: at most 32896 bytes.
//   work    the weights of a tile, 2 N rows of 256 doubles (65536 bytes at N = 16), and, once the sums
//           are done, IN THE SAME BYTES the four M x M matrices of every source (Phi_s, Phi_v -> L,
//           L^-1 and a product: 65536 bytes at M = 8, N = 16)
//   filter  N rows w_n^H: 2048 bytes
//   at most 49280 + 65536 + 2048 = 116864 bytes.
#include <cfloat>

#include "hermitian.hpp"

namespace ssspy {

constexpr int BF_THREADS = 256;
constexpr int BF_TILE = 256;  // frames per tile: one per thread in the staging and the apply walk
constexpr int BF_MAX_CHANNELS = 8;
constexpr int BF_MAX_SOURCES = 16;
constexpr int BF_SLAB_LDS_BYTES = 48 * 1024;
constexpr int BF_MAX_NPT =
    (2 * BF_MAX_SOURCES * (BF_MAX_CHANNELS * (BF_MAX_CHANNELS + 1) / 2) + BF_THREADS - 1) / BF_THREADS;
constexpr double BF_EPS = 1e-10;  // the project's EPS

// what a launch does
enum {
  BF_COVARIANCES = 0,  // the sums (raw or divided by max(weight sum, eps)) to memory, nothing else
  BF_RUN = 1,          // sums, Phi_s / Phi_v, the filters, Y
  BF_FILTER = 2,       // Phi_s and Phi_v from memory, the filters
  BF_APPLY = 3,        // the filters from memory, Y
};

struct BfArgs {
  const c128 *X;        // (B, M, F, T)
  const double *mask;   // (B, N, F, T)
  const double *noise;  // NULL: 1 - mask; (B, F, T) when noise_shared, else (B, N, F, T)
  c128 *W;              // (B, F, N, M), rows w_n^H: written, or read by BF_APPLY
  c128 *Y;              // (B, N, F, T)
  c128 *Cs, *Cv;        // (B, F, N, M, M): S_n, N_n / Phi_s, Phi_v; read by BF_FILTER
  double *a, *b;        // (B, F, N)
  int *info;
  double loading, mu;
  int B, M, N, F, T;
  int noise_shared, mode, normalize, kind, ref;
};

struct BfLds {
  size_t slab_bytes, work_bytes, filter_bytes;
  size_t total() const { return slab_bytes + work_bytes + filter_bytes; }
};
__host__ __device__ inline int bf_row_stride(int T, bool resident) {
  return resident ? (T | 1) : BF_TILE + 1;
}
__host__ __device__ inline size_t bf_work_elems(int M, int N) {
  const size_t stage = (size_t)N * BF_TILE;  // 2 N rows of BF_TILE doubles, in c128
  const size_t mats = (size_t)N * 4 * M * M;
  return stage > mats ? stage : mats;
}
static BfLds bf_lds(int M, int N, int T, bool resident, int mode) {
  BfLds s;
  s.slab_bytes = mode == BF_FILTER ? 0 : (size_t)M * bf_row_stride(T, resident) * sizeof(c128);
  s.work_bytes = bf_work_elems(M, N) * sizeof(c128);
  s.filter_bytes = (size_t)N * M * sizeof(c128);
  return s;
}
static bool bf_resident(int M, int T) {
  return (long long)M * (long long)T * (long long)sizeof(c128) <= BF_SLAB_LDS_BYTES;
}

// The filter of one source, by one lane, on M x M matrices in LDS: S = Phi_s and V = Phi_v (both
// full; destroyed), Li and T1 scratch.  wd (M) receives w^H.  False: a pivot of the Cholesky
// factorisation was not positive and finite (wd = 0).
__device__ __forceinline__ bool bf_filter_one(int M, c128 *S, c128 *V, c128 *Li, c128 *T1, int kind,
                                              int ref, double mu, c128 *wd) {
  const Runtime d{M};
  const int MM = M * M;
  bool zero = true;
  for (int e = 0; e < MM; ++e) zero = zero && S[e].x == 0.0 && S[e].y == 0.0;
  for (int m = 0; m < M; ++m) wd[m] = cmake(0.0, 0.0);
  bool ok = true;
  if (!zero) {
    if (kind == SSSPY_BEAMFORM_MWF)
      for (int e = 0; e < MM; ++e) V[e] = cadd(S[e], cscale(V[e], mu));
    ok = cholesky_lower(d, V);
    for (int c = 0; c < M; ++c) ok = ok && (V[c * M + c].x <= DBL_MAX);
  }
  const bool live = !zero && ok;
  if (live) {
    lower_inverse(d, V, Li);
    matmul(d, Li, S, T1);  // L^-1 Phi_s
  }
  if (live && (kind == SSSPY_BEAMFORM_MVDR || kind == SSSPY_BEAMFORM_MWF)) {
    matmul_hl(d, Li, T1, S);  // A = L^-H L^-1 Phi_s
    double den = 1.0;
    if (kind == SSSPY_BEAMFORM_MVDR) {
      double tr = 0.0;
      for (int c = 0; c < M; ++c) tr += S[c * M + c].x;
      den = tr < BF_EPS ? BF_EPS : tr;
    }
    for (int m = 0; m < M; ++m) {
      const c128 z = S[m * M + ref];
      wd[m] = cmake(z.x / den, -z.y / den);
    }
  }
  if (live && (kind == SSSPY_BEAMFORM_GEV_REFERENCE || kind == SSSPY_BEAMFORM_GEV_BAN)) {
    matmul_h(d, T1, Li, S);  // C = L^-1 Phi_s L^-H
    hermitize(d, S);
    jacobi(d, S, T1);  // the eigenvalues on the diagonal of S, the eigenvectors in the columns of T1
    int k = 0;
    for (int c = 1; c < M; ++c)
      if (S[c * M + c].x > S[k * M + k].x) k = c;
    // a = L v: its entry ref and its norm; w0 = L^-H v into wd
    c128 aref = cmake(0.0, 0.0);
    double norm2 = 0.0;
    for (int m = 0; m < M; ++m) {
      c128 am = cmake(0.0, 0.0), wm = cmake(0.0, 0.0);
      for (int r = 0; r <= m; ++r) cfma(am, V[m * M + r], T1[r * M + k]);
      for (int r = m; r < M; ++r) cfma(wm, cconj(Li[r * M + m]), T1[r * M + k]);
      norm2 += cabs2(am);
      if (m == ref) aref = am;
      wd[m] = wm;
    }
    c128 gain = cconj(aref);
    if (kind == SSSPY_BEAMFORM_GEV_BAN) {
      const double mag = sqrt(cabs2(aref));
      const double s = sqrt(norm2) / sqrt((double)M);
      gain = mag > 0.0 ? cmake(aref.x / mag * s, -aref.y / mag * s) : cmake(s, 0.0);
    }
    for (int m = 0; m < M; ++m) wd[m] = cconj(cmul(wd[m], gain));
  }
  return zero || ok;
}

// grid: (F, B), 256 threads; see BfArgs and the modes above.
template <int NPT, bool RESIDENT>
__global__ __launch_bounds__(BF_THREADS) void k_beamform(const BfArgs g) {
  extern __shared__ c128 lds[];
  const int tid = threadIdx.x;
  const int f = blockIdx.x, b = blockIdx.y;
  const int M = g.M, N = g.N, F = g.F, T = g.T, MM = M * M;
  const int HS = bf_row_stride(T, RESIDENT);
  c128 *xs = lds;
  c128 *work = xs + (g.mode == BF_FILTER ? 0 : M * HS);
  double *stage = reinterpret_cast<double *>(work);
  c128 *Wd = work + bf_work_elems(M, N);

  const long long row_stride = (long long)F * T;
  const long long bf = (long long)b * F + f;
  const c128 *__restrict__ Xb = g.X + ((long long)b * M * F + f) * T;  // row m at + m * row_stride

  if (g.mode == BF_APPLY) {
    for (int e = tid; e < N * M; e += BF_THREADS) Wd[e] = g.W[bf * N * M + e];
    __syncthreads();
  }
  if (RESIDENT && g.mode != BF_FILTER) {
    for (int m = 0; m < M; ++m)
      for (int j = tid; j < T; j += BF_THREADS) xs[m * HS + j] = Xb[m * row_stride + j];
    __syncthreads();
  }

  if (g.mode == BF_COVARIANCES || g.mode == BF_RUN) {
    const double *__restrict__ Mb = g.mask + ((long long)b * N * F + f) * T;
    const double *__restrict__ Nb =
        !g.noise ? nullptr
                 : (g.noise_shared ? g.noise + bf * T : g.noise + ((long long)b * N * F + f) * T);
    const long long noise_stride = g.noise_shared ? 0 : row_stride;
    // the sums this thread owns: entry e = (n * 2 + k) * ntri + tri, k = 0 signal / 1 noise, tri the
    // index of (p, q), p <= q, in the row-major upper triangle
    const int ntri = M * (M + 1) / 2, NE = 2 * N * ntri;
    int op[NPT], oq[NPT], orow[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      int e = tid + i * BF_THREADS;
      if (e >= NE) e = 0;  // (idle: shadows entry 0, never stores)
      int tri = e % ntri, p = 0;
      while (tri >= M - p) {
        tri -= M - p;
        ++p;
      }
      op[i] = p * HS;
      oq[i] = (p + tri) * HS;
      orow[i] = (e / ntri) * BF_TILE;
    }
    c128 acc[NPT];
    double wsum[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      acc[i] = cmake(0.0, 0.0);
      wsum[i] = 0.0;
    }
#pragma unroll 1
    for (int t0 = 0; t0 < T; t0 += BF_TILE) {
      const int nt = min(BF_TILE, T - t0);
      __syncthreads();  // the previous tile has been read
      if (!RESIDENT)
        for (int m = 0; m < M; ++m)
          for (int j = tid; j < nt; j += BF_THREADS) xs[m * HS + j] = Xb[m * row_stride + t0 + j];
      if (tid < nt) {
        for (int n = 0; n < N; ++n) {
          const double mk = Mb[n * row_stride + t0 + tid];
          stage[(2 * n) * BF_TILE + tid] = mk;
          stage[(2 * n + 1) * BF_TILE + tid] = Nb ? Nb[n * noise_stride + t0 + tid] : 1.0 - mk;
        }
      }
      __syncthreads();
      const c128 *xb = RESIDENT ? xs + t0 : xs;
#pragma unroll 1
      for (int tt = 0; tt < nt; ++tt) {
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
          const double w = stage[orow[i] + tt];
          cfmac(acc[i], cscale(xb[op[i] + tt], w), xb[oq[i] + tt]);
          wsum[i] += w;
        }
      }
    }
    __syncthreads();  // the weights of the last tile have been read: `work` becomes the matrices
    const bool raw = g.mode == BF_COVARIANCES && !g.normalize;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const int e = tid + i * BF_THREADS;
      if (e >= NE) continue;
      const int n = e / (2 * ntri), k = (e / ntri) & 1;
      int tri = e % ntri, p = 0;
      while (tri >= M - p) {
        tri -= M - p;
        ++p;
      }
      const int q = p + tri;
      c128 v = acc[i];
      if (!raw) {
        const double den = wsum[i] < BF_EPS ? BF_EPS : wsum[i];
        v = cmake(v.x / den, v.y / den);
      }
      if (p == q) v.y = 0.0;
      if (g.mode == BF_COVARIANCES) {
        c128 *out = (k ? g.Cv : g.Cs) + (bf * N + n) * MM;
        out[p * M + q] = v;
        if (p != q) out[q * M + p] = cconj(v);
        if (tri == 0 && p == 0) (k ? g.b : g.a)[bf * N + n] = wsum[i];
      } else {
        c128 *mat = work + (n * 4 + k) * MM;
        mat[p * M + q] = v;
        if (p != q) mat[q * M + p] = cconj(v);
      }
    }
    if (g.mode == BF_COVARIANCES) return;
    __syncthreads();
    if (tid < N && g.loading != 0.0) {
      c128 *V = work + (tid * 4 + 1) * MM;
      double tr = 0.0;
      for (int c = 0; c < M; ++c) tr += V[c * M + c].x;
      const double add = g.loading * (tr / (double)M);
      for (int c = 0; c < M; ++c) V[c * M + c].x += add;
    }
    __syncthreads();
    if (g.Cs && g.Cv) {
      for (int e = tid; e < 2 * N * MM; e += BF_THREADS) {
        const int n = e / (2 * MM), k = (e / MM) & 1, idx = e % MM;
        (k ? g.Cv : g.Cs)[(bf * N + n) * MM + idx] = work[(n * 4 + k) * MM + idx];
      }
      __syncthreads();  // before the factorisations overwrite them
    }
  }
  if (g.mode == BF_FILTER) {
    for (int e = tid; e < 2 * N * MM; e += BF_THREADS) {
      const int n = e / (2 * MM), k = (e / MM) & 1, idx = e % MM;
      work[(n * 4 + k) * MM + idx] = (k ? g.Cv : g.Cs)[(bf * N + n) * MM + idx];
    }
    __syncthreads();
  }
  if (g.mode == BF_RUN || g.mode == BF_FILTER) {
    if (tid < N) {
      c128 *S = work + (tid * 4) * MM;
      const bool ok =
          bf_filter_one(M, S, S + MM, S + 2 * MM, S + 3 * MM, g.kind, g.ref, g.mu, Wd + tid * M);
      if (!ok && g.info) atomicAdd(g.info, 1);
    }
    __syncthreads();
    if (g.W)
      for (int e = tid; e < N * M; e += BF_THREADS) g.W[bf * N * M + e] = Wd[e];
  }
  if (g.mode == BF_FILTER || !g.Y) return;

  // ---- the apply walk: thread tt, frame t0 + tt, y_n = sum_m conj(w_n[m]) x_m in channel order
#pragma unroll 1
  for (int t0 = 0; t0 < T; t0 += BF_TILE) {
    const int nt = min(BF_TILE, T - t0);
    if (!RESIDENT) {
      __syncthreads();  // the previous tile has been read
      for (int m = 0; m < M; ++m)
        for (int j = tid; j < nt; j += BF_THREADS) xs[m * HS + j] = Xb[m * row_stride + t0 + j];
      __syncthreads();
    }
    const c128 *xb = RESIDENT ? xs + t0 : xs;
    if (tid < nt) {
      c128 x[BF_MAX_CHANNELS];
#pragma unroll
      for (int c = 0; c < BF_MAX_CHANNELS; ++c) x[c] = c < M ? xb[c * HS + tid] : cmake(0.0, 0.0);
#pragma unroll 1
      for (int n = 0; n < N; ++n) {
        c128 y = cmake(0.0, 0.0);
#pragma unroll
        for (int c = 0; c < BF_MAX_CHANNELS; ++c)
          if (c < M) cfma(y, Wd[n * M + c], x[c]);
        g.Y[((long long)b * N + n) * row_stride + (long long)f * T + t0 + tid] = y;
      }
    }
  }
}

template <int NPT, bool RESIDENT>
static int launch_beamform_as(const BfArgs &g, size_t smem, hipStream_t st) {
  if (smem > 64 * 1024) {
    // (granted once per instantiation and device, not on every launch)
    static size_t granted[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (smem > granted[dev]) {
      hipError_t e = hipFuncSetAttribute((const void *)k_beamform<NPT, RESIDENT>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      if (e != hipSuccess) return fail(SSSPY_ERR_HIP, hipGetErrorString(e));
      granted[dev] = smem;
    }
  }
  hipLaunchKernelGGL((k_beamform<NPT, RESIDENT>), dim3((unsigned)g.F, (unsigned)g.B),
                     dim3(BF_THREADS), smem, st, g);
  return check_launch("k_beamform");
}

static int bf_check(int B, int M, int N, int F, int T, const char **why) {
  *why = nullptr;
  if (B <= 0 || F <= 0 || T <= 0 || M < 1 || N < 1) {
    *why = "beamform: bad argument (sizes positive)";
    return SSSPY_ERR_BADARG;
  }
  if (M > BF_MAX_CHANNELS || N > BF_MAX_SOURCES || B > 65535 || T > (1 << 30)) {
    *why = "beamform: 1..8 channels, 1..16 masks, up to 65535 mixtures";
    return SSSPY_ERR_UNSUPPORTED;
  }
  return SSSPY_OK;
}

static int launch_beamform(BfArgs g, int route, void *stream) {
  const char *why;
  const int rc = bf_check(g.B, g.M, g.N, g.F, g.T, &why);
  if (rc != SSSPY_OK) return fail(rc, why);
  SSSPY_REQUIRE(route >= SSSPY_BEAMFORM_ROUTE_AUTO && route <= SSSPY_BEAMFORM_ROUTE_STREAMING,
                "beamform: route is one of SSSPY_BEAMFORM_ROUTE_*");
  const bool sums = g.mode == BF_COVARIANCES || g.mode == BF_RUN;
  // only a launch that reads the slab twice (the sums, then the apply walk) gains from keeping it
  const bool resident = g.mode == BF_RUN && g.Y && route != SSSPY_BEAMFORM_ROUTE_STREAMING &&
                        bf_resident(g.M, g.T);
  const int npt =
      sums ? (2 * g.N * (g.M * (g.M + 1) / 2) + BF_THREADS - 1) / BF_THREADS : 1;
  const size_t smem = bf_lds(g.M, g.N, g.T, resident, g.mode).total();
  const hipStream_t st = as_stream(stream);
#define BF_CASE(NPT_)                                                           \
  case NPT_:                                                                    \
    return resident ? launch_beamform_as<NPT_, true>(g, smem, st)               \
                    : launch_beamform_as<NPT_, false>(g, smem, st)
  static_assert(BF_MAX_NPT == 5, "the cases below cover 1..BF_MAX_NPT sums per thread");
  switch (npt) {
    BF_CASE(1);
    BF_CASE(2);
    BF_CASE(3);
    BF_CASE(4);
    BF_CASE(5);
  }
#undef BF_CASE
  return fail(SSSPY_ERR_INTERNAL, "beamform: no kernel for this shape");
}

static int bf_check_kind(int M, int kind, int ref, double loading, double mu) {
  SSSPY_REQUIRE(kind >= SSSPY_BEAMFORM_MVDR && kind <= SSSPY_BEAMFORM_MWF,
                "beamform: kind is one of SSSPY_BEAMFORM_*");
  SSSPY_REQUIRE(ref >= 0 && ref < M, "beamform: 0 <= reference_id < n_channels");
  SSSPY_REQUIRE(loading >= 0.0 && loading <= DBL_MAX, "beamform: diagonal_loading >= 0");
  SSSPY_REQUIRE(kind != SSSPY_BEAMFORM_MWF || (mu > 0.0 && mu <= DBL_MAX), "beamform: mu > 0");
  return SSSPY_OK;
}

}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_beamform_route(int B, int M, int N, int F, int T, int *lds_bytes) {
  const char *why;
  if (bf_check(B, M, N, F, T, &why) != SSSPY_OK) return -1;
  const bool resident = bf_resident(M, T);
  if (lds_bytes) *lds_bytes = (int)bf_lds(M, N, T, resident, BF_RUN).total();
  return resident ? SSSPY_BEAMFORM_ROUTE_RESIDENT : SSSPY_BEAMFORM_ROUTE_STREAMING;
}

int ssspy_beamform_covariances(const void *X, const double *mask, const double *noise_mask,
                               int noise_shared, void *S, void *Nv, double *a, double *b, int B,
                               int M, int N, int F, int T, int normalize, void *stream) {
  SSSPY_REQUIRE(X && mask && S && Nv && a && b, "beamform_covariances: bad argument");
  BfArgs g = {};
  g.X = (const c128 *)X;
  g.mask = mask;
  g.noise = noise_mask;
  g.noise_shared = noise_shared != 0;
  g.Cs = (c128 *)S;
  g.Cv = (c128 *)Nv;
  g.a = a;
  g.b = b;
  g.B = B, g.M = M, g.N = N, g.F = F, g.T = T;
  g.mode = BF_COVARIANCES;
  g.normalize = normalize != 0;
  return launch_beamform(g, SSSPY_BEAMFORM_ROUTE_AUTO, stream);
}

int ssspy_beamform_filter(const void *Phi_s, const void *Phi_v, void *W, int B, int M, int N, int F,
                          int kind, int reference_id, double mu, int *info, void *stream) {
  SSSPY_REQUIRE(Phi_s && Phi_v && W, "beamform_filter: bad argument");
  const int rc = bf_check_kind(M, kind, reference_id, 0.0, mu);
  if (rc != SSSPY_OK) return rc;
  BfArgs g = {};
  g.Cs = (c128 *)const_cast<void *>(Phi_s);
  g.Cv = (c128 *)const_cast<void *>(Phi_v);
  g.W = (c128 *)W;
  g.info = info;
  g.mu = mu;
  g.B = B, g.M = M, g.N = N, g.F = F, g.T = 1;
  g.mode = BF_FILTER;
  g.kind = kind;
  g.ref = reference_id;
  return launch_beamform(g, SSSPY_BEAMFORM_ROUTE_AUTO, stream);
}

int ssspy_beamform_run(const void *X, const double *mask, const double *noise_mask, int noise_shared,
                       void *W, void *Y, void *Phi_s, void *Phi_v, int B, int M, int N, int F, int T,
                       int kind, int reference_id, double diagonal_loading, double mu, int *info,
                       int route, void *stream) {
  SSSPY_REQUIRE(X && mask && X != Y && (W || Y || Phi_s) && !Phi_s == !Phi_v,
                "beamform_run: bad argument");
  const int rc = bf_check_kind(M, kind, reference_id, diagonal_loading, mu);
  if (rc != SSSPY_OK) return rc;
  BfArgs g = {};
  g.X = (const c128 *)X;
  g.mask = mask;
  g.noise = noise_mask;
  g.noise_shared = noise_shared != 0;
  g.W = (c128 *)W;
  g.Y = (c128 *)Y;
  g.Cs = (c128 *)Phi_s;
  g.Cv = (c128 *)Phi_v;
  g.info = info;
  g.loading = diagonal_loading;
  g.mu = mu;
  g.B = B, g.M = M, g.N = N, g.F = F, g.T = T;
  g.mode = BF_RUN;
  g.kind = kind;
  g.ref = reference_id;
  return launch_beamform(g, route, stream);
}

int ssspy_beamform_apply(const void *X, const void *W, void *Y, int B, int M, int N, int F, int T,
                         void *stream) {
  SSSPY_REQUIRE(X && W && Y && X != Y, "beamform_apply: bad argument");
  BfArgs g = {};
  g.X = (const c128 *)X;
  g.W = (c128 *)const_cast<void *>(W);
  g.Y = (c128 *)Y;
  g.B = B, g.M = M, g.N = N, g.F = F, g.T = T;
  g.mode = BF_APPLY;
  return launch_beamform(g, SSSPY_BEAMFORM_ROUTE_AUTO, stream);
}

}  // extern "C"
