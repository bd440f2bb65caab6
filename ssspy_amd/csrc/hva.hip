// Harmonic vector analysis (MaskingPDSHVA / HVA): the cosine-shrinkage mask on the cepstrum inside
// the dual step of MaskingPDSBSS.  ref: ssspy/bss/hva.py:91-115 with ssspy/bss/pdsbss.py:396-412.
//
// Two passes after the contraction and the filter step of pdsbss.hip; no spectrogram-sized complex
// mask is ever stored:
//   k_hva_cepstrum:  per (mixture, source, tile of frames) Z = dual + W2 x, zeta = log floor(|Z|),
//     the mean over bins m, rho = zeta - m, nu = D(rho) / (2 (F - 1)), sigma = min(1, nu) through
//     mask_iter cosine shrinkages, varrho = D(sigma nu) + m (B,N,F,T) real.  D is the DCT-I along
//     the bins (both irfft calls of the reference on a real length-F input).  The F x tile slab of
//     the source sits in LDS; loads and stores run along T.
//   k_hva_dual_step: per (b, f, t) Z again, the mask as a softmax over sources with the maximum
//     subtracted, Yt = Z - mask Z and the relaxation of the dual variable.
// MaskingADMMHVA (ref: ssspy/bss/hva.py:202-236 with ssspy/bss/admmbss.py:415-442) runs the same two
// passes after the contraction and the filter step of admmbss.hip, on ADMM's operand
// Z = relaxation W x + (1 - relaxation) auxiliary2 + dual2 (auxiliary2 is not read at relaxation 1):
//   k_hva_cepstrum with the other Z former (HvaAdmmZ in the place of HvaPdsZ), one body;
//   k_hva_aux_step: per (b, f, t) Z again, the same mask, auxiliary2 <- mask Z and
//     dual2 <- Z - auxiliary2 in place, both from the registers that hold Z.
// D by one of two routes (hva_plan):
//   FFT    F - 1 = M a power of two: the even extension of length L = 2 M of TWO frames as the real
//          and the imaginary part of one complex sequence; its DFT is D(frame a) + i D(frame b), both
//          real, so nothing is untangled.  Decimation in frequency (natural in, bit-reversed out),
//          the shrinkage element by element, decimation in time back (bit-reversed in, natural out):
//          no permutation pass.  The rounding of a frame's transform is relative to the larger of
//          the pair.
//   DIRECT any F: the sum over j with the table at (j k) mod 2 (F - 1), the index kept in integers.
// Both read one table cos(pi j / (F - 1)), j < 2 (F - 1) (k_hva_cos_table).
// fp64, no atomics, every sum in a fixed order: two runs give the same bits.
#include "common.hpp"
#include "prox_passes.hpp"

#include <cmath>

namespace ssspy {

namespace {

constexpr int HVA_THREADS = 512;
constexpr int HVA_SLAB_DOUBLES = 16384;  // the slab of a workgroup: 128 KiB of the CU's 160
constexpr int HVA_MAX_TILE = 32;         // frames of a tile (a power of two)
constexpr int HVA_MAX_BINS = HVA_SLAB_DOUBLES / 2;  // DIRECT: two slabs of F rows, one frame

struct HvaPlan {
  bool ok;
  int route;     // SSSPY_HVA_ROUTE_FFT / _DIRECT
  int rows;      // slab rows: L = 2 (F - 1) (FFT), 2 F (DIRECT: input and output)
  int log2len;   // FFT: log2 L
  int max_tile;  // the largest tile of frames the slab budget allows (a power of two)
};

static int ilog2_floor(int n) {
  int l = 0;
  while ((2 << l) <= n) ++l;
  return l;
}

static HvaPlan hva_plan(int F, int route) {
  HvaPlan p = {false, 0, 0, 0, 0};
  if (F < 2 || F > HVA_MAX_BINS || route < SSSPY_HVA_ROUTE_AUTO || route > SSSPY_HVA_ROUTE_DIRECT)
    return p;
  const int M = F - 1;
  // two frames per transform: the slab holds L rows of at least two frames
  const bool fft_ok = (M & (M - 1)) == 0 && 2 * M * 2 <= HVA_SLAB_DOUBLES;
  if (route == SSSPY_HVA_ROUTE_FFT && !fft_ok) return p;
  p.route = (route == SSSPY_HVA_ROUTE_DIRECT || !fft_ok) ? SSSPY_HVA_ROUTE_DIRECT
                                                         : SSSPY_HVA_ROUTE_FFT;
  p.rows = p.route == SSSPY_HVA_ROUTE_FFT ? 2 * M : 2 * F;
  p.log2len = p.route == SSSPY_HVA_ROUTE_FFT ? ilog2_floor(2 * M) : 0;
  int tile = HVA_SLAB_DOUBLES / p.rows;
  if (tile > HVA_MAX_TILE) tile = HVA_MAX_TILE;
  p.max_tile = 1 << ilog2_floor(tile);
  p.ok = true;
  return p;
}

// dynamic LDS of k_hva_cepstrum: the slab, the partial sums of the mean, the means, the flags
static size_t hva_lds_bytes(int rows, int tile) {
  return ((size_t)rows * tile + HVA_THREADS + HVA_MAX_TILE) * sizeof(double) +
         HVA_MAX_TILE * sizeof(int);
}

// table[j] = cos(pi j / h), j < 2 h: j is folded to [0, h / 2] first, so the argument of cospi is
// at most 1 / 2 and the quarter points are exact
__global__ __launch_bounds__(256) void k_hva_cos_table(double *__restrict__ table, int h) {
  const int j0 = blockIdx.x * 256 + threadIdx.x;
  if (j0 >= 2 * h) return;
  int j = j0 > h ? 2 * h - j0 : j0;  // cos(pi (2 h - j) / h) = cos(pi j / h)
  double sign = 1.0;
  if (2 * j > h) {  // cos(pi (h - j) / h) = -cos(pi j / h)
    j = h - j;
    sign = -1.0;
  }
  const double v = 2 * j == h ? 0.0 : cospi((double)j / (double)h);
  table[j0] = sign * v;
}

// sigma = min(1, nu), mask_iter times sigma <- (1 - cos(pi sigma)) / 2; returns sigma nu
// (ref: ssspy/bss/hva.py:104-109; pi as the double the reference multiplies by)
__device__ __forceinline__ double hva_shrink(double nu, int mask_iter) {
  double sigma = nu < 1.0 ? nu : 1.0;
  for (int it = 0; it < mask_iter; ++it) sigma = (1.0 - cos(M_PI * sigma)) / 2.0;
  return sigma * nu;
}

// The two forms of Z the cepstral pass runs over: an entry of Z from y = (W x) of it and the entry's
// offset in the state, off = b bstride + (n F + f) T + t.
//   PDS:  Z = dual + W2 x
struct HvaPdsZ {
  const c128 *__restrict__ dual;
  long long bstride;
  __device__ __forceinline__ c128 at(c128 y, long long off) const { return cadd(dual[off], y); }
};
//   ADMM: Z = relax W x + (1 - relax) auxiliary2 + dual2, in the order of admm_form_z; mix == false
//   (relaxation 1): auxiliary2 is not read
struct HvaAdmmZ {
  const c128 *__restrict__ aux2, *__restrict__ dual2;
  long long bstride;
  double relax;
  bool mix;
  __device__ __forceinline__ c128 at(c128 y, long long off) const {
    if (mix) {
      const double om = 1.0 - relax;
      const c128 a = aux2[off];
      y = cmake(relax * y.x + om * a.x, relax * y.y + om * a.y);
    }
    return cadd(y, dual2[off]);
  }
};

// ---- the cepstral pass.  grid (N tiles, B), 512 threads, dynamic LDS hva_lds_bytes.  Workgroup
// (n, tile, b) owns frames [tile TT, tile TT + TT) of source n; TT = 1 << log2tile.  Thread
// (k0, tl) = (tid / TT, tid % TT) walks rows k0, k0 + 512 / TT, ... of column tl, so that the lanes
// of a row read and write TT consecutive frames.  Columns past T hold zeros and are not stored.
// ZForm: HvaPdsZ (W2 the filters of the dual step) or HvaAdmmZ (W2 the demixing filters).
template <typename ZForm>
__global__ __launch_bounds__(HVA_THREADS) void k_hva_cepstrum(
    const c128 *__restrict__ X, const c128 *__restrict__ W2, ZForm zform,
    const double *__restrict__ tab, double *__restrict__ varrho, int N, int F,
    int T, int floor_kind, double floor_eps, int mask_iter, int fft, int log2tile, int log2len) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int TT = 1 << log2tile;
  const int rows = fft ? 2 * (F - 1) : 2 * F;
  double *S = reinterpret_cast<double *>(smem);
  double *red = S + (size_t)rows * TT;  // HVA_THREADS partial sums
  double *mean = red + HVA_THREADS;     // HVA_MAX_TILE
  int *bad = reinterpret_cast<int *>(mean + HVA_MAX_TILE);
  const int tid = threadIdx.x, tl = tid & (TT - 1), k0 = tid >> log2tile;
  const int KS = HVA_THREADS >> log2tile;
  const int n = blockIdx.x % N, b = blockIdx.y;
  const int t = (blockIdx.x / N) * TT + tl;
  const bool live = t < T;
  const long long FT = (long long)F * T;
  const c128 *__restrict__ Xb = X + (long long)b * N * FT;
  const long long zoff = (long long)b * zform.bstride + (long long)n * FT;

  // zeta = log floor(|Z|) into rows 0 .. F - 1, the column sums on the way
  double part = 0.0;
  for (int f = k0; f < F; f += KS) {
    double zeta = 0.0;
    if (live) {
      const c128 *__restrict__ Wn = W2 + (((long long)b * F + f) * N + n) * N;
      c128 y = cmake(0.0, 0.0);
      for (int m = 0; m < N; ++m) cfma(y, Wn[m], Xb[((long long)m * F + f) * T + t]);
      const c128 z = zform.at(y, zoff + (long long)f * T + t);
      zeta = log(apply_floor(hypot(z.x, z.y), floor_kind, floor_eps));
    }
    S[f * TT + tl] = zeta;
    part += zeta;
  }
  red[tid] = part;
  __syncthreads();
  for (int s = KS >> 1; s > 0; s >>= 1) {
    if (k0 < s) red[tid] += red[tid + s * TT];
    __syncthreads();
  }
  if (tid < TT) {
    const double m = red[tid] / (double)F;
    mean[tid] = m;
    // log 0 without a floor: the reference's column is NaN throughout (rho holds inf - inf).  The
    // column is transformed as zeros, so that the frame it shares a transform with stays clean.
    bad[tid] = !(fabs(m) <= 1.79769313486231570815e308);
  }
  __syncthreads();
  const double mu = mean[tl];
  const bool isbad = bad[tl] != 0;

  if (fft) {
    const int M = F - 1, L = 2 * M;
    // rho and its even extension: row L - f = row f
    for (int f = k0; f <= M; f += KS) {
      const double v = isbad ? 0.0 : S[f * TT + tl] - mu;
      S[f * TT + tl] = v;
      if (f > 0 && f < M) S[(L - f) * TT + tl] = v;
    }
    __syncthreads();
    c128 *C = reinterpret_cast<c128 *>(S);  // C[j * P + p]: frames (2 p, 2 p + 1) of row j
    const int log2P = log2tile - 1, P = 1 << log2P;
    const int n_butterflies = M << log2P;
    // decimation in frequency: natural order in, bit-reversed order out
    for (int s = log2len - 1; s >= 0; --s) {
      const int half = 1 << s;
      for (int o = tid; o < n_butterflies; o += HVA_THREADS) {
        const int p = o & (P - 1), i = o >> log2P;
        const int pos = i & (half - 1);
        const int j1 = ((i >> s) << (s + 1)) + pos, j2 = j1 + half;
        const int tw = pos << (log2len - 1 - s);  // e^{-2 pi i tw / L}
        const double wr = tab[tw];
        const double wi = L >= 4 ? -tab[(tw + L - (L >> 2)) & (L - 1)] : 0.0;
        const c128 a = C[j1 * P + p], c = C[j2 * P + p];
        C[j1 * P + p] = cadd(a, c);
        C[j2 * P + p] = cmul(csub(a, c), cmake(wr, wi));
      }
      __syncthreads();
    }
    // the shrinkage on k = 0 .. M, written to k and L - k: the input of the second transform is
    // exactly even again
    const double inv = 1.0 / (double)L;
    for (int k = k0; k <= M; k += KS) {
      const int q1 = (int)(__brev((unsigned)k) >> (32 - log2len));
      const int q2 = (int)(__brev((unsigned)((L - k) & (L - 1))) >> (32 - log2len));
      const double v = hva_shrink(S[q1 * TT + tl] * inv, mask_iter);
      S[q1 * TT + tl] = v;
      S[q2 * TT + tl] = v;
    }
    __syncthreads();
    // decimation in time: bit-reversed order in, natural order out
    for (int s = 0; s < log2len; ++s) {
      const int half = 1 << s;
      for (int o = tid; o < n_butterflies; o += HVA_THREADS) {
        const int p = o & (P - 1), i = o >> log2P;
        const int pos = i & (half - 1);
        const int j1 = ((i >> s) << (s + 1)) + pos, j2 = j1 + half;
        const int tw = pos << (log2len - 1 - s);
        const double wr = tab[tw];
        const double wi = L >= 4 ? -tab[(tw + L - (L >> 2)) & (L - 1)] : 0.0;
        const c128 a = C[j1 * P + p], c = cmul(C[j2 * P + p], cmake(wr, wi));
        C[j1 * P + p] = cadd(a, c);
        C[j2 * P + p] = csub(a, c);
      }
      __syncthreads();
    }
  } else {
    double *S0 = S, *S1 = S + (size_t)F * TT;
    const int n2 = 2 * (F - 1);
    for (int f = k0; f < F; f += KS) S0[f * TT + tl] = isbad ? 0.0 : S0[f * TT + tl] - mu;
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
      const double *src = pass == 0 ? S0 : S1;
      double *dst = pass == 0 ? S1 : S0;
      const double c0 = src[tl], cl = src[(F - 1) * TT + tl];
      for (int k = k0; k < F; k += KS) {
        double acc = 0.0;
        int idx = 0;  // (j k) mod n2
        for (int j = 1; j < F - 1; ++j) {
          idx += k;
          if (idx >= n2) idx -= n2;
          acc = fma(src[j * TT + tl], tab[idx], acc);
        }
        const double d = c0 + ((k & 1) ? -cl : cl) + 2.0 * acc;
        dst[k * TT + tl] = pass == 0 ? hva_shrink(d / (double)n2, mask_iter) : d;
      }
      __syncthreads();  // (pass 1 writes S0 after every read of it in pass 0 is done)
    }
  }
  if (live) {
    double *out = varrho + ((long long)b * N + n) * FT + t;
    for (int k = k0; k < F; k += KS)
      out[(long long)k * T] = isbad ? __longlong_as_double(0x7ff8000000000000ll) : S[k * TT + tl] + mu;
  }
}

// ---- the masked dual step.  grid (F, B), 256 threads; thread j walks frames j, j + 256, ... with
// the N rows of Z in registers, as k_pds_dual_step.
template <int G>
__global__ __launch_bounds__(PROX_THREADS) void k_hva_dual_step(
    const c128 *__restrict__ X, const c128 *__restrict__ W2, c128 *dual, long long dual_bstride,
    const double *__restrict__ varrho, int N, int F, int T, double gamma, double relax) {
  __shared__ c128 Ws[G * G];
  const int tid = threadIdx.x;
  const int i = blockIdx.x, b = blockIdx.y;
  const long long FT = (long long)F * T;
  const c128 *__restrict__ Xb = X + ((long long)b * N * F + i) * T;
  c128 *Db = dual + (long long)b * dual_bstride + (long long)i * T;
  const double *__restrict__ Vb = varrho + ((long long)b * N * F + i) * T;  // row n at + n FT
  if (tid < N * N) Ws[tid] = W2[((long long)b * F + i) * (N * N) + tid];
  __syncthreads();
  for (int j = tid; j < T; j += PROX_THREADS) {
    c128 z[G];
    pds_form_z<G>(z, Xb, Db, Ws, N, FT, j);
    double mask[G];
    hva_mask<G>(mask, Vb, N, FT, j, gamma);
#pragma unroll
    for (int n = 0; n < G; ++n) {
      if (n < N) {
        const c128 yt = cmake(z[n].x - mask[n] * z[n].x, z[n].y - mask[n] * z[n].y);
        const c128 d = Db[n * FT + j];
        Db[n * FT + j] = cmake(relax * yt.x + (1.0 - relax) * d.x, relax * yt.y + (1.0 - relax) * d.y);
      }
    }
  }
}

// ---- the masked auxiliary step of MaskingADMMHVA.  Grid and registers as k_hva_dual_step; a thread
// reads the N entries of auxiliary2 / dual2 of its frame (admm_form_z) before it writes them.
template <int G>
__global__ __launch_bounds__(PROX_THREADS) void k_hva_aux_step(
    const c128 *__restrict__ X, const c128 *__restrict__ W, c128 *aux2, c128 *dual2, long long bstride,
    const double *__restrict__ varrho, int N, int F, int T, double gamma, double relax) {
  __shared__ c128 Ws[G * G];
  const int tid = threadIdx.x;
  const int i = blockIdx.x, b = blockIdx.y;
  const long long FT = (long long)F * T;
  const bool mix = relax != 1.0;
  const c128 *__restrict__ Xb = X + ((long long)b * N * F + i) * T;
  const long long so = (long long)b * bstride + (long long)i * T;
  c128 *Ab = aux2 + so, *Db = dual2 + so;
  const double *__restrict__ Vb = varrho + ((long long)b * N * F + i) * T;  // row n at + n FT
  if (tid < N * N) Ws[tid] = W[((long long)b * F + i) * (N * N) + tid];
  __syncthreads();
  for (int j = tid; j < T; j += PROX_THREADS) {
    c128 z[G];
    admm_form_z<G>(z, Xb, Ab, Db, Ws, N, FT, j, relax, mix);
    double mask[G];
    hva_mask<G>(mask, Vb, N, FT, j, gamma);
#pragma unroll
    for (int n = 0; n < G; ++n) {
      if (n < N) {
        const c128 v = cscale(z[n], mask[n]);
        Ab[n * FT + j] = v;
        Db[n * FT + j] = csub(z[n], v);
      }
    }
  }
}

// ---- the checks and the launch of the cepstral pass over either form of Z; `present`: the pointers
// of the form hold.  `word`: what the messages call the form's batch stride.
template <typename ZForm>
static int launch_cepstrum(const char *name, const char *word, bool present, const void *X,
                           const void *W2, const ZForm &zform, const double *table, double *varrho,
                           int B, int N, int F, int T, int floor_kind, double floor_eps, int mask_iter,
                           int route, void *stream) {
  char msg[160];
  if (!(present && table && varrho && B > 0 && F > 0 && T > 0 && mask_iter >= 0)) {
    std::snprintf(msg, sizeof(msg), "%s: bad argument", name);
    return fail(SSSPY_ERR_BADARG, msg);
  }
  if (!(floor_kind >= SSSPY_FLOOR_NONE && floor_kind <= SSSPY_FLOOR_ADD)) {
    std::snprintf(msg, sizeof(msg), "%s: bad flooring", name);
    return fail(SSSPY_ERR_BADARG, msg);
  }
  if (!prox_shape_ok(B, N, F, T)) {
    std::snprintf(msg, sizeof(msg), "%s: 1..16 sources, up to 65535 mixtures", name);
    return fail(SSSPY_ERR_UNSUPPORTED, msg);
  }
  if (zform.bstride < (long long)N * F * T) {
    std::snprintf(msg, sizeof(msg), "%s: bad %s stride", name, word);
    return fail(SSSPY_ERR_BADARG, msg);
  }
  const HvaPlan plan = hva_plan(F, route);
  if (!plan.ok) {
    std::snprintf(msg, sizeof(msg),
                  "%s: 2..8192 bins; the FFT route needs n_bins - 1 a power of two, n_bins <= 4097",
                  name);
    return fail(SSSPY_ERR_UNSUPPORTED, msg);
  }
  const bool fft = plan.route == SSSPY_HVA_ROUTE_FFT;
  // no wider a tile than the frames there are (the FFT pairs frames: two at least)
  int log2tile = ilog2_floor(plan.max_tile);
  while (log2tile > (fft ? 1 : 0) && (1 << (log2tile - 1)) >= T) --log2tile;
  const int tile = 1 << log2tile;
  const long long blocks = ((long long)T + tile - 1) / tile * N;
  if (blocks > 0x7fffffffll) {
    std::snprintf(msg, sizeof(msg), "%s: too many frames", name);
    return fail(SSSPY_ERR_UNSUPPORTED, msg);
  }
  const size_t lds = hva_lds_bytes(plan.rows, tile);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void *)k_hva_cepstrum<ZForm>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(SSSPY_ERR_HIP, hipGetErrorString(e));
  }
  hipLaunchKernelGGL((k_hva_cepstrum<ZForm>), dim3((unsigned)blocks, (unsigned)B), dim3(HVA_THREADS),
                     lds, as_stream(stream), (const c128 *)X, (const c128 *)W2, zform, table, varrho, N,
                     F, T, floor_kind, floor_eps, mask_iter, fft ? 1 : 0, log2tile, plan.log2len);
  return check_launch("k_hva_cepstrum");
}

}  // namespace

}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_hva_route(int F, int route) {
  const HvaPlan p = hva_plan(F, route);
  return p.ok ? p.route : -1;
}

int ssspy_hva_cos_table(double *table, int F, void *stream) {
  SSSPY_REQUIRE(table, "hva_cos_table: bad argument");
  if (F < 2 || F > HVA_MAX_BINS) return fail(SSSPY_ERR_UNSUPPORTED, "hva_cos_table: 2..8192 bins");
  const int h = F - 1;
  hipLaunchKernelGGL(k_hva_cos_table, dim3((unsigned)((2 * h + 255) / 256)), dim3(256), 0,
                     as_stream(stream), table, h);
  return check_launch("k_hva_cos_table");
}

int ssspy_hva_cepstrum(const void *X, const void *W2, const void *dual_q,
                       long long dual_batch_stride, const double *table, double *varrho, int B,
                       int N, int F, int T, int floor_kind, double floor_eps, int mask_iter,
                       int route, void *stream) {
  const HvaPdsZ zform = {(const c128 *)dual_q, dual_batch_stride};
  return launch_cepstrum("hva_cepstrum", "dual", X && W2 && dual_q, X, W2, zform, table, varrho, B, N,
                         F, T, floor_kind, floor_eps, mask_iter, route, stream);
}

int ssspy_hva_admm_cepstrum(const void *X, const void *W, const void *aux2_q, const void *dual2_q,
                            long long batch_stride, const double *table, double *varrho, int B, int N,
                            int F, int T, double relaxation, int floor_kind, double floor_eps,
                            int mask_iter, int route, void *stream) {
  const HvaAdmmZ zform = {(const c128 *)aux2_q, (const c128 *)dual2_q, batch_stride, relaxation,
                          relaxation != 1.0};
  return launch_cepstrum("hva_admm_cepstrum", "batch", X && W && aux2_q && dual2_q && aux2_q != dual2_q,
                         X, W, zform, table, varrho, B, N, F, T, floor_kind, floor_eps, mask_iter,
                         route, stream);
}

int ssspy_hva_dual_step(const void *X, const void *W2, void *dual_q, long long dual_batch_stride,
                        const double *varrho, double attenuation, double relaxation, int B, int N,
                        int F, int T, void *stream) {
  const int rc = prox_check_args("hva_dual_step", X && W2 && dual_q && varrho, B, N, F, T,
                                 {"dual", dual_batch_stride});
  if (rc != SSSPY_OK) return rc;
  SSSPY_PROX_DISPATCH_G(N, hipLaunchKernelGGL((k_hva_dual_step<GG>), dim3((unsigned)F, (unsigned)B),
                                              dim3(PROX_THREADS), 0, as_stream(stream), (const c128 *)X,
                                              (const c128 *)W2, (c128 *)dual_q, dual_batch_stride,
                                              varrho, N, F, T, attenuation, relaxation));
  return check_launch("k_hva_dual_step");
}

int ssspy_hva_aux_step(const void *X, const void *W, void *aux2_q, void *dual2_q,
                       long long batch_stride, const double *varrho, double attenuation,
                       double relaxation, int B, int N, int F, int T, void *stream) {
  const int rc = prox_check_args("hva_aux_step",
                                 X && W && aux2_q && dual2_q && varrho && aux2_q != dual2_q, B, N, F, T,
                                 {"batch", batch_stride});
  if (rc != SSSPY_OK) return rc;
  SSSPY_PROX_DISPATCH_G(N, hipLaunchKernelGGL((k_hva_aux_step<GG>), dim3((unsigned)F, (unsigned)B),
                                              dim3(PROX_THREADS), 0, as_stream(stream), (const c128 *)X,
                                              (const c128 *)W, (c128 *)aux2_q, (c128 *)dual2_q,
                                              batch_stride, varrho, N, F, T, attenuation, relaxation));
  return check_launch("k_hva_aux_step");
}

}  // extern "C"
