// Weighted prediction error (WPE) dereverberation: the bin-resident iteration kernel.
// Nakatani, Yoshioka, Kinoshita, Miyoshi, Juang, "Speech dereverberation based on variance-normalized
// delayed linear prediction", IEEE TASLP 18(7), 2010 (eq. numbers below are the paper's).
//
// Per bin, with x_t in C^M the mixture at frame t, K taps, delay D and L = K M:
//   xs_t in C^L, entry k M + m = x[m, t - D - k] (zero before the first frame)       (eq. 24)
//   y_t = x_t - G^H xs_t,  G (L, M)                                                  (eq. 26)
//   lambda_t = floor((1 / M) sum_m |y_mt|^2)                                         (eq. 45)
//   R = sum_t xs_t xs_t^H / lambda_t,  P = sum_t xs_t x_t^H / lambda_t,  G = R^-1 P  (eq. 46-48)
// The bins never talk to each other (the model of csrc/fdica.hip): a workgroup owns one (mixture,
// bin), keeps G, R and P on chip and runs every iteration inside one launch.
//
// A walk over the frames goes in tiles of WPE_TILE frames.  Power: thread tt forms y of frame
// t0 + tt from the current G and leaves 1 / lambda in LDS (and the loss term of the state the walk
// starts from).  Sums: every thread owns up to NPT fixed entries of the packed upper triangle of R and
// up to two of P and walks the frames of the tile in order: no atomics, the same bits on every run.
// Then the Cholesky factorisation R = U^H U in LDS (right-looking: row j scaled, the trailing block
// updated by all 256 threads), M forward and back substitutions by rows, and G is replaced.
//
// LDS (dynamic; 160 KiB per CU decide the bounds):
//   fixed   R packed L (L + 1) / 2, the right-hand sides L M, G L M (c128), 1 / diag (L), 1 / lambda
//           (WPE_TILE) and 16 doubles: 33280 + 8192 + 8192 + 512 + 2048 + 128 = 52352 bytes at L = 64
//   RESIDENT  the bin's slab, M rows of K - 1 zeros and the T frames: at most WPE_SLAB_LDS_BYTES = 48 KiB
//           (the rule of fdica.hip; two workgroups fit a CU up to L = 40), 101504 bytes with the above
//   otherwise per tile the history rows (WPE_TILE + K - 1 frames, zeros before frame 0) and the
//           current rows (WPE_TILE frames), re-read from memory on every walk: at most
//           8 * (319 + 256) * 16 = 73600, 125952 bytes with the above
#include "common.hpp"

namespace ssspy {

constexpr int WPE_THREADS = 256;
constexpr int WPE_TILE = 256;  // frames per tile: one per thread in the power pass
constexpr int WPE_MAX_CHANNELS = 8;
constexpr int WPE_MAX_ORDER = 64;  // taps * n_channels
constexpr int WPE_SLAB_LDS_BYTES = 48 * 1024;
constexpr int WPE_MAX_NPT = (WPE_MAX_ORDER * (WPE_MAX_ORDER + 1) / 2 + WPE_THREADS - 1) / WPE_THREADS;

// index of (p, q), p <= q, in the row-major upper triangle of an L x L matrix
__device__ __forceinline__ int wpe_tri(int L, int p, int q) {
  return p * L - p * (p - 1) / 2 + (q - p);
}

struct WpeLds {
  size_t fixed_bytes, slab_bytes;
};
static WpeLds wpe_lds(int M, int K, int T, bool resident) {
  const size_t L = (size_t)K * M;
  WpeLds s;
  s.fixed_bytes = (L * (L + 1) / 2 + 2 * L * M) * sizeof(c128) +
                  (((L + 1) & ~(size_t)1) + WPE_TILE + 16) * sizeof(double);
  s.slab_bytes = resident ? (size_t)M * (T + K - 1) * sizeof(c128)
                          : (size_t)M * (2 * WPE_TILE + K - 1) * sizeof(c128);
  return s;
}
static bool wpe_resident(int M, int K, int T) {
  return (long long)M * ((long long)T + K - 1) * (long long)sizeof(c128) <= WPE_SLAB_LDS_BYTES;
}

// y of one frame: thread-private, M outputs.  H: history rows (row m at H + m * HS, tap k one frame
// back per step), C: current rows.
template <int M>
__device__ __forceinline__ void wpe_frame(const c128 *H, int HS, const c128 *C, int CS,
                                          const c128 *Gs, int K, int tt, bool history,
                                          c128 (&y)[WPE_MAX_CHANNELS]) {
#pragma unroll
  for (int c = 0; c < M; ++c) y[c] = C[c * CS + tt];
  if (history) {
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const c128 x = H[m * HS + tt - k];
        const c128 *g = Gs + (k * M + m) * M;
#pragma unroll
        for (int c = 0; c < M; ++c) cfmsc(y[c], g[c], x);  // y_c -= conj(G[l, c]) xs[l]
      }
    }
  }
}

// grid: (F, B), 256 threads.  n_steps iterations on G (B, F, L, M) in place, then a last walk that
// writes Y (B, M, F, T) (when not NULL).
//   loss (may be NULL): walk s leaves (1 / T) sum_t [M log lambda_t + sum_m |y_mt|^2 / lambda_t] of the
//   state it STARTS from at loss[f * slot_stride + s * B + b]; the last walk leaves entry n_steps.
//   lam_out (B, F, T), R_out (B, F, L, L), P_out (B, F, L, M), U_out (B, F, L, L): what the LAST
//   iteration formed (tests); any may be NULL.
//   A pivot that is not positive and finite bumps info[0] once and ends the iterations of the bin: G
//   stays what the iteration started from and Y is formed from it.
template <int NPT, bool RESIDENT>
__global__ __launch_bounds__(WPE_THREADS) void k_wpe(
    const c128 *__restrict__ X, c128 *G, c128 *Y, int B, int M, int F, int T, int K, int D,
    int floor_kind, double eps, int n_steps, double *loss, long long slot_stride, int *info,
    double *lam_out, c128 *R_out, c128 *P_out, c128 *U_out) {
  extern __shared__ c128 lds[];
  const int tid = threadIdx.x;
  const int f = blockIdx.x, b = blockIdx.y;
  const int L = K * M, NE = L * (L + 1) / 2, LM = L * M;
  c128 *Rs = lds;
  c128 *Ps = Rs + NE;
  c128 *Gs = Ps + LM;
  double *invd = reinterpret_cast<double *>(Gs + LM);
  double *rlam = invd + ((L + 1) & ~1);
  double *red = rlam + WPE_TILE;  // 16 doubles: block_sum's scratch
  c128 *slab = reinterpret_cast<c128 *>(red + 16);
  const int pad = K - 1;
  // history (m, frame t0 + tt, tap k) at Hb[m * HS + tt - k], current at Cb[m * CS + tt]
  const int HS = RESIDENT ? T + pad : WPE_TILE + pad;
  const int CS = RESIDENT ? HS : WPE_TILE;
  c128 *Hs = slab, *Cs = RESIDENT ? slab + pad : slab + (size_t)M * HS;

  const long long row_stride = (long long)F * T;
  const c128 *__restrict__ Xb = X + ((long long)b * M * F + f) * T;  // row m at Xb + m * row_stride
  c128 *Gb = G + ((long long)b * F + f) * LM;
  const long long bf = (long long)b * F + f;

  for (int e = tid; e < LM; e += WPE_THREADS) Gs[e] = Gb[e];
  if (RESIDENT) {
    for (int m = 0; m < M; ++m) {
      for (int j = tid; j < pad; j += WPE_THREADS) slab[m * HS + j] = cmake(0.0, 0.0);
      for (int j = tid; j < T; j += WPE_THREADS) slab[m * HS + pad + j] = Xb[m * row_stride + j];
    }
  }
  // the entries this thread owns: offsets of their two operands within a history / current row set
  int op[NPT], oq[NPT];
#pragma unroll
  for (int i = 0; i < NPT; ++i) {
    int e = tid + i * WPE_THREADS;
    if (e >= NE) e = 0;  // (idle: shadows entry 0, never stores)
    int p = 0;
    while (e >= L - p) {
      e -= L - p;
      ++p;
    }
    const int q = p + e;
    op[i] = (p % M) * HS - p / M;
    oq[i] = (q % M) * HS - q / M;
  }
  int pl[2], pc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int e = tid + i * WPE_THREADS;
    if (e >= LM) e = 0;
    const int l = e / M;
    pl[i] = (l % M) * HS - l / M;
    pc[i] = (e % M) * CS;
  }
  __syncthreads();

  const double inv_t = 1.0 / (double)T, inv_m = 1.0 / (double)M;
  bool failed = false;
#pragma unroll 1
  for (int s = 0; s <= n_steps; ++s) {
    const bool last = s == n_steps || failed;
    const bool keep = !last && s == n_steps - 1;  // the iteration whose statistics are handed out
    c128 acc[NPT], accp[2];
#pragma unroll
    for (int i = 0; i < NPT; ++i) acc[i] = cmake(0.0, 0.0);
    accp[0] = accp[1] = cmake(0.0, 0.0);
    double term = 0.0;
#pragma unroll 1
    for (int t0 = 0; t0 < T; t0 += WPE_TILE) {
      const int nt = min(WPE_TILE, T - t0);
      const c128 *Hb, *Cb;
      if (RESIDENT) {
        Hb = slab + pad + (t0 - D);  // (read only at frames t >= D: never below the zeros)
        Cb = Cs + t0;
      } else {
        __syncthreads();  // the previous tile has been read
        const int first = t0 - D - pad;  // frame of history column 0
        for (int m = 0; m < M; ++m) {
          for (int j = tid; j < nt + pad; j += WPE_THREADS) {
            const int fr = first + j;
            Hs[m * HS + j] = fr >= 0 && fr < T ? Xb[m * row_stride + fr] : cmake(0.0, 0.0);
          }
          for (int j = tid; j < nt; j += WPE_THREADS) Cs[m * CS + j] = Xb[m * row_stride + t0 + j];
        }
        Hb = Hs + pad;
        Cb = Cs;
        __syncthreads();
      }
      // ---- power: thread tt, frame t0 + tt
      if (tid < nt) {
        const int tt = tid, t = t0 + tt;
        c128 y[WPE_MAX_CHANNELS];
        switch (M) {
          case 1: wpe_frame<1>(Hb, HS, Cb, CS, Gs, K, tt, t >= D, y); break;
          case 2: wpe_frame<2>(Hb, HS, Cb, CS, Gs, K, tt, t >= D, y); break;
          case 3: wpe_frame<3>(Hb, HS, Cb, CS, Gs, K, tt, t >= D, y); break;
          case 4: wpe_frame<4>(Hb, HS, Cb, CS, Gs, K, tt, t >= D, y); break;
          case 5: wpe_frame<5>(Hb, HS, Cb, CS, Gs, K, tt, t >= D, y); break;
          case 6: wpe_frame<6>(Hb, HS, Cb, CS, Gs, K, tt, t >= D, y); break;
          case 7: wpe_frame<7>(Hb, HS, Cb, CS, Gs, K, tt, t >= D, y); break;
          default: wpe_frame<8>(Hb, HS, Cb, CS, Gs, K, tt, t >= D, y); break;
        }
        double pw = 0.0;
#pragma unroll
        for (int c = 0; c < WPE_MAX_CHANNELS; ++c)
          if (c < M) pw += cabs2(y[c]);
        const double lam = apply_floor(pw * inv_m, floor_kind, eps);
        term += (double)M * log(lam) + pw / lam;
        rlam[tt] = 1.0 / lam;
        if (keep && lam_out) lam_out[bf * T + t] = lam;
        if (last && Y) {
#pragma unroll
          for (int c = 0; c < WPE_MAX_CHANNELS; ++c)
            if (c < M) Y[((long long)b * M + c) * row_stride + (long long)f * T + t] = y[c];
        }
      }
      if (!last) {
        __syncthreads();  // 1 / lambda of the tile
        // ---- sums: frames in order inside every thread; frames before D have no history
#pragma unroll 1
        for (int tt = max(0, D - t0); tt < nt; ++tt) {
          const double w = rlam[tt];
#pragma unroll
          for (int i = 0; i < NPT; ++i)
            cfmac(acc[i], cscale(Hb[op[i] + tt], w), Hb[oq[i] + tt]);
#pragma unroll
          for (int i = 0; i < 2; ++i)
            cfmac(accp[i], cscale(Hb[pl[i] + tt], w), Cb[pc[i] + tt]);
        }
        __syncthreads();  // rlam is rewritten by the next tile
      }
    }
    if (loss) {  // (uniform: every thread reaches the barriers of block_sum)
      const double total = block_sum(term, red);
      if (tid == 0) loss[(long long)f * slot_stride + (long long)s * B + b] = total * inv_t;
    }
    if (last) break;

    // ---- R (packed upper triangle) and P to LDS
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const int e = tid + i * WPE_THREADS;
      if (e < NE) Rs[e] = acc[i];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + i * WPE_THREADS;
      if (e < LM) Ps[e] = accp[i];
    }
    __syncthreads();
    if (keep && R_out) {
      for (int e = tid; e < L * L; e += WPE_THREADS) {
        const int p = e / L, q = e % L;
        c128 v = p <= q ? Rs[wpe_tri(L, p, q)] : cconj(Rs[wpe_tri(L, q, p)]);
        if (p == q) v.y = 0.0;
        R_out[bf * L * L + e] = v;
      }
    }
    if (keep && P_out)
      for (int e = tid; e < LM; e += WPE_THREADS) P_out[bf * LM + e] = Ps[e];
    if (keep && (R_out || P_out)) __syncthreads();

    // ---- Cholesky R = U^H U in place, right-looking: row j <- row j / sqrt(pivot), then
    // A[k][i] -= conj(U[j][k]) U[j][i] for j < k <= i
    const int ty = tid >> 4, tx = tid & 15;
#pragma unroll 1
    for (int j = 0; j < L; ++j) {
      const int rj = wpe_tri(L, j, j);
      const double d = Rs[rj].x;
      if (!(d > 0.0) || !(d <= 1.79769313486231570815e308)) {  // (uniform)
        failed = true;
        break;
      }
      const double root = sqrt(d), ir = 1.0 / root;
      __syncthreads();  // everybody has read the pivot
      if (tid == 0) {
        Rs[rj] = cmake(root, 0.0);
        invd[j] = ir;
      }
      for (int i = j + 1 + tid; i < L; i += WPE_THREADS) Rs[rj + i - j] = cscale(Rs[rj + i - j], ir);
      __syncthreads();
      for (int k = j + 1 + ty; k < L; k += 16) {
        const c128 ujk = Rs[rj + k - j];
        const int rk = wpe_tri(L, k, k);
        for (int i = k + tx; i < L; i += 16) cfmsc(Rs[rk + i - k], ujk, Rs[rj + i - j]);
      }
      __syncthreads();
    }
    if (failed) {
      __syncthreads();
      if (tid == 0 && info) atomicAdd(info, 1);
      continue;  // the last walk, from the G this iteration started from
    }
    if (keep && U_out) {
      for (int e = tid; e < L * L; e += WPE_THREADS) {
        const int p = e / L, q = e % L;
        U_out[bf * L * L + e] = p <= q ? Rs[wpe_tri(L, p, q)] : cmake(0.0, 0.0);
      }
    }

    // ---- U^H z = P, then U g = z: thread e owns (row e / M, right-hand side e % M); in step j the
    // rows behind j take the finished row j, one barrier per step
    int row[2], col[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + i * WPE_THREADS;
      row[i] = e < LM ? e / M : -1;
      col[i] = e < LM ? e % M : 0;
    }
#pragma unroll 1
    for (int j = 0; j < L; ++j) {
      const int rj = wpe_tri(L, j, j);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (row[i] > j)
          cfmsc(Ps[row[i] * M + col[i]], Rs[rj + row[i] - j], cscale(Ps[j * M + col[i]], invd[j]));
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (row[i] >= 0) Ps[row[i] * M + col[i]] = cscale(Ps[row[i] * M + col[i]], invd[row[i]]);
    __syncthreads();
#pragma unroll 1
    for (int j = L - 1; j >= 0; --j) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (row[i] >= 0 && row[i] < j)
          cfms(Ps[row[i] * M + col[i]], Rs[wpe_tri(L, row[i], j)], cscale(Ps[j * M + col[i]], invd[j]));
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (row[i] >= 0) Gs[row[i] * M + col[i]] = cscale(Ps[row[i] * M + col[i]], invd[row[i]]);
    __syncthreads();
  }
  if (n_steps > 0)
    for (int e = tid; e < LM; e += WPE_THREADS) Gb[e] = Gs[e];
}

template <int NPT, bool RESIDENT>
static int launch_wpe_as(const c128 *X, c128 *G, c128 *Y, int B, int M, int F, int T, int K, int D,
                         int floor_kind, double eps, int n_steps, double *loss,
                         long long slot_stride, int *info, double *lam, c128 *R, c128 *P, c128 *U,
                         hipStream_t st) {
  const WpeLds need = wpe_lds(M, K, T, RESIDENT);
  const size_t smem = need.fixed_bytes + need.slab_bytes;
  if (smem > 64 * 1024) {
    // (granted once per instantiation and device, not on every launch)
    static size_t granted[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (smem > granted[dev]) {
      hipError_t e = hipFuncSetAttribute((const void *)k_wpe<NPT, RESIDENT>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      if (e != hipSuccess) return fail(SSSPY_ERR_HIP, hipGetErrorString(e));
      granted[dev] = smem;
    }
  }
  hipLaunchKernelGGL((k_wpe<NPT, RESIDENT>), dim3((unsigned)F, (unsigned)B), dim3(WPE_THREADS), smem,
                     st, X, G, Y, B, M, F, T, K, D, floor_kind, eps, n_steps, loss, slot_stride, info,
                     lam, R, P, U);
  return check_launch("k_wpe");
}

static int wpe_check(int B, int M, int F, int T, int K, int D, int floor_kind, const char **why) {
  *why = nullptr;
  if (B <= 0 || F <= 0 || T <= 0 || K < 1 || M < 1 || D < 1 || floor_kind < SSSPY_FLOOR_NONE ||
      floor_kind > SSSPY_FLOOR_ADD) {
    *why = "wpe: bad argument (sizes and taps positive, delay >= 1, a floor the kernels apply)";
    return SSSPY_ERR_BADARG;
  }
  if (M > WPE_MAX_CHANNELS || (long long)K * M > WPE_MAX_ORDER || B > 65535 ||
      T > (1 << 30)) {
    *why = "wpe: 1..8 channels, taps * n_channels <= 64, up to 65535 mixtures";
    return SSSPY_ERR_UNSUPPORTED;
  }
  return SSSPY_OK;
}

static int launch_wpe(const void *X, void *G, void *Y, int B, int M, int F, int T, int K, int D,
                      int floor_kind, double eps, int n_steps, double *loss, long long slot_stride,
                      int *info, double *lam, void *R, void *P, void *U, int route, void *stream) {
  const char *why;
  const int rc = wpe_check(B, M, F, T, K, D, floor_kind, &why);
  if (rc != SSSPY_OK) return fail(rc, why);
  SSSPY_REQUIRE(X && G && X != Y && n_steps >= 0 && (n_steps > 0 || Y || loss), "wpe: bad argument");
  SSSPY_REQUIRE(!loss || slot_stride >= ((long long)n_steps + 1) * B,
                "wpe: slot_stride >= (n_steps + 1) B");
  SSSPY_REQUIRE(route >= SSSPY_WPE_ROUTE_AUTO && route <= SSSPY_WPE_ROUTE_STREAMING,
                "wpe: route is one of SSSPY_WPE_ROUTE_*");
  const bool resident = route != SSSPY_WPE_ROUTE_STREAMING && wpe_resident(M, K, T);
  const int L = K * M;
  const int npt = (L * (L + 1) / 2 + WPE_THREADS - 1) / WPE_THREADS;
  D = D < T ? D : T;  // (no frame has a history from delay = n_frames on)
#define WPE_CASE(NPT_)                                                                              \
  case NPT_:                                                                                        \
    return resident ? launch_wpe_as<NPT_, true>((const c128 *)X, (c128 *)G, (c128 *)Y, B, M, F, T, \
                                                 K, D, floor_kind, eps, n_steps, loss, slot_stride, \
                                                 info, lam, (c128 *)R, (c128 *)P, (c128 *)U,        \
                                                 as_stream(stream))                                 \
                    : launch_wpe_as<NPT_, false>((const c128 *)X, (c128 *)G, (c128 *)Y, B, M, F, T, \
                                                  K, D, floor_kind, eps, n_steps, loss,             \
                                                  slot_stride, info, lam, (c128 *)R, (c128 *)P,     \
                                                  (c128 *)U, as_stream(stream))
  static_assert(WPE_MAX_NPT == 9, "the cases below cover 1..WPE_MAX_NPT entries per thread");
  switch (npt) {
    WPE_CASE(1);
    WPE_CASE(2);
    WPE_CASE(3);
    WPE_CASE(4);
    WPE_CASE(5);
    WPE_CASE(6);
    WPE_CASE(7);
    WPE_CASE(8);
    WPE_CASE(9);
  }
#undef WPE_CASE
  return fail(SSSPY_ERR_INTERNAL, "wpe: no kernel for this order");
}

}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_wpe_route(int B, int M, int F, int T, int taps, int *lds_bytes) {
  const char *why;
  if (wpe_check(B, M, F, T, taps, 1, SSSPY_FLOOR_NONE, &why) != SSSPY_OK) return -1;
  const bool resident = wpe_resident(M, taps, T);
  if (lds_bytes) {
    const WpeLds need = wpe_lds(M, taps, T, resident);
    *lds_bytes = (int)(need.fixed_bytes + need.slab_bytes);
  }
  return resident ? SSSPY_WPE_ROUTE_RESIDENT : SSSPY_WPE_ROUTE_STREAMING;
}

int ssspy_wpe_steps(const void *X, void *G, void *Y, int B, int M, int F, int T, int taps, int delay,
                    int floor_kind, double floor_eps, int n_steps, double *loss_data,
                    long long slot_stride, int *info, int route, void *stream) {
  SSSPY_REQUIRE(n_steps >= 1, "wpe_steps: n_steps >= 1");
  return launch_wpe(X, G, Y, B, M, F, T, taps, delay, floor_kind, floor_eps, n_steps, loss_data,
                    slot_stride, info, nullptr, nullptr, nullptr, nullptr, route, stream);
}

int ssspy_wpe_step(const void *X, void *G, void *Y, int B, int M, int F, int T, int taps, int delay,
                   int floor_kind, double floor_eps, int *info, double *lambda, void *R, void *P,
                   void *U, int route, void *stream) {
  return launch_wpe(X, G, Y, B, M, F, T, taps, delay, floor_kind, floor_eps, 1, nullptr, 0, info,
                    lambda, R, P, U, route, stream);
}

int ssspy_wpe_apply(const void *X, const void *G, void *Y, int B, int M, int F, int T, int taps,
                    int delay, int floor_kind, double floor_eps, double *loss_data,
                    long long slot_stride, int route, void *stream) {
  // (n_steps = 0: the last walk alone; G is read and stored back unchanged)
  return launch_wpe(X, const_cast<void *>(G), Y, B, M, F, T, taps, delay, floor_kind, floor_eps, 0,
                    loss_data, slot_stride, nullptr, nullptr, nullptr, nullptr, nullptr, route,
                    stream);
}

}  // extern "C"
