// The weighted power minimisation distortionless response (WPD) convolutional beamformer: the
// bin-resident iteration kernel.
// Nakatani, Kinoshita, "A unified convolutional beamformer for simultaneous denoising and
// dereverberation", IEEE SPL 26(6), 2019; Boeddeker, Nakatani, Kinoshita, Haeb-Umbach, "Jointly optimal
// dereverberation and beamforming", ICASSP 2020 (the steering-vector-free form).
//
// Per (mixture, bin, source), with x_t in C^M the mixture at frame t, K >= 0 taps, delay D >= 1 and
// Lb = (K + 1) M:
//   xb_t in C^Lb: block 0 is x_t, block j = 1..K is x_{t - D - (j - 1)} (zero before the first frame)
//   y_t = wb^H xb_t,  lambda_t = floor(|y_t|^2)
//   R = (1 / T) sum_t xb_t xb_t^H / lambda_t + loading (tr R / Lb) I
//   mask form      Phi_s = sum_t m_t x_t x_t^H / max(sum_t m_t, 1e-10) (once per launch),
//                  A = (R^-1)[:, :M] Phi_s,  wb = A[:, ref] / Re tr(A[:M, :])
//   steering form  vb = [v; 0],  a = R^-1 vb,  wb = a conj(v_ref) / (vb^H a)
//   a denominator that is zero or not finite gives wb = 0
// The filter is kept and stored conjugated, W[l] = conj(wb[l]), so that y_t = sum_l W[l] xb_t[l].
// The sources of a bin share nothing but X: a workgroup owns one (mixture, bin, source), keeps W and R
// on chip and runs every iteration inside one launch.  The layout is that of csrc/wpe.hip.
//
// A walk over the frames goes in tiles of WPD_TILE frames.  Power: thread tt forms y of frame t0 + tt
// from the current W and leaves 1 / lambda in LDS (and the loss term of the state the walk starts
// from; in the first walk of the mask form also the mask of the frame).  Sums: every thread owns up to
// NPT fixed entries of the packed upper triangle of R and walks the frames of the tile in order; in
// the first walk the owners of the M (M + 1) / 2 entries of Phi_s walk them as well.  No atomics, the
// same bits on every run and on both routes.  Then the Cholesky factorisation R = U^H U in LDS
// (right-looking), the forward and back substitutions by rows for the M (mask form) or 1 (steering
// form) right-hand sides, and W is replaced.
//
// LDS (dynamic; 160 KiB per CU decide the bounds):
//   fixed   R packed Lb (Lb + 1) / 2, the right-hand sides Lb M, W Lb, Phi_s M M, v M (c128), 1 / diag
//           (Lb), 1 / lambda and the mask of a tile (2 WPD_TILE) and 16 doubles:
//           33280 + 8192 + 1024 + 1024 + 128 + 512 + 4096 + 128 = 48384 bytes at M = 8, Lb = 64
//   RESIDENT  the bin's slab, M rows of max(K - 1, 0) zeros and the T frames: at most
//           WPD_SLAB_LDS_BYTES = 48 KiB (the rule of wpe.hip), 97536 bytes with the above
//   otherwise per tile the history rows (WPD_TILE + max(K - 1, 0) frames, zeros before frame 0) and
//           the current rows (WPD_TILE frames), re-read from memory on every walk: at most
//           8 * (262 + 256) * 16 = 66304, 114688 bytes with the above
#include "common.hpp"

namespace ssspy {

constexpr int WPD_THREADS = 256;
constexpr int WPD_TILE = 256;  // frames per tile: one per thread in the power pass
constexpr int WPD_MAX_CHANNELS = 8;
constexpr int WPD_MAX_ORDER = 64;  // (taps + 1) * n_channels
constexpr int WPD_MAX_SOURCES = 16;
constexpr int WPD_SLAB_LDS_BYTES = 48 * 1024;
constexpr int WPD_MAX_NPT = (WPD_MAX_ORDER * (WPD_MAX_ORDER + 1) / 2 + WPD_THREADS - 1) / WPD_THREADS;
constexpr double WPD_EPS = 1e-10;  // floor of the sum of a mask (the beamformers' eps)

// index of (p, q), p <= q, in the row-major upper triangle of an L x L matrix
__device__ __forceinline__ int wpd_tri(int L, int p, int q) {
  return p * L - p * (p - 1) / 2 + (q - p);
}

__device__ __forceinline__ bool wpd_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

struct WpdLds {
  size_t fixed_bytes, slab_bytes;
};
static int wpd_pad(int K) { return K > 1 ? K - 1 : 0; }
static WpdLds wpd_lds(int M, int K, int T, bool resident) {
  const size_t Lb = (size_t)(K + 1) * M, pad = (size_t)wpd_pad(K);
  WpdLds s;
  s.fixed_bytes = (Lb * (Lb + 1) / 2 + Lb * M + Lb + (size_t)M * M + M) * sizeof(c128) +
                  (((Lb + 1) & ~(size_t)1) + 2 * WPD_TILE + 16) * sizeof(double);
  s.slab_bytes = resident ? (size_t)M * (T + pad) * sizeof(c128)
                          : (size_t)M * (2 * WPD_TILE + pad) * sizeof(c128);
  return s;
}
static bool wpd_resident(int M, int K, int T) {
  return (long long)M * ((long long)T + wpd_pad(K)) * (long long)sizeof(c128) <= WPD_SLAB_LDS_BYTES;
}

// grid: (F * N, B), 256 threads; block x = f * N + n.  n_steps iterations on W (B, F, N, Lb) in place,
// then a last walk that writes Y (B, N, F, T) (when not NULL).
//   mask (B, N, F, T) or V (B, F, N, M) chooses the form (V wins); both may be NULL with n_steps = 0.
//   Phi_out (B, F, N, M, M) (may be NULL): Phi_s of the mask form as a full Hermitian matrix.
//   loss (may be NULL): walk s leaves (1 / T) sum_t [log lambda_t + |y_t|^2 / lambda_t] of the state it
//   STARTS from at loss[(f * N + n) * slot_stride + s * B + b]; the last walk leaves entry n_steps
//   (after a failed pivot in iteration s: every entry from s + 1 on, all of the kept state).
//   lam_out (B, F, N, T), R_out, U_out (B, F, N, Lb, Lb): what the LAST iteration formed (tests); any
//   may be NULL.
//   A pivot that is not positive and finite bumps info[0] once and ends the iterations of the triple:
//   W stays what the iteration started from and Y is formed from it.
template <int NPT, bool RESIDENT>
__global__ __launch_bounds__(WPD_THREADS) void k_wpd(
    const c128 *__restrict__ X, const double *__restrict__ mask, const c128 *__restrict__ V, c128 *W,
    c128 *Phi_out, c128 *Y, int B, int M, int N, int F, int T, int K, int D, int ref, double loading,
    int floor_kind, double eps, int n_steps, double *loss, long long slot_stride, int *info,
    double *lam_out, c128 *R_out, c128 *U_out) {
  extern __shared__ c128 lds[];
  const int tid = threadIdx.x;
  const int f = blockIdx.x / N, n = blockIdx.x % N, b = blockIdx.y;
  const int Lb = (K + 1) * M, NE = Lb * (Lb + 1) / 2;
  const bool steer = V != nullptr;
  const int NR = steer ? 1 : M;  // right-hand sides
  c128 *Rs = lds;
  c128 *Zs = Rs + NE;       // (Lb, NR): the right-hand sides, then the solutions
  c128 *Ws = Zs + Lb * M;   // conj(wb)
  c128 *Phis = Ws + Lb;     // (M, M) full
  c128 *Vs = Phis + M * M;  // v
  double *invd = reinterpret_cast<double *>(Vs + M);
  double *rlam = invd + ((Lb + 1) & ~1);
  double *msk = rlam + WPD_TILE;
  double *red = msk + WPD_TILE;  // 16 doubles: block_sum's scratch, the terms of the denominator
  c128 *slab = reinterpret_cast<c128 *>(red + 16);
  const int pad = K > 1 ? K - 1 : 0;
  // history (m, frame t0 + tt, block j >= 1) at Hb[m * HS + tt - (j - 1)], current at Cb[m * CS + tt]
  const int HS = RESIDENT ? T + pad : WPD_TILE + pad;
  const int CS = RESIDENT ? HS : WPD_TILE;
  c128 *Hs = slab, *Cs = RESIDENT ? slab + pad : slab + (size_t)M * HS;
  // Cb - Hb, the same in every tile: the operands of the sums are all addressed from Hb
  const int cur = RESIDENT ? D : M * HS - pad;

  const long long row_stride = (long long)F * T;
  const c128 *__restrict__ Xb = X + ((long long)b * M * F + f) * T;  // row m at Xb + m * row_stride
  const long long bfn = ((long long)b * F + f) * N + n;
  c128 *Wb = W + bfn * Lb;
  const double *__restrict__ mrow = mask ? mask + (((long long)b * N + n) * F + f) * T : nullptr;

  for (int e = tid; e < Lb; e += WPD_THREADS) Ws[e] = Wb[e];
  if (steer)
    for (int e = tid; e < M; e += WPD_THREADS) Vs[e] = V[bfn * M + e];
  if (RESIDENT) {
    for (int m = 0; m < M; ++m) {
      for (int j = tid; j < pad; j += WPD_THREADS) slab[m * HS + j] = cmake(0.0, 0.0);
      for (int j = tid; j < T; j += WPD_THREADS) slab[m * HS + pad + j] = Xb[m * row_stride + j];
    }
  }
  // the entries this thread owns: offsets of their two operands from Hb, and whether both lie in
  // block 0 (the only entries the frames before D add to)
  int op[NPT], oq[NPT];
  unsigned both_current = 0;
#pragma unroll
  for (int i = 0; i < NPT; ++i) {
    int e = tid + i * WPD_THREADS;
    if (e >= NE) e = 0;  // (idle: shadows entry 0, never stores)
    int p = 0;
    while (e >= Lb - p) {
      e -= Lb - p;
      ++p;
    }
    const int q = p + e;
    op[i] = p < M ? cur + p * CS : (p % M) * HS - (p / M - 1);
    oq[i] = q < M ? cur + q * CS : (q % M) * HS - (q / M - 1);
    if (q < M) both_current |= 1u << i;
  }
  // the entry of Phi_s this thread owns (mask form): (pi, pj), pi <= pj
  const int nphi = steer || !mask ? 0 : M * (M + 1) / 2;
  int pi = 0, pj = 0;
  if (tid < nphi) {
    int e = tid;
    while (e >= M - pi) {
      e -= M - pi;
      ++pi;
    }
    pj = pi + e;
  }
  __syncthreads();

  const double inv_t = 1.0 / (double)T;
  bool failed = false;
#pragma unroll 1
  for (int s = 0; s <= n_steps; ++s) {
    const bool last = s == n_steps || failed;
    const bool keep = !last && s == n_steps - 1;  // the iteration whose statistics are handed out
    const bool first = !last && s == 0 && nphi > 0;  // the walk that sums Phi_s as well
    c128 acc[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) acc[i] = cmake(0.0, 0.0);
    c128 accphi = cmake(0.0, 0.0);
    double weight = 0.0, term = 0.0;
#pragma unroll 1
    for (int t0 = 0; t0 < T; t0 += WPD_TILE) {
      const int nt = min(WPD_TILE, T - t0);
      const c128 *Hb, *Cb;
      if (RESIDENT) {
        Hb = slab + pad + (t0 - D);  // (read only at frames t >= D: never below the zeros)
        Cb = Cs + t0;
      } else {
        __syncthreads();  // the previous tile has been read
        const int first_frame = t0 - D - pad;  // frame of history column 0
        for (int m = 0; m < M; ++m) {
          if (K > 0)
            for (int j = tid; j < nt + pad; j += WPD_THREADS) {
              const int fr = first_frame + j;
              Hs[m * HS + j] = fr >= 0 && fr < T ? Xb[m * row_stride + fr] : cmake(0.0, 0.0);
            }
          for (int j = tid; j < nt; j += WPD_THREADS) Cs[m * CS + j] = Xb[m * row_stride + t0 + j];
        }
        Hb = Hs + pad;
        Cb = Cs;
        __syncthreads();
      }
      // ---- power: thread tt, frame t0 + tt
      if (tid < nt) {
        const int tt = tid, t = t0 + tt;
        c128 y = cmake(0.0, 0.0);
        for (int m = 0; m < M; ++m) cfma(y, Ws[m], Cb[m * CS + tt]);
        if (t >= D) {
#pragma unroll 1
          for (int j = 1; j <= K; ++j)
            for (int m = 0; m < M; ++m) cfma(y, Ws[j * M + m], Hb[m * HS + tt - (j - 1)]);
        }
        const double pw = cabs2(y);
        const double lam = apply_floor(pw, floor_kind, eps);
        term += log(lam) + pw / lam;
        rlam[tt] = 1.0 / lam;
        if (first) msk[tt] = mrow[t];
        if (keep && lam_out) lam_out[bfn * T + t] = lam;
        if (last && Y) Y[((long long)b * N + n) * row_stride + (long long)f * T + t] = y;
      }
      if (!last) {
        __syncthreads();  // 1 / lambda (and the mask) of the tile
        // ---- sums: frames in order inside every thread; the frames before D have no history
        const int head = min(nt, max(0, D - t0));
#pragma unroll 1
        for (int tt = 0; tt < head; ++tt) {
          const double w = rlam[tt];
#pragma unroll
          for (int i = 0; i < NPT; ++i)
            if ((both_current >> i) & 1u) cfmac(acc[i], cscale(Hb[op[i] + tt], w), Hb[oq[i] + tt]);
        }
#pragma unroll 1
        for (int tt = head; tt < nt; ++tt) {
          const double w = rlam[tt];
#pragma unroll
          for (int i = 0; i < NPT; ++i) cfmac(acc[i], cscale(Hb[op[i] + tt], w), Hb[oq[i] + tt]);
        }
        if (first && tid < nphi) {
#pragma unroll 1
          for (int tt = 0; tt < nt; ++tt) {
            const double w = msk[tt];
            cfmac(accphi, cscale(Cb[pi * CS + tt], w), Cb[pj * CS + tt]);
            weight += w;
          }
        }
        __syncthreads();  // rlam is rewritten by the next tile
      }
    }
    if (loss) {  // (uniform: every thread reaches the barriers of block_sum)
      const double total = block_sum(term, red);
      // (after a failed pivot this walk is the last: the kept state fills the entries that remain)
      if (tid == 0)
        for (int k = s; k <= (failed ? n_steps : s); ++k)
          loss[((long long)f * N + n) * slot_stride + (long long)k * B + b] = total * inv_t;
    }
    if (last) break;

    // ---- Phi_s (first walk of the mask form) and R (packed upper triangle) to LDS
    if (first && tid < nphi) {
      c128 v = cscale(accphi, 1.0 / (weight < WPD_EPS ? WPD_EPS : weight));
      if (pi == pj) v.y = 0.0;
      Phis[pi * M + pj] = v;
      Phis[pj * M + pi] = cconj(v);
    }
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const int e = tid + i * WPD_THREADS;
      if (e < NE) Rs[e] = cscale(acc[i], inv_t);
    }
    __syncthreads();
    if (first && Phi_out)
      for (int e = tid; e < M * M; e += WPD_THREADS) Phi_out[bfn * M * M + e] = Phis[e];
    // the loading: every thread adds the diagonal in the same order, the owners of the diagonal add
    double trace = 0.0;
    for (int p = 0; p < Lb; ++p) trace += Rs[wpd_tri(Lb, p, p)].x;
    __syncthreads();
    if (tid < Lb) {
      const int r = wpd_tri(Lb, tid, tid);
      Rs[r] = cmake(Rs[r].x + loading * (trace / (double)Lb), 0.0);
    }
    __syncthreads();
    if (keep && R_out) {
      for (int e = tid; e < Lb * Lb; e += WPD_THREADS) {
        const int p = e / Lb, q = e % Lb;
        R_out[bfn * Lb * Lb + e] = p <= q ? Rs[wpd_tri(Lb, p, q)] : cconj(Rs[wpd_tri(Lb, q, p)]);
      }
      __syncthreads();
    }

    // ---- Cholesky R = U^H U in place, right-looking: row j <- row j / sqrt(pivot), then
    // A[k][i] -= conj(U[j][k]) U[j][i] for j < k <= i
    const int ty = tid >> 4, tx = tid & 15;
#pragma unroll 1
    for (int j = 0; j < Lb; ++j) {
      const int rj = wpd_tri(Lb, j, j);
      const double d = Rs[rj].x;
      if (!(d > 0.0) || !wpd_finite(d)) {  // (uniform)
        failed = true;
        break;
      }
      const double root = sqrt(d), ir = 1.0 / root;
      __syncthreads();  // everybody has read the pivot
      if (tid == 0) {
        Rs[rj] = cmake(root, 0.0);
        invd[j] = ir;
      }
      for (int i = j + 1 + tid; i < Lb; i += WPD_THREADS) Rs[rj + i - j] = cscale(Rs[rj + i - j], ir);
      __syncthreads();
      for (int k = j + 1 + ty; k < Lb; k += 16) {
        const c128 ujk = Rs[rj + k - j];
        const int rk = wpd_tri(Lb, k, k);
        for (int i = k + tx; i < Lb; i += 16) cfmsc(Rs[rk + i - k], ujk, Rs[rj + i - j]);
      }
      __syncthreads();
    }
    if (failed) {
      __syncthreads();
      if (tid == 0 && info) atomicAdd(info, 1);
      continue;  // the last walk, from the W this iteration started from
    }
    if (keep && U_out) {
      for (int e = tid; e < Lb * Lb; e += WPD_THREADS) {
        const int p = e / Lb, q = e % Lb;
        U_out[bfn * Lb * Lb + e] = p <= q ? Rs[wpd_tri(Lb, p, q)] : cmake(0.0, 0.0);
      }
    }

    // ---- the right-hand sides: e_0 .. e_{M-1} (mask form) or [v; 0] (steering form); then
    // U^H z = rhs and U g = z: thread e owns (row e / NR, right-hand side e % NR); in step j the rows
    // behind j take the finished row j, one barrier per step
    const int LR = Lb * NR;
    int row[2], col[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + i * WPD_THREADS;
      row[i] = e < LR ? e / NR : -1;
      col[i] = e < LR ? e % NR : 0;
      if (row[i] >= 0) {
        c128 v = cmake(0.0, 0.0);
        if (steer) {
          if (row[i] < M) v = Vs[row[i]];
        } else if (row[i] == col[i]) {
          v = cmake(1.0, 0.0);
        }
        Zs[row[i] * NR + col[i]] = v;
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < Lb; ++j) {
      const int rj = wpd_tri(Lb, j, j);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (row[i] > j)
          cfmsc(Zs[row[i] * NR + col[i]], Rs[rj + row[i] - j], cscale(Zs[j * NR + col[i]], invd[j]));
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (row[i] >= 0) Zs[row[i] * NR + col[i]] = cscale(Zs[row[i] * NR + col[i]], invd[row[i]]);
    __syncthreads();
#pragma unroll 1
    for (int j = Lb - 1; j >= 0; --j) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (row[i] >= 0 && row[i] < j)
          cfms(Zs[row[i] * NR + col[i]], Rs[wpd_tri(Lb, row[i], j)],
               cscale(Zs[j * NR + col[i]], invd[j]));
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (row[i] >= 0) Zs[row[i] * NR + col[i]] = cscale(Zs[row[i] * NR + col[i]], invd[row[i]]);
    __syncthreads();

    // ---- the new filter.  Thread l < Lb holds the numerator of wb[l]; the terms of the denominator
    // go through LDS and every thread adds them in the same order.
    c128 num = cmake(0.0, 0.0);
    if (steer) {
      if (tid < Lb) num = cmulc(Zs[tid], Vs[ref]);  // a[l] conj(v_ref)
      if (tid < M) {                                // conj(v_m) a_m
        const c128 d = cmulc(Zs[tid], Vs[tid]);
        red[2 * tid] = d.x;
        red[2 * tid + 1] = d.y;
      }
    } else {
      if (tid < Lb)
        for (int k = 0; k < M; ++k) cfma(num, Zs[tid * M + k], Phis[k * M + ref]);  // A[l, ref]
      if (tid < M) {                                                                // A[m, m]
        c128 d = cmake(0.0, 0.0);
        for (int k = 0; k < M; ++k) cfma(d, Zs[tid * M + k], Phis[k * M + tid]);
        red[2 * tid] = d.x;
        red[2 * tid + 1] = 0.0;  // (the trace of a product of two Hermitian matrices is real)
      }
    }
    __syncthreads();
    c128 den = cmake(0.0, 0.0);
    for (int m = 0; m < M; ++m) den = cadd(den, cmake(red[2 * m], red[2 * m + 1]));
    const bool usable = wpd_finite(den.x) && wpd_finite(den.y) && (den.x != 0.0 || den.y != 0.0);
    if (tid < Lb) {
      c128 wb = cmake(0.0, 0.0);
      if (usable) wb = steer ? cdiv(num, den) : cmake(num.x / den.x, num.y / den.x);
      Ws[tid] = cconj(wb);
    }
    __syncthreads();
  }
  if (n_steps > 0)
    for (int e = tid; e < Lb; e += WPD_THREADS) Wb[e] = Ws[e];
}

template <int NPT, bool RESIDENT>
static int launch_wpd_as(const c128 *X, const double *mask, const c128 *V, c128 *W, c128 *Phi,
                         c128 *Y, int B, int M, int N, int F, int T, int K, int D, int ref,
                         double loading, int floor_kind, double eps, int n_steps, double *loss,
                         long long slot_stride, int *info, double *lam, c128 *R, c128 *U,
                         hipStream_t st) {
  const WpdLds need = wpd_lds(M, K, T, RESIDENT);
  const size_t smem = need.fixed_bytes + need.slab_bytes;
  if (smem > 64 * 1024) {
    // (granted once per instantiation and device, not on every launch)
    static size_t granted[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (smem > granted[dev]) {
      hipError_t e = hipFuncSetAttribute((const void *)k_wpd<NPT, RESIDENT>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      if (e != hipSuccess) return fail(SSSPY_ERR_HIP, hipGetErrorString(e));
      granted[dev] = smem;
    }
  }
  hipLaunchKernelGGL((k_wpd<NPT, RESIDENT>), dim3((unsigned)((long long)F * N), (unsigned)B),
                     dim3(WPD_THREADS), smem, st, X, mask, V, W, Phi, Y, B, M, N, F, T, K, D, ref,
                     loading, floor_kind, eps, n_steps, loss, slot_stride, info, lam, R, U);
  return check_launch("k_wpd");
}

static int wpd_check(int B, int M, int N, int F, int T, int K, int D, int floor_kind,
                     const char **why) {
  *why = nullptr;
  if (B <= 0 || F <= 0 || T <= 0 || K < 0 || M < 1 || N < 1 || D < 1 ||
      floor_kind < SSSPY_FLOOR_NONE || floor_kind > SSSPY_FLOOR_ADD) {
    *why = "wpd: bad argument (sizes positive, taps >= 0, delay >= 1, a floor the kernels apply)";
    return SSSPY_ERR_BADARG;
  }
  if (M > WPD_MAX_CHANNELS || ((long long)K + 1) * M > WPD_MAX_ORDER || N > WPD_MAX_SOURCES ||
      B > 65535 || T > (1 << 30) || (long long)F * N > 0x7fffffffLL) {
    *why = "wpd: 1..8 channels, (taps + 1) * n_channels <= 64, 1..16 sources, up to 65535 mixtures";
    return SSSPY_ERR_UNSUPPORTED;
  }
  return SSSPY_OK;
}

static int launch_wpd(const void *X, const double *mask, const void *V, void *W, void *Phi, void *Y,
                      int B, int M, int N, int F, int T, int K, int D, int ref, double loading,
                      int floor_kind, double eps, int n_steps, double *loss, long long slot_stride,
                      int *info, double *lam, void *R, void *U, int route, void *stream) {
  const char *why;
  const int rc = wpd_check(B, M, N, F, T, K, D, floor_kind, &why);
  if (rc != SSSPY_OK) return fail(rc, why);
  SSSPY_REQUIRE(X && W && X != Y && n_steps >= 0 && (n_steps > 0 || Y || loss), "wpd: bad argument");
  SSSPY_REQUIRE(n_steps == 0 || mask || V, "wpd: an iteration needs the masks or the steering vectors");
  SSSPY_REQUIRE(ref >= 0 && ref < M, "wpd: 0 <= reference_id < n_channels");
  SSSPY_REQUIRE(loading >= 0.0 && loading <= 1.79769313486231570815e308,
                "wpd: diagonal_loading is finite and >= 0");
  SSSPY_REQUIRE(!loss || slot_stride >= ((long long)n_steps + 1) * B,
                "wpd: slot_stride >= (n_steps + 1) B");
  SSSPY_REQUIRE(route >= SSSPY_WPD_ROUTE_AUTO && route <= SSSPY_WPD_ROUTE_STREAMING,
                "wpd: route is one of SSSPY_WPD_ROUTE_*");
  const bool resident = route != SSSPY_WPD_ROUTE_STREAMING && wpd_resident(M, K, T);
  const int Lb = (K + 1) * M;
  const int npt = (Lb * (Lb + 1) / 2 + WPD_THREADS - 1) / WPD_THREADS;
  D = D < T ? D : T;  // (no frame has a history from delay = n_frames on)
#define WPD_CASE(NPT_)                                                                             \
  case NPT_:                                                                                       \
    return resident                                                                                \
               ? launch_wpd_as<NPT_, true>((const c128 *)X, mask, (const c128 *)V, (c128 *)W,      \
                                           (c128 *)Phi, (c128 *)Y, B, M, N, F, T, K, D, ref,       \
                                           loading, floor_kind, eps, n_steps, loss, slot_stride,   \
                                           info, lam, (c128 *)R, (c128 *)U, as_stream(stream))     \
               : launch_wpd_as<NPT_, false>((const c128 *)X, mask, (const c128 *)V, (c128 *)W,     \
                                            (c128 *)Phi, (c128 *)Y, B, M, N, F, T, K, D, ref,      \
                                            loading, floor_kind, eps, n_steps, loss, slot_stride,  \
                                            info, lam, (c128 *)R, (c128 *)U, as_stream(stream))
  static_assert(WPD_MAX_NPT == 9, "the cases below cover 1..WPD_MAX_NPT entries per thread");
  switch (npt) {
    WPD_CASE(1);
    WPD_CASE(2);
    WPD_CASE(3);
    WPD_CASE(4);
    WPD_CASE(5);
    WPD_CASE(6);
    WPD_CASE(7);
    WPD_CASE(8);
    WPD_CASE(9);
  }
#undef WPD_CASE
  return fail(SSSPY_ERR_INTERNAL, "wpd: no kernel for this order");
}

}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_wpd_route(int B, int M, int N, int F, int T, int taps, int *lds_bytes) {
  const char *why;
  if (wpd_check(B, M, N, F, T, taps, 1, SSSPY_FLOOR_NONE, &why) != SSSPY_OK) return -1;
  const bool resident = wpd_resident(M, taps, T);
  if (lds_bytes) {
    const WpdLds need = wpd_lds(M, taps, T, resident);
    *lds_bytes = (int)(need.fixed_bytes + need.slab_bytes);
  }
  return resident ? SSSPY_WPD_ROUTE_RESIDENT : SSSPY_WPD_ROUTE_STREAMING;
}

int ssspy_wpd_steps(const void *X, const double *mask, const void *steering, void *W, void *Phi_s,
                    void *Y, int B, int M, int N, int F, int T, int taps, int delay, int reference_id,
                    double diagonal_loading, int floor_kind, double floor_eps, int n_steps,
                    double *loss_data, long long slot_stride, int *info, int route, void *stream) {
  SSSPY_REQUIRE(n_steps >= 1, "wpd_steps: n_steps >= 1");
  return launch_wpd(X, mask, steering, W, Phi_s, Y, B, M, N, F, T, taps, delay, reference_id,
                    diagonal_loading, floor_kind, floor_eps, n_steps, loss_data, slot_stride, info,
                    nullptr, nullptr, nullptr, route, stream);
}

int ssspy_wpd_step(const void *X, const double *mask, const void *steering, void *W, void *Phi_s,
                   void *Y, int B, int M, int N, int F, int T, int taps, int delay, int reference_id,
                   double diagonal_loading, int floor_kind, double floor_eps, int *info,
                   double *lambda, void *R, void *U, int route, void *stream) {
  return launch_wpd(X, mask, steering, W, Phi_s, Y, B, M, N, F, T, taps, delay, reference_id,
                    diagonal_loading, floor_kind, floor_eps, 1, nullptr, 0, info, lambda, R, U, route,
                    stream);
}

int ssspy_wpd_apply(const void *X, const void *W, void *Y, int B, int M, int N, int F, int T, int taps,
                    int delay, int floor_kind, double floor_eps, double *loss_data,
                    long long slot_stride, int route, void *stream) {
  // (n_steps = 0: the last walk alone; W is read, never stored)
  return launch_wpd(X, nullptr, nullptr, const_cast<void *>(W), nullptr, Y, B, M, N, F, T, taps,
                    delay, 0, 0.0, floor_kind, floor_eps, 0, loss_data, slot_stride, nullptr, nullptr,
                    nullptr, nullptr, route, stream);
}

}  // extern "C"
