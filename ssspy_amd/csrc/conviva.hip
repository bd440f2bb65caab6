// IVA with joint dereverberation (convolutional AuxIVA): the statistics kernel and the composition
// of the convolutional filters.
// Nakatani et al., "Computationally efficient and versatile framework for joint optimization of blind
// speech separation and dereverberation", Interspeech 2020 (the source-wise factorisation); Ikeshita,
// Ito, Nakatani, Kinoshita, "Independent low-rank matrix analysis with decorrelation learning", WASPAA
// 2019.
//
// Per (mixture, bin, source), with x_t in C^M the mixture at frame t, K >= 0 taps, delay D >= 1,
// L = K M and Lb = (K + 1) M:
//   xb_t in C^Lb: block 0 is x_t, block j = 1..K is x_{t - D - (j - 1)} (zero before the first frame)
//   Rb = (1 / T) sum_t phi_t xb_t xb_t^H,  C = Rb[:M, :M],  P = Rb[M:, :M],  R = Rb[M:, M:]
//   R += loading (Re tr R / L) I  (K > 0)
//   G = R^-1 P through the Cholesky factorisation R = U^H U,  Sigma = C - P^H G
// phi (B, N, T) are the auxiliary weights of AuxIVA, formed by ssspy_iva_weight from the frame powers
// of the current estimate.  Sigma goes to ssspy_update_by_ip1 as the weighted covariance of the
// source; ssspy_conviva_compose then forms the convolutional filter wb = [q; -G q] from the demixing
// row and stores it conjugated, W[l] = conj(wb[l]), so that ssspy_wpd_apply forms y = W xb.
// ILRMA with joint dereverberation (ILRMA-T) takes the same statistics with weights that depend on
// the bin, phi_nft = (T V)_nft^(-2/p), formed inside the kernel (ssspy_conviva_statistics_nmf), and
// adds the power normalisation of the convolutional state (ssspy_convilrma_normalize).
//
// The frame walk is that of csrc/wpd.hip (the structure is copied, not shared: wpd.hip interleaves
// its power pass and the sums of Phi_s with the walk): tiles of CONVIVA_TILE frames,
// every thread owns up to NPT fixed entries of the packed upper triangle of Rb and walks the frames of
// a tile in order.  No atomics on the sums, the same bits on every run and on both routes.  Then the
// Cholesky factorisation of the trailing L x L block in place in LDS (right-looking), the forward and
// back substitutions by rows for the M right-hand sides P, and Sigma.
//
// LDS (dynamic; 160 KiB per CU decide the bounds):
//   fixed   Rb packed Lb (Lb + 1) / 2, the right-hand sides L M (c128), 1 / diag (Lb), the weights of
//           a tile (CONVIVA_TILE) and 16 doubles: 33280 + 7168 + 512 + 2048 + 128 = 43136 bytes at
//           M = 8, Lb = 64
//   RESIDENT  the bin's slab, M rows of max(K - 1, 0) zeros and the T frames: at most
//           CONVIVA_SLAB_LDS_BYTES = 48 KiB (the rule of wpd.hip), 92288 bytes with the above
//   otherwise per tile the history rows (CONVIVA_TILE + max(K - 1, 0) frames, zeros before frame 0)
//           and the current rows (CONVIVA_TILE frames), re-read from memory: at most
//           8 * (262 + 256) * 16 = 66304, 109440 bytes with the above
#include "common.hpp"

namespace ssspy {

constexpr int CONVIVA_THREADS = 256;
constexpr int CONVIVA_TILE = 256;  // frames per tile
constexpr int CONVIVA_SLAB_LDS_BYTES = 48 * 1024;
constexpr int CONVIVA_MAX_NPT =
    (SSSPY_CONVIVA_MAX_ORDER * (SSSPY_CONVIVA_MAX_ORDER + 1) / 2 + CONVIVA_THREADS - 1) /
    CONVIVA_THREADS;

// index of (p, q), p <= q, in the row-major upper triangle of an L x L matrix
__device__ __forceinline__ int conviva_tri(int L, int p, int q) {
  return p * L - p * (p - 1) / 2 + (q - p);
}

__device__ __forceinline__ bool conviva_finite(double v) {
  return fabs(v) <= 1.79769313486231570815e308;
}

struct ConvivaLds {
  size_t fixed_bytes, slab_bytes;
};
static int conviva_pad(int K) { return K > 1 ? K - 1 : 0; }
static ConvivaLds conviva_lds(int M, int K, int T, bool resident) {
  const size_t Lb = (size_t)(K + 1) * M, L = (size_t)K * M, pad = (size_t)conviva_pad(K);
  ConvivaLds s;
  s.fixed_bytes = (Lb * (Lb + 1) / 2 + L * M) * sizeof(c128) +
                  (((Lb + 1) & ~(size_t)1) + CONVIVA_TILE + 16) * sizeof(double);
  s.slab_bytes = resident ? (size_t)M * (T + pad) * sizeof(c128)
                          : (size_t)M * (2 * CONVIVA_TILE + pad) * sizeof(c128);
  return s;
}
static bool conviva_resident(int M, int K, int T) {
  return (long long)M * ((long long)T + conviva_pad(K)) * (long long)sizeof(c128) <=
         CONVIVA_SLAB_LDS_BYTES;
}

// grid: (F * M, B), 256 threads; block x = f * M + n (as many sources as channels).
//   Sigma (B, F, M, M, M): the Schur complement of source n as a full Hermitian matrix.
//   G (B, F, M, L, M): R^-1 P (not touched with K = 0).
//   failed (B, F, M): bit 0 = this launch met a pivot that is not positive and finite (Sigma and G of
//   the triple are then not written), bit 1 = some launch since the caller zeroed the word did; info[0]
//   is bumped when bit 1 is set for the first time: once per triple and call.
//   Rb_out (B, F, M, Lb, Lb) (full Hermitian, loading included), U_out (B, F, M, L, L) (upper
//   triangular, zeros below the diagonal): tests; each may be NULL.
//
// The weights of a tile come from one of two sources, a compile-time choice of the one body:
//   NMF = false  phi (B, N, T), one weight per (source, frame): IVA.  `nmf` is not read.
//   NMF = true   phi_nft = (sum_k basis[b,n,f,k] activation[b,n,k,t])^(-2/domain), formed by the
//                workgroup itself for the tile, one thread per frame, k ascending (1 / s with domain
//                = 2: no pow); the basis row of the (b, n, f) is staged once in LDS behind the slab,
//                the activation is read coalesced along t: ILRMA.  `phi` is not read.  Not floored: a
//                sum of zero gives phi = inf, R is not finite and the pivot check fails the triple.
// The frame-weight instantiations keep the argument list they had in front of `nmf` and compile to
// the instructions they compiled to before there was a second source.
struct NmfWeights {
  const double *basis;       // (B, N, F, Kb)
  const double *activation;  // (B, N, Kb, T)
  double *phi_out;           // (B, N, F, T) or NULL: tests
  double domain;
  int Kb;
};

template <int NPT, bool RESIDENT, bool NMF>
__global__ __launch_bounds__(CONVIVA_THREADS) void k_conviva(
    const c128 *__restrict__ X, const double *__restrict__ phi, c128 *Sigma, c128 *G, int B, int M,
    int F, int T, int K, int D, double loading, int *info, int *failed, c128 *Rb_out, c128 *U_out,
    const NmfWeights nmf) {
  extern __shared__ c128 lds[];
  const int tid = threadIdx.x;
  const int N = M;
  const int f = blockIdx.x / N, n = blockIdx.x % N, b = blockIdx.y;
  const int Lb = (K + 1) * M, L = K * M, NE = Lb * (Lb + 1) / 2;
  c128 *Rs = lds;
  c128 *Zs = Rs + NE;  // (L, M): the right-hand sides P, then the solutions G
  double *invd = reinterpret_cast<double *>(Zs + L * M);
  double *wgt = invd + ((Lb + 1) & ~1);
  double *red = wgt + CONVIVA_TILE;  // 16 doubles (keeps the slab 16-byte aligned)
  c128 *slab = reinterpret_cast<c128 *>(red + 16);
  const int pad = K > 1 ? K - 1 : 0;
  // history (m, frame t0 + tt, block j >= 1) at Hb[m * HS + tt - (j - 1)], current at Cb[m * CS + tt]
  const int HS = RESIDENT ? T + pad : CONVIVA_TILE + pad;
  const int CS = RESIDENT ? HS : CONVIVA_TILE;
  c128 *Hs = slab, *Cs = RESIDENT ? slab + pad : slab + (size_t)M * HS;
  // Cb - Hb, the same in every tile: the operands of the sums are all addressed from Hb
  const int cur = RESIDENT ? D : M * HS - pad;

  const long long row_stride = (long long)F * T;
  const c128 *__restrict__ Xb = X + ((long long)b * M * F + f) * T;  // row m at Xb + m * row_stride
  const long long bfn = ((long long)b * F + f) * N + n;
  const double *__restrict__ prow = NMF ? nullptr : phi + ((long long)b * N + n) * T;
  // NMF = true: the activation of (b, n), (Kb, T); the basis row in LDS; phi_out of (b, n, f)
  const double *__restrict__ arow = nullptr;
  double *bs = nullptr, *pout = nullptr;
  if constexpr (NMF) {
    bs = reinterpret_cast<double *>(slab + (size_t)M * (RESIDENT ? HS : HS + CS));
    arow = nmf.activation + ((long long)b * N + n) * nmf.Kb * T;
    if (nmf.phi_out) pout = nmf.phi_out + (((long long)b * N + n) * F + f) * T;
    if (tid < nmf.Kb) bs[tid] = nmf.basis[(((long long)b * N + n) * F + f) * nmf.Kb + tid];
  }

  if (RESIDENT) {
    for (int m = 0; m < M; ++m) {
      for (int j = tid; j < pad; j += CONVIVA_THREADS) slab[m * HS + j] = cmake(0.0, 0.0);
      for (int j = tid; j < T; j += CONVIVA_THREADS) slab[m * HS + pad + j] = Xb[m * row_stride + j];
    }
  }
  // the entries this thread owns: offsets of their two operands from Hb, and whether both lie in
  // block 0 (the only entries the frames before D add to)
  int op[NPT], oq[NPT];
  unsigned both_current = 0;
#pragma unroll
  for (int i = 0; i < NPT; ++i) {
    int e = tid + i * CONVIVA_THREADS;
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
  __syncthreads();

  c128 acc[NPT];
#pragma unroll
  for (int i = 0; i < NPT; ++i) acc[i] = cmake(0.0, 0.0);
#pragma unroll 1
  for (int t0 = 0; t0 < T; t0 += CONVIVA_TILE) {
    const int nt = min(CONVIVA_TILE, T - t0);
    const c128 *Hb;
    __syncthreads();  // the previous tile (its weights, its rows) has been read
    if (RESIDENT) {
      Hb = slab + pad + (t0 - D);  // (read only at frames t >= D: never below the zeros)
    } else {
      const int first_frame = t0 - D - pad;  // frame of history column 0
      for (int m = 0; m < M; ++m) {
        if (K > 0)
          for (int j = tid; j < nt + pad; j += CONVIVA_THREADS) {
            const int fr = first_frame + j;
            Hs[m * HS + j] = fr >= 0 && fr < T ? Xb[m * row_stride + fr] : cmake(0.0, 0.0);
          }
        for (int j = tid; j < nt; j += CONVIVA_THREADS) Cs[m * CS + j] = Xb[m * row_stride + t0 + j];
      }
      Hb = Hs + pad;
    }
    if constexpr (NMF) {
      // (bs was written before the barrier that follows the entry table)
      if (tid < nt) {
        double sum = 0.0;
        for (int k = 0; k < nmf.Kb; ++k) sum += bs[k] * arow[(long long)k * T + t0 + tid];
        const double w = nmf.domain == 2.0 ? 1.0 / sum : pow(sum, -2.0 / nmf.domain);
        wgt[tid] = w;
        if (pout) pout[t0 + tid] = w;
      }
    } else {
      if (tid < nt) wgt[tid] = prow[t0 + tid];
    }
    __syncthreads();
    // ---- sums: frames in order inside every thread; the frames before D have no history
    const int head = min(nt, max(0, D - t0));
#pragma unroll 1
    for (int tt = 0; tt < head; ++tt) {
      const double w = wgt[tt];
#pragma unroll
      for (int i = 0; i < NPT; ++i)
        if ((both_current >> i) & 1u) cfmac(acc[i], cscale(Hb[op[i] + tt], w), Hb[oq[i] + tt]);
    }
#pragma unroll 1
    for (int tt = head; tt < nt; ++tt) {
      const double w = wgt[tt];
#pragma unroll
      for (int i = 0; i < NPT; ++i) cfmac(acc[i], cscale(Hb[op[i] + tt], w), Hb[oq[i] + tt]);
    }
  }

  // ---- Rb (packed upper triangle) to LDS, the diagonal exactly real
  const double inv_t = 1.0 / (double)T;
#pragma unroll
  for (int i = 0; i < NPT; ++i) {
    const int e = tid + i * CONVIVA_THREADS;
    if (e < NE) Rs[e] = cscale(acc[i], inv_t);
  }
  __syncthreads();
  if (tid < Lb) {
    const int r = conviva_tri(Lb, tid, tid);
    Rs[r] = cmake(Rs[r].x, 0.0);
  }
  __syncthreads();
  // the loading of R: every thread adds the diagonal in the same order, the owners of the diagonal add
  if (K > 0) {
    double trace = 0.0;
    for (int p = M; p < Lb; ++p) trace += Rs[conviva_tri(Lb, p, p)].x;
    __syncthreads();
    if (tid >= M && tid < Lb) {
      const int r = conviva_tri(Lb, tid, tid);
      Rs[r] = cmake(Rs[r].x + loading * (trace / (double)L), 0.0);
    }
    __syncthreads();
  }
  if (Rb_out) {
    for (int e = tid; e < Lb * Lb; e += CONVIVA_THREADS) {
      const int p = e / Lb, q = e % Lb;
      Rb_out[bfn * Lb * Lb + e] =
          p <= q ? Rs[conviva_tri(Lb, p, q)] : cconj(Rs[conviva_tri(Lb, q, p)]);
    }
  }
  // the right-hand sides P[l][m] = Rb[M + l][m] = conj(Rb[m][M + l]); rows 0..M-1 of Rs stay as they
  // are (the factorisation works on rows M..): Sigma reads P^H from them
  for (int e = tid; e < L * M; e += CONVIVA_THREADS)
    Zs[e] = cconj(Rs[conviva_tri(Lb, e % M, M + e / M)]);
  __syncthreads();

  // ---- Cholesky R = U^H U in place on rows M.. of the triangle, right-looking: row j <- row j /
  // sqrt(pivot), then A[k][i] -= conj(U[j][k]) U[j][i] for j < k <= i
  const int ty = tid >> 4, tx = tid & 15;
  bool bad = false;
#pragma unroll 1
  for (int j = M; j < Lb; ++j) {
    const int rj = conviva_tri(Lb, j, j);
    const double d = Rs[rj].x;
    if (!(d > 0.0) || !conviva_finite(d)) {  // (uniform)
      bad = true;
      break;
    }
    const double root = sqrt(d), ir = 1.0 / root;
    __syncthreads();  // everybody has read the pivot
    if (tid == 0) {
      Rs[rj] = cmake(root, 0.0);
      invd[j] = ir;
    }
    for (int i = j + 1 + tid; i < Lb; i += CONVIVA_THREADS) Rs[rj + i - j] = cscale(Rs[rj + i - j], ir);
    __syncthreads();
    for (int k = j + 1 + ty; k < Lb; k += 16) {
      const c128 ujk = Rs[rj + k - j];
      const int rk = conviva_tri(Lb, k, k);
      for (int i = k + tx; i < Lb; i += 16) cfmsc(Rs[rk + i - k], ujk, Rs[rj + i - j]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int old = failed[bfn];
    if (bad) {
      if (!(old & 2) && info) atomicAdd(info, 1);
      failed[bfn] = 3;
    } else {
      failed[bfn] = old & 2;
    }
  }
  if (bad) return;  // Sigma and G of the triple stay what they were
  if (U_out) {
    for (int e = tid; e < L * L; e += CONVIVA_THREADS) {
      const int p = e / L, q = e % L;
      U_out[bfn * L * L + e] = p <= q ? Rs[conviva_tri(Lb, M + p, M + q)] : cmake(0.0, 0.0);
    }
  }

  // ---- U^H z = P and U g = z: thread e owns (row e / M, right-hand side e % M); in step j the rows
  // behind j take the finished row j, one barrier per step
  const int LR = L * M;
  int row[2], col[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = tid + i * CONVIVA_THREADS;
    row[i] = e < LR ? e / M : -1;
    col[i] = e < LR ? e % M : 0;
  }
#pragma unroll 1
  for (int j = 0; j < L; ++j) {
    const int rj = conviva_tri(Lb, M + j, M + j);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (row[i] > j)
        cfmsc(Zs[row[i] * M + col[i]], Rs[rj + row[i] - j], cscale(Zs[j * M + col[i]], invd[M + j]));
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
    if (row[i] >= 0) Zs[row[i] * M + col[i]] = cscale(Zs[row[i] * M + col[i]], invd[M + row[i]]);
  __syncthreads();
#pragma unroll 1
  for (int j = L - 1; j >= 0; --j) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (row[i] >= 0 && row[i] < j)
        cfms(Zs[row[i] * M + col[i]], Rs[conviva_tri(Lb, M + row[i], M + j)],
             cscale(Zs[j * M + col[i]], invd[M + j]));
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
    if (row[i] >= 0) Zs[row[i] * M + col[i]] = cscale(Zs[row[i] * M + col[i]], invd[M + row[i]]);
  __syncthreads();
  for (int e = tid; e < LR; e += CONVIVA_THREADS) G[bfn * LR + e] = Zs[e];

  // ---- Sigma = C - P^H G: thread e < M (M + 1) / 2 owns (a, c), a <= c, and stores both halves;
  // (P^H)[a][l] = Rb[a][M + l] is row a of the triangle
  if (tid < M * (M + 1) / 2) {
    int e = tid, a = 0;
    while (e >= M - a) {
      e -= M - a;
      ++a;
    }
    const int c = a + e;
    c128 v = Rs[conviva_tri(Lb, a, c)];
    const int ra = conviva_tri(Lb, a, M);
    for (int l = 0; l < L; ++l) cfms(v, Rs[ra + l], Zs[l * M + c]);
    if (a == c) v.y = 0.0;
    Sigma[bfn * M * M + a * M + c] = v;
    Sigma[bfn * M * M + c * M + a] = cconj(v);
  }
}

// W (B, F, N, Lb) from the demixing rows Q (B, F, N, M) and G (B, F, N, L, M): W[:M] = Q row,
// W[M + l] = conj(-(G q)[l]) = -sum_m conj(G[l][m]) Q[m], q = conj(Q row).  One thread per entry; the
// row of a triple whose bit 0 of `failed` is set is not touched.
__global__ __launch_bounds__(256) void k_conviva_compose(const c128 *__restrict__ Q,
                                                         const c128 *__restrict__ G, c128 *W,
                                                         const int *__restrict__ failed,
                                                         long long rows, int M, int Lb) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= rows * Lb) return;
  const long long bfn = e / Lb;
  const int l = (int)(e % Lb);
  if (failed && (failed[bfn] & 1)) return;
  const c128 *q = Q + bfn * M;
  if (l < M) {
    W[e] = q[l];
    return;
  }
  const c128 *g = G + (bfn * (Lb - M) + (l - M)) * M;
  c128 v = cmake(0.0, 0.0);
  for (int m = 0; m < M; ++m) cfmsc(v, g[m], q[m]);
  W[e] = v;
}

// ---- power normalisation of the ILRMA source model: psi_n = floor(sqrt(mean_{f,t} |y_nft|^2)); the
// estimate, the whole row of the convolutional filter (all Lb entries) and the basis take the same
// psi, so Y stays W xb to one rounding per entry.
// acc[(b N + n) slots + s] = sum of |y|^2 over CONVILRMA_POWER_BINS bin rows (one contiguous run):
// one slot per block, added in slot order by the consumer: no atomics
constexpr int CONVILRMA_POWER_BINS = 16;

__global__ __launch_bounds__(256) void k_convilrma_power(const c128 *__restrict__ Y, double *acc,
                                                         int N, int F, int T) {
  __shared__ double scratch[4];
  const int n = blockIdx.y, b = blockIdx.z;
  const int f0 = blockIdx.x * CONVILRMA_POWER_BINS;
  const long long len = (long long)min(CONVILRMA_POWER_BINS, F - f0) * T;
  const c128 *run = Y + (((long long)b * N + n) * F + f0) * T;
  double local = 0.0;
  for (long long e = threadIdx.x; e < len; e += blockDim.x) local += cabs2(run[e]);
  const double total = block_sum(local, scratch);
  if (threadIdx.x == 0) acc[((long long)b * N + n) * gridDim.x + blockIdx.x] = total;
}

// grid: (F, N, B).  Y (B, N, F, T) /= psi, W (B, F, N, Lb) /= psi, basis (B, N, F, Kb) /= psi^p.
__global__ __launch_bounds__(256) void k_convilrma_scale(c128 *Y, c128 *W, double *basis,
                                                         const double *__restrict__ acc, int slots,
                                                         int N, int F, int T, int Lb, int Kb,
                                                         double p, int floor_kind, double eps) {
  const int f = blockIdx.x, n = blockIdx.y, b = blockIdx.z;
  const double *a = acc + ((long long)b * N + n) * slots;
  double v = 0.0;
  for (int s = 0; s < slots; ++s) v += a[s];  // (every thread the same sum)
  const double psi = apply_floor(sqrt(v / ((double)F * (double)T)), floor_kind, eps);
  c128 *yrow = Y + (((long long)b * N + n) * F + f) * T;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const c128 y = yrow[t];
    yrow[t] = cmake(y.x / psi, y.y / psi);
  }
  c128 *wrow = W + (((long long)b * F + f) * N + n) * Lb;
  for (int l = threadIdx.x; l < Lb; l += blockDim.x) {
    const c128 w = wrow[l];
    wrow[l] = cmake(w.x / psi, w.y / psi);
  }
  const double pp = p == 2.0 ? psi * psi : pow(psi, p);
  double *trow = basis + (((long long)b * N + n) * F + f) * Kb;
  for (int k = threadIdx.x; k < Kb; k += blockDim.x) trow[k] = trow[k] / pp;
}

// One launch of the statistics kernel; nmf == NULL: the frame weights phi.
template <int NPT, bool RESIDENT, bool NMF>
static int launch_conviva_as(const c128 *X, const double *phi, const NmfWeights *nmf, c128 *Sigma,
                             c128 *G, int B, int M, int F, int T, int K, int D, double loading,
                             int *info, int *failed, c128 *Rb, c128 *U, hipStream_t st) {
  const ConvivaLds need = conviva_lds(M, K, T, RESIDENT);
  // (NMF: the basis row behind the slab)
  const size_t smem = need.fixed_bytes + need.slab_bytes + (NMF ? nmf->Kb * sizeof(double) : 0);
  if (smem > 64 * 1024) {
    // (granted once per instantiation and device, not on every launch)
    static size_t granted[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (smem > granted[dev]) {
      hipError_t e = hipFuncSetAttribute((const void *)k_conviva<NPT, RESIDENT, NMF>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      if (e != hipSuccess) return fail(SSSPY_ERR_HIP, hipGetErrorString(e));
      granted[dev] = smem;
    }
  }
  hipLaunchKernelGGL((k_conviva<NPT, RESIDENT, NMF>), dim3((unsigned)((long long)F * M), (unsigned)B),
                     dim3(CONVIVA_THREADS), smem, st, X, phi, Sigma, G, B, M, F, T, K, D, loading,
                     info, failed, Rb, U, NMF ? *nmf : NmfWeights{});
  return check_launch("k_conviva");
}

static int conviva_check(int B, int M, int F, int T, int K, int D, const char **why) {
  *why = nullptr;
  if (B <= 0 || F <= 0 || T <= 0 || K < 0 || M < 1 || D < 1) {
    *why = "conviva: bad argument (sizes positive, taps >= 0, delay >= 1)";
    return SSSPY_ERR_BADARG;
  }
  if (M < SSSPY_CONVIVA_MIN_CHANNELS || M > SSSPY_CONVIVA_MAX_CHANNELS ||
      ((long long)K + 1) * M > SSSPY_CONVIVA_MAX_ORDER || B > 65535 || T > (1 << 30) ||
      (long long)F * M > 0x7fffffffLL) {
    *why = "conviva: 2..8 channels, (taps + 1) * n_channels <= 64, up to 65535 mixtures";
    return SSSPY_ERR_UNSUPPORTED;
  }
  return SSSPY_OK;
}

// Checks and the choice of the instantiation, for either weight source (nmf == NULL: phi).
template <bool NMF>
static int conviva_statistics(const void *X, const double *phi, const NmfWeights *nmf, void *Sigma,
                              void *G, int B, int M, int F, int T, int taps, int delay,
                              double diagonal_loading, int *info, int *failed, void *Rb_out,
                              void *U_out, int route, void *stream) {
  const char *why;
  const int rc = conviva_check(B, M, F, T, taps, delay, &why);
  if (rc != SSSPY_OK) return fail(rc, why);
  const int K = taps;
  SSSPY_REQUIRE(X && (NMF ? nmf->basis && nmf->activation : phi != nullptr) && Sigma && failed &&
                    (G || K == 0),
                "conviva_statistics: bad argument");
  SSSPY_REQUIRE(diagonal_loading >= 0.0 && diagonal_loading <= 1.79769313486231570815e308,
                "conviva_statistics: diagonal_loading is finite and >= 0");
  SSSPY_REQUIRE(route >= SSSPY_CONVIVA_ROUTE_AUTO && route <= SSSPY_CONVIVA_ROUTE_STREAMING,
                "conviva_statistics: route is one of SSSPY_CONVIVA_ROUTE_*");
  const bool resident = route != SSSPY_CONVIVA_ROUTE_STREAMING && conviva_resident(M, K, T);
  const int Lb = (K + 1) * M;
  const int npt = (Lb * (Lb + 1) / 2 + CONVIVA_THREADS - 1) / CONVIVA_THREADS;
  const int D = delay < T ? delay : T;  // (no frame has a history from delay = n_frames on)
#define CONVIVA_CASE(NPT_)                                                                         \
  case NPT_:                                                                                       \
    return resident                                                                                \
               ? launch_conviva_as<NPT_, true, NMF>((const c128 *)X, phi, nmf, (c128 *)Sigma,       \
                                                    (c128 *)G, B, M, F, T, K, D, diagonal_loading, \
                                                    info, failed, (c128 *)Rb_out, (c128 *)U_out,   \
                                                    as_stream(stream))                             \
               : launch_conviva_as<NPT_, false, NMF>((const c128 *)X, phi, nmf, (c128 *)Sigma,      \
                                                     (c128 *)G, B, M, F, T, K, D,                  \
                                                     diagonal_loading, info, failed,               \
                                                     (c128 *)Rb_out, (c128 *)U_out,                \
                                                     as_stream(stream))
  static_assert(CONVIVA_MAX_NPT == 9, "the cases below cover 1..CONVIVA_MAX_NPT entries per thread");
  switch (npt) {
    CONVIVA_CASE(1);
    CONVIVA_CASE(2);
    CONVIVA_CASE(3);
    CONVIVA_CASE(4);
    CONVIVA_CASE(5);
    CONVIVA_CASE(6);
    CONVIVA_CASE(7);
    CONVIVA_CASE(8);
    CONVIVA_CASE(9);
  }
#undef CONVIVA_CASE
  return fail(SSSPY_ERR_INTERNAL, "conviva_statistics: no kernel for this order");
}

}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_conviva_route(int B, int M, int F, int T, int taps, int *lds_bytes) {
  const char *why;
  if (conviva_check(B, M, F, T, taps, 1, &why) != SSSPY_OK) return -1;
  const bool resident = conviva_resident(M, taps, T);
  if (lds_bytes) {
    const ConvivaLds need = conviva_lds(M, taps, T, resident);
    *lds_bytes = (int)(need.fixed_bytes + need.slab_bytes);
  }
  return resident ? SSSPY_CONVIVA_ROUTE_RESIDENT : SSSPY_CONVIVA_ROUTE_STREAMING;
}

int ssspy_conviva_statistics(const void *X, const double *phi, void *Sigma, void *G, int B, int M,
                             int F, int T, int taps, int delay, double diagonal_loading, int *info,
                             int *failed, void *Rb_out, void *U_out, int route, void *stream) {
  return conviva_statistics<false>(X, phi, nullptr, Sigma, G, B, M, F, T, taps, delay,
                                   diagonal_loading, info, failed, Rb_out, U_out, route, stream);
}

int ssspy_conviva_statistics_nmf(const void *X, const double *basis, const double *activation,
                                 void *Sigma, void *G, int B, int M, int F, int T, int taps,
                                 int delay, int n_basis, double domain, double diagonal_loading,
                                 int *info, int *failed, void *Rb_out, void *U_out, double *phi_out,
                                 int route, void *stream) {
  SSSPY_REQUIRE(n_basis >= 1, "conviva_statistics_nmf: bad argument");
  SSSPY_REQUIRE(domain > 0.0 && domain <= 2.0, "conviva_statistics_nmf: domain is in (0, 2]");
  if (n_basis > SSSPY_CONVIVA_MAX_BASIS)
    return fail(SSSPY_ERR_UNSUPPORTED, "conviva_statistics_nmf: up to 32 bases");
  const NmfWeights nmf = {basis, activation, phi_out, domain, n_basis};
  return conviva_statistics<true>(X, nullptr, &nmf, Sigma, G, B, M, F, T, taps, delay,
                                  diagonal_loading, info, failed, Rb_out, U_out, route, stream);
}

size_t ssspy_convilrma_normalize_workspace_bytes(int B, int M, int F) {
  if (B <= 0 || M <= 0 || F <= 0) return 0;
  return (size_t)B * M * ((F + CONVILRMA_POWER_BINS - 1) / CONVILRMA_POWER_BINS) * sizeof(double);
}

int ssspy_convilrma_normalize(void *Y, void *W, double *basis, int B, int M, int F, int T, int taps,
                              int n_basis, double domain, int floor_kind, double floor_eps,
                              void *workspace, size_t workspace_bytes, void *stream) {
  const char *why;
  const int rc = conviva_check(B, M, F, T, taps, 1, &why);
  if (rc != SSSPY_OK) return fail(rc, why);
  SSSPY_REQUIRE(Y && W && basis && n_basis >= 1 && domain > 0.0 && domain <= 2.0,
                "convilrma_normalize: bad argument");
  SSSPY_REQUIRE(workspace && workspace_bytes >= ssspy_convilrma_normalize_workspace_bytes(B, M, F),
                "convilrma_normalize: workspace too small");
  const int slots = (F + CONVILRMA_POWER_BINS - 1) / CONVILRMA_POWER_BINS;
  hipStream_t st = as_stream(stream);
  double *acc = (double *)workspace;
  hipLaunchKernelGGL(k_convilrma_power, dim3(slots, M, B), dim3(256), 0, st, (const c128 *)Y, acc, M,
                     F, T);
  hipLaunchKernelGGL(k_convilrma_scale, dim3(F, M, B), dim3(256), 0, st, (c128 *)Y, (c128 *)W, basis,
                     acc, slots, M, F, T, (taps + 1) * M, n_basis, domain, floor_kind, floor_eps);
  return check_launch("k_convilrma_scale");
}

int ssspy_conviva_compose(const void *Q, const void *G, void *W, const int *failed, int B, int M,
                          int F, int taps, void *stream) {
  const char *why;
  const int rc = conviva_check(B, M, F, 1, taps, 1, &why);
  if (rc != SSSPY_OK) return fail(rc, why);
  SSSPY_REQUIRE(Q && W && Q != W && (G || taps == 0), "conviva_compose: bad argument");
  const long long rows = (long long)B * F * M;
  const int Lb = (taps + 1) * M;
  const long long blocks = (rows * Lb + 255) / 256;
  SSSPY_REQUIRE(blocks <= 0x7fffffffLL, "conviva_compose: too many filters for one launch");
  hipLaunchKernelGGL(k_conviva_compose, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                     (const c128 *)Q, (const c128 *)G, (c128 *)W, failed, rows, M, Lb);
  return check_launch("k_conviva_compose");
}

}  // extern "C"
