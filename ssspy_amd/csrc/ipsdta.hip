// Block-decomposed IPSDTA (GaussIPSDTA / TIPSDTA, MM source model + VCD spatial model).
//   R_ntc = to_psd(sum_k v_nkt T_nkc), an L x L Hermitian matrix per (source, frame, block)
//                                                           (ssspy/bss/ipsdta.py:584-664)
//   basis statistics  P = mean_t v R^-1, Q = mean_t v pi R^-1 y y^H R^-1     (:922-939, :1464-1483)
//   activation        num = sum_c pi Re(u^H T u), den = sum_c Re tr(R^-1 T)   (:991-1006, :1574-1591)
//   VCD covariance    mean_t pi R^-1[b, a] x_a x_b^H                         (:1096-1102, :1711-1718)
//   VCD sweep                                      (ssspy/bss/_update_spatial_model.py:516-608)
//   loss                                                    (ssspy/bss/ipsdta.py:1169-1187, :1840-1866)
// One frame kernel, k_ipsdta_frame<L>, with four modes.  A workgroup of one wave owns a (mixture,
// source, block) and walks the frames 64 at a time, a lane per frame: y = W x for the block's bins,
// R, its factorisation, u = R^-1 y.  What leaves a chunk of 64 frames depends on the mode; sums over
// frames are formed from LDS by the lane that owns the output element, chunk after chunk in frame
// order, so no sum crosses a workgroup and every result has the same bits on every run.
// to_psd's floor (max-flooring of the eigenvalues at 1e-10, whatever flooring_fn the separator
// carries) costs a Jacobi decomposition; it is the identity up to rounding whenever every
// eigenvalue exceeds the floor, which a successful Cholesky factorisation of R - 1e-10 I proves.
// The wave votes: only if one of its 64 matrices fails that test does the wave run the repair.
// fp64 / complex128, no fp64 atomics.
#include "common.hpp"
#include "hermitian.hpp"
#include "smallmat.hpp"

namespace ssspy {

namespace {

constexpr double IPSDTA_PSD_EPS = 1e-10;  // EPS of ssspy/special/psd.py
constexpr int IPSDTA_MAX_L = 8;
constexpr int IPSDTA_MAX_K = 32;

struct FrameArgs {
  const c128 *X;       // (B, N, F, T)
  const c128 *W;       // (B, F, N, N)
  const c128 *basis;   // (B, N, K, Cn, L, L)
  const double *V;     // (B, N, K, T)
  const double *pi;    // (B, N, T) or null (weight 1)
  double *out0, *out1;
  int *route;          // null, or (B, N, Call, T): 1 where the matrix went through the repair
  int N, F, T, K, Cn, f0, c0, Call, mode;
};

// true when A (Hermitian, lower triangle read) is positive definite to working precision
template <int L>
__device__ __forceinline__ bool chol_pd(c128 (&A)[L][L]) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < L; ++c) {
    double d = A[c][c].x;
#pragma unroll
    for (int k = 0; k < c; ++k) d -= cabs2(A[c][k]);
    ok = ok && (d > 0.0);
    const double il = 1.0 / sqrt(d > 0.0 ? d : 1.0);
#pragma unroll
    for (int r = c + 1; r < L; ++r) {
      c128 s = A[r][c];
#pragma unroll
      for (int k = 0; k < c; ++k) cfms(s, A[r][k], cconj(A[c][k]));
      A[r][c] = cscale(s, il);
    }
  }
  return ok;
}

// to_psd with its default floor: eigenvalues below 1e-10 raised to it (ssspy/special/psd.py:11-71).
// Every lane of the wave must be in the call (the Jacobi sweeps end on a wave vote).
template <int L>
__device__ __noinline__ void psd_repair(c128 (&R)[L][L]) {
  if constexpr (L == 1) {
    R[0][0] = cmake(apply_floor(R[0][0].x, SSSPY_FLOOR_MAX, IPSDTA_PSD_EPS), 0.0);
  } else {
    c128 P[L][L];
    double lam[L];
    psd_eigen<L, (L > 4)>(R, P, lam, SSSPY_FLOOR_MAX, IPSDTA_PSD_EPS);
    herm_rebuild<L, (L > 4)>(P, lam, R);
  }
}

// packed Hermitian: element e = i * L + j holds Re M[i][j] for i >= j and Im M[j][i] for i < j
template <int L>
__device__ __forceinline__ double packed(const c128 (&M)[L][L], int i, int j) {
  return i >= j ? M[i][j].x : M[j][i].y;
}

enum { MODE_QUAD = 0, MODE_BASIS = 1, MODE_ACT = 2, MODE_COV = 3 };

template <int L>
__global__ __launch_bounds__(64) void k_ipsdta_frame(const FrameArgs g) {
  extern __shared__ double lds[];
  constexpr int E = L * L, E1 = E + 1;
  const int c = blockIdx.x, n = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x;
  const int N = g.N, F = g.F, T = g.T, K = g.K;
  const c128 *Tn = g.basis + ((size_t)(b * N + n) * K) * g.Cn * E;  // + (k * Cn + c) * E
  const double *Vn = g.V + (size_t)(b * N + n) * K * T;
  const int fb = g.f0 + c * L;
  const int cg = g.c0 + c;
  const double inv_T = 1.0 / (double)T;

  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    const bool live = t < T;
    const int tt = live ? t : T - 1;
    // y = W x for the block's bins (the covariance pass needs neither y nor u)
    const bool want_y = g.mode != MODE_COV;
    c128 y[L];
#pragma unroll
    for (int a = 0; a < L; ++a) {
      c128 s = cmake(0.0, 0.0);
      if (want_y) {
        const c128 *w = g.W + ((size_t)(b * F + fb + a) * N + n) * N;
        for (int m = 0; m < N; ++m) cfma(s, w[m], g.X[((size_t)(b * N + m) * F + fb + a) * T + tt]);
      }
      y[a] = s;
    }
    // R = sum_k v T_k, Hermitised
    c128 R[L][L];
#pragma unroll
    for (int i = 0; i < L; ++i)
#pragma unroll
      for (int j = 0; j < L; ++j) R[i][j] = cmake(0.0, 0.0);
    for (int k = 0; k < K; ++k) {
      const double v = Vn[(size_t)k * T + tt];
      const c128 *Tk = Tn + ((size_t)k * g.Cn + c) * E;
#pragma unroll
      for (int i = 0; i < L; ++i)
#pragma unroll
        for (int j = 0; j < L; ++j) {
          R[i][j].x = fma(v, Tk[i * L + j].x, R[i][j].x);
          R[i][j].y = fma(v, Tk[i * L + j].y, R[i][j].y);
        }
    }
    hermitize<L>(R);
    // the floor: proven idle by a Cholesky factorisation of R - eps I, else the Jacobi route
    bool pd;
    {
      c128 A[L][L];
#pragma unroll
      for (int i = 0; i < L; ++i)
#pragma unroll
        for (int j = 0; j < L; ++j) A[i][j] = R[i][j];
#pragma unroll
      for (int i = 0; i < L; ++i) A[i][i].x -= IPSDTA_PSD_EPS;
      pd = chol_pd<L>(A);
    }
    if (__any(!pd)) {
      c128 R2[L][L];
#pragma unroll
      for (int i = 0; i < L; ++i)
#pragma unroll
        for (int j = 0; j < L; ++j) R2[i][j] = R[i][j];
      psd_repair<L>(R2);
      if (!pd) {
#pragma unroll
        for (int i = 0; i < L; ++i)
#pragma unroll
          for (int j = 0; j < L; ++j) R[i][j] = R2[i][j];
        hermitize<L>(R);
      }
    }
    if (g.route != nullptr && live)
      g.route[((size_t)(b * N + n) * g.Call + cg) * T + t] = pd ? 0 : 1;
    c128 Inv[L][L];
    double logdet;
    chol_inverse<L>(R, Inv, logdet);  // (R is destroyed)
    c128 u[L];
    double quad = 0.0;
#pragma unroll
    for (int i = 0; i < L; ++i) {
      c128 s = cmake(0.0, 0.0);
      if (want_y) {
#pragma unroll
        for (int j = 0; j < L; ++j) cfma(s, Inv[i][j], y[j]);
      }
      u[i] = s;
      quad += y[i].x * s.x + y[i].y * s.y;  // Re(conj(y_i) u_i)
    }
    const double pw = g.pi != nullptr ? g.pi[(size_t)(b * N + n) * T + tt] : 1.0;

    if (g.mode == MODE_QUAD) {
      if (live) {
        const size_t o = ((size_t)(b * N + n) * g.Call + cg) * T + t;
        g.out0[o] = quad;
        g.out1[o] = logdet;
      }
    } else if (g.mode == MODE_ACT) {
      // num = pi Re(u^H T_k u), den = Re tr(R^-1 T_k)
      for (int k = 0; k < K; ++k) {
        const c128 *Tk = Tn + ((size_t)k * g.Cn + c) * E;
        double num = 0.0, den = 0.0;
#pragma unroll
        for (int i = 0; i < L; ++i) {
          c128 s = cmake(0.0, 0.0);
#pragma unroll
          for (int j = 0; j < L; ++j) {
            const c128 tij = Tk[i * L + j];
            cfma(s, tij, u[j]);
            den += Inv[j][i].x * tij.x - Inv[j][i].y * tij.y;  // Re(Inv_ji T_ij)
          }
          num += u[i].x * s.x + u[i].y * s.y;
        }
        if (live) {
          const size_t o = (((size_t)(b * N + n) * K + k) * g.Call + cg) * T + t;
          g.out0[o] = pw * num;
          g.out1[o] = den;
        }
      }
    } else if (g.mode == MODE_BASIS) {
      // SA[lane][e]: R^-1 packed, SB[lane][e]: pi u u^H packed, SV[k][lane]: v; zero past the end
      double *SA = lds, *SB = lds + 64 * E1, *SV = lds + 128 * E1;
      const double lw = live ? 1.0 : 0.0;
      __syncthreads();
#pragma unroll
      for (int i = 0; i < L; ++i)
#pragma unroll
        for (int j = 0; j < L; ++j) {
          SA[lane * E1 + i * L + j] = lw * packed<L>(Inv, i, j);
          // (u u^H)[i][j] = u_i conj(u_j): Re for i >= j, Im of [j][i] for i < j
          const c128 uu = i >= j ? cmulc(u[i], u[j]) : cmulc(u[j], u[i]);
          SB[lane * E1 + i * L + j] = lw * pw * (i >= j ? uu.x : uu.y);
        }
      for (int k = 0; k < K; ++k) SV[k * 64 + lane] = lw * Vn[(size_t)k * T + tt];
      __syncthreads();
      const bool last = t0 + 64 >= T;
      for (int o = lane; o < K * E; o += 64) {
        const int k = o / E, e = o - k * E;
        const int i = e / L, j = e - i * L;
        double sp = 0.0, sq = 0.0;
        for (int l = 0; l < 64; ++l) {
          const double v = SV[k * 64 + l];
          sp = fma(v, SA[l * E1 + e], sp);
          sq = fma(v, SB[l * E1 + e], sq);
        }
        // element (i >= j: Re of [i][j] and [j][i]; i < j: Im of [j][i], minus it of [i][j])
        double *P = g.out0 + 2 * ((((size_t)(b * N + n) * K + k) * g.Cn + c) * E);
        double *Q = g.out1 + 2 * ((((size_t)(b * N + n) * K + k) * g.Cn + c) * E);
        const int lo = 2 * (i >= j ? i * L + j : j * L + i) + (i >= j ? 0 : 1);
        if (t0 > 0) {
          sp += P[lo];
          sq += Q[lo];
        }
        if (last) {
          sp *= inv_T;
          sq *= inv_T;
        }
        P[lo] = sp;
        Q[lo] = sq;
        if (i > j) {
          P[2 * (j * L + i)] = sp;
          Q[2 * (j * L + i)] = sq;
        } else if (i < j) {
          P[2 * (i * L + j) + 1] = -sp;
          Q[2 * (i * L + j) + 1] = -sq;
        } else {
          P[lo + 1] = 0.0;
          Q[lo + 1] = 0.0;
        }
      }
    } else {  // MODE_COV
      // SA[lane][e]: pi R^-1 packed, SX[lane][m][a]: x of the block's bins
      const int XS = 2 * N * L + 1;
      double *SA = lds, *SX = lds + 64 * E1;
      const double lw = live ? pw : 0.0;
      __syncthreads();
#pragma unroll
      for (int i = 0; i < L; ++i)
#pragma unroll
        for (int j = 0; j < L; ++j) SA[lane * E1 + i * L + j] = lw * packed<L>(Inv, i, j);
      for (int m = 0; m < N; ++m)
#pragma unroll
        for (int a = 0; a < L; ++a) {
          const c128 x = g.X[((size_t)(b * N + m) * F + fb + a) * T + tt];
          SX[lane * XS + 2 * (m * L + a)] = x.x;
          SX[lane * XS + 2 * (m * L + a) + 1] = x.y;
        }
      __syncthreads();
      const bool last = t0 + 64 >= T;
      // out[b][c][a][bb][n][m1][m2] = mean_t pi R^-1[bb][a] x[m1][a] conj(x[m2][bb])
      c128 *out = reinterpret_cast<c128 *>(g.out0);
      for (int o = lane; o < E * N * N; o += 64) {
        const int m2 = o % N, m1 = (o / N) % N, e = o / (N * N);
        const int a = e / L, bb = e - a * L;
        const int ere = bb >= a ? bb * L + a : a * L + bb;  // Re R^-1[bb][a]
        const int eim = bb >= a ? a * L + bb : bb * L + a;  // |Im|; sign below
        const double sgn = bb > a ? 1.0 : (bb < a ? -1.0 : 0.0);
        c128 s = cmake(0.0, 0.0);
        for (int l = 0; l < 64; ++l) {
          const c128 r = cmake(SA[l * E1 + ere], sgn * SA[l * E1 + eim]);
          const c128 x1 = cmake(SX[l * XS + 2 * (m1 * L + a)], SX[l * XS + 2 * (m1 * L + a) + 1]);
          const c128 x2 = cmake(SX[l * XS + 2 * (m2 * L + bb)], SX[l * XS + 2 * (m2 * L + bb) + 1]);
          cfma(s, r, cmulc(x1, x2));
        }
        const size_t idx = ((((size_t)(b * g.Cn + c) * E + e) * N + n) * N + m1) * N + m2;
        if (t0 > 0) s = cadd(s, out[idx]);
        if (last) s = cscale(s, inv_T);
        out[idx] = s;
      }
    }
  }
}

template <int L>
int launch_frame(const FrameArgs &g, int B, hipStream_t st) {
  constexpr int E1 = L * L + 1;
  size_t lds = 0;
  if (g.mode == MODE_BASIS) lds = (size_t)(128 * E1 + 64 * g.K) * sizeof(double);
  if (g.mode == MODE_COV) lds = (size_t)(64 * E1 + 64 * (2 * g.N * L + 1)) * sizeof(double);
  if (lds > 65536) {  // (64 KiB is the default ceiling of a launch; the device has 160 KiB)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ipsdta_frame<L>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(SSSPY_ERR_HIP, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(k_ipsdta_frame<L>, dim3(g.Cn, g.N, B), dim3(64), lds, st, g);
  return check_launch("k_ipsdta_frame");
}

// pi (B, N, T) and the data term of the loss (B) from the quadratic forms and log-determinants
// (B, N, Call, T).  One workgroup per mixture: frames over the threads, sources and blocks in order.
__global__ __launch_bounds__(256) void k_ipsdta_weight_loss(const double *__restrict__ quad,
                                                            const double *__restrict__ logdet,
                                                            int N, int Call, int Clow, int T, int F,
                                                            int model, double dof, double *pi,
                                                            double *loss) {
  __shared__ double scratch[4];
  const int b = blockIdx.x;
  double acc = 0.0;
  for (int t = threadIdx.x; t < T; t += 256) {
    double term = 0.0, qlow = 0.0, qhigh = 0.0;
    for (int n = 0; n < N; ++n) {
      const double *q = quad + ((size_t)(b * N + n) * Call) * T + t;
      const double *ld = logdet + ((size_t)(b * N + n) * Call) * T + t;
      double s = 0.0, sl = 0.0;
      for (int c = 0; c < Call; ++c) {
        const double qc = q[(size_t)c * T];
        if (model == SSSPY_SOURCE_T) s += qc < 0.0 ? 0.0 : qc;  // (NaN propagates, as np.maximum)
        else if (c < Clow) qlow += qc;
        else qhigh += qc;
        sl += ld[(size_t)c * T];
      }
      if (model == SSSPY_SOURCE_T) {
        if (pi != nullptr) pi[(size_t)(b * N + n) * T + t] = (dof + 2.0 * F) / (dof + 2.0 * s);
        term += 0.5 * (dof + 2.0 * F) * log(1.0 + (2.0 / dof) * s);
      }
      term += sl;
    }
    if (model != SSSPY_SOURCE_T) {
      term += qlow < 0.0 ? 0.0 : qlow;
      if (Clow < Call) term += qhigh < 0.0 ? 0.0 : qhigh;
    }
    acc += term;
  }
  const double total = block_sum(acc, scratch);
  if (threadIdx.x == 0 && loss != nullptr) loss[b] = total / (double)T;
}

// V <- V sqrt(num / den), num and den summed over the blocks in order
__global__ __launch_bounds__(256) void k_ipsdta_activation(double *V, const double *__restrict__ num,
                                                           const double *__restrict__ den,
                                                           long long rows, int Call, int T) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * T) return;
  const long long r = i / T;
  const int t = (int)(i - r * T);
  double sn = 0.0, sd = 0.0;
  for (int c = 0; c < Call; ++c) {
    sn += num[((size_t)r * Call + c) * T + t];
    sd += den[((size_t)r * Call + c) * T + t];
  }
  V[i] *= sqrt(sn / sd);
}

// trace normalisation of (T, V) per (mixture, source, basis), traces summed across both partitions
__global__ __launch_bounds__(256) void k_ipsdta_normalize(c128 *Tlow, c128 *Thigh, double *V,
                                                          int Clow, int Llow, int Chigh, int Lhigh,
                                                          int T) {
  __shared__ double scratch[4];
  __shared__ double tr;
  const size_t r = blockIdx.x;
  c128 *lo = Tlow + r * Clow * Llow * Llow;
  c128 *hi = Chigh > 0 ? Thigh + r * Chigh * Lhigh * Lhigh : nullptr;
  double acc = 0.0;
  for (int i = threadIdx.x; i < Clow * Llow; i += 256)
    acc += lo[(size_t)(i / Llow) * Llow * Llow + (i % Llow) * (Llow + 1)].x;
  const double slow = block_sum(acc, scratch);
  acc = 0.0;
  for (int i = threadIdx.x; i < Chigh * Lhigh; i += 256)
    acc += hi[(size_t)(i / Lhigh) * Lhigh * Lhigh + (i % Lhigh) * (Lhigh + 1)].x;
  const double shigh = block_sum(acc, scratch);
  if (threadIdx.x == 0) tr = slow + shigh;
  __syncthreads();
  const double trace = tr;
  for (int i = threadIdx.x; i < Clow * Llow * Llow; i += 256)
    lo[i] = cmake(lo[i].x / trace, lo[i].y / trace);
  for (int i = threadIdx.x; i < Chigh * Lhigh * Lhigh; i += 256)
    hi[i] = cmake(hi[i].x / trace, hi[i].y / trace);
  for (int t = threadIdx.x; t < T; t += 256) V[r * T + t] *= trace;
}

// The VCD sweep (ssspy/bss/_update_spatial_model.py:565-606): a lane per (mixture, block); the L x N
// row updates of a block are sequential, gamma reads the current rows of the block's other bins.
// W (B, F, N, N), block c of the launch covers bins f0 + c L .. + L; RXX (B, Cn, L, L, N, N, N).
template <int N>
__global__ __launch_bounds__(64) void k_ipsdta_vcd(c128 *W, const c128 *__restrict__ RXX, int B,
                                                   int F, int Cn, int L, int f0, double threshold,
                                                   int *info) {
  const int item = blockIdx.x * 64 + threadIdx.x;
  if (item >= B * Cn) return;
  const int b = item / Cn, c = item - b * Cn;
  c128 *Wb = W + ((size_t)b * F + f0 + (size_t)c * L) * N * N;  // [l][n][m]
  const c128 *Rc = RXX + (size_t)item * L * L * N * N * N;      // [a][bb][n][m1][m2]
  int singular = 0;
  for (int i = 0; i < L; ++i) {
#pragma unroll 1
    for (int n = 0; n < N; ++n) {
      Mat<N> U;
      load_mat<N>(U, Rc + (((size_t)i * L + i) * N + n) * N * N);
      // gamma = sum_{l != i} RXX[i][l][n] conj(w_ln)
      c128 rhs[N][1];
#pragma unroll
      for (int m = 0; m < N; ++m) rhs[m][0] = cmake(0.0, 0.0);
      for (int l = 0; l < L; ++l) {
        if (l == i) continue;
        const c128 *Ril = Rc + (((size_t)i * L + l) * N + n) * N * N;
        const c128 *wl = Wb + ((size_t)l * N + n) * N;
#pragma unroll
        for (int m1 = 0; m1 < N; ++m1) {
          c128 s = cmake(0.0, 0.0);
#pragma unroll
          for (int m2 = 0; m2 < N; ++m2) cfma(s, Ril[m1 * N + m2], cconj(wl[m2]));
          rhs[m1][0] = cadd(rhs[m1][0], s);
        }
      }
      // eta = (W_i U)^-1 e_n, eta_hat = U^-1 gamma
      Mat<N> Wi, WU;
      load_mat<N>(Wi, Wb + (size_t)i * N * N);
      matmul<N>(WU, Wi, U);
      c128 eta[N];
      bool ok = solve_unit<N>(WU, n, eta);
      Mat<N> U2 = U;
      ok = lu_forward<N, 1>(U2, rhs) && ok;
      lu_backward<N, 1>(U2, rhs);
      singular += ok ? 0 : 1;
      // xi = Re(eta^H U eta) floored at 0, xi_hat = eta^H U eta_hat
      double xi = 0.0;
      c128 xih = cmake(0.0, 0.0);
#pragma unroll
      for (int m = 0; m < N; ++m) {
        c128 eu = cmake(0.0, 0.0);
#pragma unroll
        for (int a = 0; a < N; ++a) cfma(eu, cconj(eta[a]), U.a[a][m]);
        const c128 p = cmul(eu, eta[m]);
        xi += p.x;
        cfma(xih, eu, rhs[m][0]);
      }
      xi = xi < 0.0 ? 0.0 : xi;
      const bool sing = hypot(xih.x, xih.y) < threshold;
      if (sing) xih = cmake(1.0, 0.0);
      const double mag = hypot(xih.x, xih.y);
      const double f = (1.0 - sqrt(1.0 + 4.0 * xi / (mag * mag))) / (2.0 * xi);
      c128 coeff = cscale(xih, f);
      if (sing) coeff = cmake(1.0 / sqrt(xi), 0.0);
      c128 *wn = Wb + ((size_t)i * N + n) * N;
#pragma unroll
      for (int m = 0; m < N; ++m) wn[m] = cconj(csub(cmul(coeff, eta[m]), rhs[m][0]));
    }
  }
  if (singular && info != nullptr) atomicAdd(info, singular);
}

// out = (A B) C for n matrices of size L x L, a lane per matrix.  Row r of A B goes through out
// itself (the lane's own stores, read back into L registers), and the column loops are rolled: the
// live set is one row and one dot product whatever L is.
template <int L>
__global__ __launch_bounds__(64) void k_matmul3(const c128 *__restrict__ A, const c128 *__restrict__ Bm,
                                                const c128 *__restrict__ C, c128 *out, long long n) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  A += i * L * L;
  Bm += i * L * L;
  C += i * L * L;
  out += i * L * L;
#pragma unroll 1
  for (int r = 0; r < L; ++r) {
#pragma unroll 1
    for (int j = 0; j < L; ++j) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < L; ++k) cfma(s, A[r * L + k], Bm[k * L + j]);
      out[r * L + j] = s;
    }
    c128 row[L];
#pragma unroll
    for (int k = 0; k < L; ++k) row[k] = out[r * L + k];
#pragma unroll 1
    for (int j = 0; j < L; ++j) {
      c128 s = cmake(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < L; ++k) cfma(s, row[k], C[k * L + j]);
      out[r * L + j] = s;
    }
  }
}

// R[s, t, c] = to_psd(sum_k v[s, k, t] T[s, k, c]) handed out: (S, T, Cn, L, L), a lane per matrix
// (c fastest).  The sum over k stays in the lane, in the order of k; then the per-lane Hermitian
// to_psd (hermitian.hpp) at every matrix -- no Cholesky shortcut: what leaves is what the floor made.
// basis_last == 0: basis (S, K, Cn, L, L); != 0: (S, Cn, L, L, K), the reference's other layout.
// A lane past the end works on the last matrix and stores nothing (the Jacobi sweeps end on a wave
// vote).  D: Fixed<L> to 4 x 4, Fixed<L, true> to 8 x 8, Runtime above (the full-matrix PSDTF).
template <class D>
__global__ __launch_bounds__(64) void k_psdtf_reconstruct(D d, const c128 *__restrict__ basis,
                                                          const double *__restrict__ V, c128 *out,
                                                          long long n, int K, int T, int Cn,
                                                          int basis_last, int floor_kind,
                                                          double eps) {
  constexpr int CC = D::cap * D::cap;
  const int L = d.n(), E = L * L;
  const long long lane = (long long)blockIdx.x * 64 + threadIdx.x;
  const bool live = lane < n;
  const long long idx = live ? lane : n - 1;
  const int c = (int)(idx % Cn);
  const int t = (int)((idx / Cn) % T);
  const long long s = idx / ((long long)Cn * T);
  const double *v = V + s * K * T + t;  // + k * T
  // element e of T_k: basis_last == 0 at Tb[k * k_stride + e], else at Tb[e * K + k]
  const c128 *Tb = basis_last ? basis + (s * Cn + c) * E * K : basis + (s * K * Cn + c) * E;
  const long long k_stride = basis_last ? 1 : (long long)Cn * E;
  const long long e_stride = basis_last ? K : 1;
  c128 R[CC], P[CC];
  double lam[D::cap];
#pragma unroll D::unroll
  for (int e = 0; e < E; ++e) R[e] = cmake(0.0, 0.0);
  for (int k = 0; k < K; ++k) {
    const double vk = v[(long long)k * T];
#pragma unroll D::unroll
    for (int e = 0; e < E; ++e) {
      const c128 z = Tb[k * k_stride + e * e_stride];
      R[e].x = fma(vk, z.x, R[e].x);
      R[e].y = fma(vk, z.y, R[e].y);
    }
  }
  psd_eigen(d, R, P, lam, floor_kind, eps);
  rebuild(d, P, lam, R);
  if (!live) return;
#pragma unroll D::unroll
  for (int e = 0; e < E; ++e) out[idx * E + e] = R[e];
}

int check_sizes(int N, int L, int K) {
  if (N < 2 || N > 8) return fail(SSSPY_ERR_UNSUPPORTED, "IPSDTA takes 2 to 8 sources");
  if (L < 1 || L > IPSDTA_MAX_L)
    return fail(SSSPY_ERR_UNSUPPORTED, "IPSDTA takes block sizes 1 to 8");
  if (K < 1 || K > IPSDTA_MAX_K) return fail(SSSPY_ERR_UNSUPPORTED, "IPSDTA takes 1 to 32 bases");
  return SSSPY_OK;
}

}  // namespace

}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_ipsdta_frame_pass(const void *X, const void *W, const void *basis, const double *activation,
                            const double *pi, int B, int N, int F, int T, int K, int n_part_blocks,
                            int L, int first_bin, int first_block, int n_blocks, int mode,
                            void *out0, void *out1, int *route, void *stream) {
  SSSPY_REQUIRE(X && W && basis && activation && out0, "ipsdta_frame_pass: null pointer");
  SSSPY_REQUIRE(B > 0 && F > 0 && T > 0 && n_part_blocks > 0, "ipsdta_frame_pass: empty problem");
  SSSPY_REQUIRE(mode >= MODE_QUAD && mode <= MODE_COV, "ipsdta_frame_pass: mode must be 0..3");
  SSSPY_REQUIRE(mode == MODE_COV || out1 != nullptr, "ipsdta_frame_pass: out1 is null");
  SSSPY_REQUIRE(first_bin >= 0 && (long long)first_bin + (long long)n_part_blocks * L <= F,
                "ipsdta_frame_pass: the blocks leave the bins");
  SSSPY_REQUIRE(first_block >= 0 && first_block + n_part_blocks <= n_blocks,
                "ipsdta_frame_pass: the blocks leave n_blocks");
  SSSPY_REQUIRE(B <= 65535 && N <= 65535, "ipsdta_frame_pass: grid too large");
  if (int rc = check_sizes(N, L, K)) return rc;
  FrameArgs g;
  g.X = (const c128 *)X;
  g.W = (const c128 *)W;
  g.basis = (const c128 *)basis;
  g.V = activation;
  g.pi = pi;
  g.out0 = (double *)out0;
  g.out1 = (double *)out1;
  g.route = route;
  g.N = N; g.F = F; g.T = T; g.K = K;
  g.Cn = n_part_blocks; g.f0 = first_bin; g.c0 = first_block; g.Call = n_blocks; g.mode = mode;
  DISPATCH_N(L, return launch_frame<NN>(g, B, as_stream(stream)));
  return SSSPY_OK;
}

int ssspy_ipsdta_weight_loss(const double *quad, const double *logdet, int B, int N, int n_blocks,
                             int n_low_blocks, int T, int F, int model, double dof, double *pi,
                             double *loss, void *stream) {
  SSSPY_REQUIRE(quad && logdet, "ipsdta_weight_loss: null pointer");
  SSSPY_REQUIRE(B > 0 && N > 0 && n_blocks > 0 && T > 0, "ipsdta_weight_loss: empty problem");
  SSSPY_REQUIRE(n_low_blocks >= 0 && n_low_blocks <= n_blocks, "ipsdta_weight_loss: n_low_blocks");
  SSSPY_REQUIRE(model == SSSPY_SOURCE_GAUSS || model == SSSPY_SOURCE_T,
                "ipsdta_weight_loss: model must be Gauss or t");
  hipLaunchKernelGGL(k_ipsdta_weight_loss, dim3(B), dim3(256), 0, as_stream(stream), quad, logdet, N,
                     n_blocks, n_low_blocks, T, F, model, dof, pi, loss);
  return check_launch("k_ipsdta_weight_loss");
}

int ssspy_ipsdta_activation(double *activation, const double *num, const double *den, int B, int N,
                            int K, int n_blocks, int T, void *stream) {
  SSSPY_REQUIRE(activation && num && den, "ipsdta_activation: null pointer");
  SSSPY_REQUIRE(B > 0 && N > 0 && K > 0 && n_blocks > 0 && T > 0, "ipsdta_activation: empty problem");
  const long long rows = (long long)B * N * K;
  const long long blocks = (rows * T + 255) / 256;
  SSSPY_REQUIRE(blocks < 2147483647LL, "ipsdta_activation: grid too large");
  hipLaunchKernelGGL(k_ipsdta_activation, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                     activation, num, den, rows, n_blocks, T);
  return check_launch("k_ipsdta_activation");
}

int ssspy_ipsdta_normalize(void *basis_low, void *basis_high, double *activation, int B, int N, int K,
                           int n_low_blocks, int L_low, int n_high_blocks, int L_high, int T,
                           void *stream) {
  SSSPY_REQUIRE(basis_low && activation, "ipsdta_normalize: null pointer");
  SSSPY_REQUIRE(n_high_blocks == 0 || basis_high, "ipsdta_normalize: basis_high is null");
  SSSPY_REQUIRE(B > 0 && N > 0 && K > 0 && n_low_blocks > 0 && L_low > 0 && T > 0 &&
                    n_high_blocks >= 0 && (n_high_blocks == 0 || L_high > 0),
                "ipsdta_normalize: empty problem");
  hipLaunchKernelGGL(k_ipsdta_normalize, dim3((unsigned)(B * N * K)), dim3(256), 0, as_stream(stream),
                     (c128 *)basis_low, (c128 *)basis_high, activation, n_low_blocks, L_low,
                     n_high_blocks, L_high, T);
  return check_launch("k_ipsdta_normalize");
}

int ssspy_ipsdta_vcd(void *W, const void *weighted_covariance, int B, int F, int N, int n_part_blocks,
                     int L, int first_bin, double threshold, int *info, void *stream) {
  SSSPY_REQUIRE(W && weighted_covariance, "ipsdta_vcd: null pointer");
  SSSPY_REQUIRE(B > 0 && n_part_blocks > 0 && L > 0, "ipsdta_vcd: empty problem");
  SSSPY_REQUIRE(first_bin >= 0 && (long long)first_bin + (long long)n_part_blocks * L <= F,
                "ipsdta_vcd: the blocks leave the bins");
  if (N < 2 || N > 8) return fail(SSSPY_ERR_UNSUPPORTED, "the VCD sweep takes 2 to 8 sources");
  const long long items = (long long)B * n_part_blocks;
  SSSPY_REQUIRE(items < 2147483647LL, "ipsdta_vcd: too many blocks");
  const unsigned grid = (unsigned)((items + 63) / 64);
  DISPATCH_N(N, hipLaunchKernelGGL(k_ipsdta_vcd<NN>, dim3(grid), dim3(64), 0, as_stream(stream),
                                   (c128 *)W, (const c128 *)weighted_covariance, B, F,
                                   n_part_blocks, L, first_bin, threshold, info));
  return check_launch("k_ipsdta_vcd");
}

int ssspy_ipsdta_reconstruct(const void *basis, const double *activation, void *out, long long S,
                             int K, int T, int n_part_blocks, int L, int basis_last, int floor_kind,
                             double floor_eps, void *stream) {
  SSSPY_REQUIRE(basis && activation && out, "ipsdta_reconstruct: null pointer");
  SSSPY_REQUIRE(S > 0 && T > 0 && n_part_blocks > 0, "ipsdta_reconstruct: empty problem");
  SSSPY_REQUIRE(floor_kind >= SSSPY_FLOOR_NONE && floor_kind <= SSSPY_FLOOR_ADD,
                "ipsdta_reconstruct: unknown floor");
  if (L < 1 || L > SSSPY_RT_MAX_SOURCES)
    return fail(SSSPY_ERR_UNSUPPORTED, "ipsdta_reconstruct takes matrices of 1 x 1 to 16 x 16");
  if (K < 1 || K > IPSDTA_MAX_K)
    return fail(SSSPY_ERR_UNSUPPORTED, "ipsdta_reconstruct takes 1 to 32 bases");
  SSSPY_REQUIRE(S <= (1LL << 36) / T / n_part_blocks, "ipsdta_reconstruct: too many matrices");
  const long long n = S * T * n_part_blocks;
  const dim3 grid((unsigned)((n + 63) / 64)), block(64);
  const hipStream_t st = as_stream(stream);
#define SSSPY_RECONSTRUCT(DESC, VALUE)                                                          \
  hipLaunchKernelGGL((k_psdtf_reconstruct<DESC>), grid, block, 0, st, VALUE, (const c128 *)basis, \
                     activation, (c128 *)out, n, K, T, n_part_blocks, basis_last ? 1 : 0,      \
                     floor_kind, floor_eps)
  using Rolled5 = Fixed<5, true>;
  using Rolled6 = Fixed<6, true>;
  using Rolled7 = Fixed<7, true>;
  using Rolled8 = Fixed<8, true>;
  switch (L) {
    case 1: SSSPY_RECONSTRUCT(Fixed<1>, Fixed<1>{}); break;
    case 2: SSSPY_RECONSTRUCT(Fixed<2>, Fixed<2>{}); break;
    case 3: SSSPY_RECONSTRUCT(Fixed<3>, Fixed<3>{}); break;
    case 4: SSSPY_RECONSTRUCT(Fixed<4>, Fixed<4>{}); break;
    case 5: SSSPY_RECONSTRUCT(Rolled5, Rolled5{}); break;
    case 6: SSSPY_RECONSTRUCT(Rolled6, Rolled6{}); break;
    case 7: SSSPY_RECONSTRUCT(Rolled7, Rolled7{}); break;
    case 8: SSSPY_RECONSTRUCT(Rolled8, Rolled8{}); break;
    default: SSSPY_RECONSTRUCT(Runtime, Runtime{L}); break;
  }
#undef SSSPY_RECONSTRUCT
  return check_launch("k_psdtf_reconstruct");
}

int ssspy_matmul3(const void *A, const void *Bm, const void *C, void *out, long long n, int L,
                  void *stream) {
  SSSPY_REQUIRE(A && Bm && C && out, "matmul3: null pointer");
  SSSPY_REQUIRE(n > 0 && n < 64LL * 2147483647LL, "matmul3: n out of range");
  SSSPY_REQUIRE(out != A && out != Bm && out != C, "matmul3: out must not alias an operand");
  if (L < 1 || L > IPSDTA_MAX_L) return fail(SSSPY_ERR_UNSUPPORTED, "matmul3 takes sizes 1 to 8");
  const unsigned grid = (unsigned)((n + 63) / 64);
  DISPATCH_N(L, hipLaunchKernelGGL(k_matmul3<NN>, dim3(grid), dim3(64), 0, as_stream(stream),
                                   (const c128 *)A, (const c128 *)Bm, (const c128 *)C, (c128 *)out,
                                   n));
  return check_launch("k_matmul3");
}

}  // extern "C"
