// What the spectrogram-sized passes of the proximal separators share (pdsbss.hip, admmbss.hip,
// hva.hip): the contraction R_i = d_i X_i^H per bin with the family's operand, Z = dual_q + W2 x of one
// (bin, frame) and ADMMBSS's Z = relax W x + (1 - relax) auxiliary2_q + dual2_q of it, the HVA mask of
// one (bin, frame), the shrinkage factor, the chunks of the norm pass over bins, the source-count
// dispatches and the argument check of the entry points.  The norm pass and the point step stay in the
// units: cut into shared templates or helpers they need more registers than the kernels they would
// replace ("PDSBSS").
// fp64 / complex128, no atomics, every sum in a fixed order: two runs give the same bits.
#pragma once

#include "common.hpp"

#include <cstdio>

namespace ssspy {

constexpr int PROX_THREADS = 256;
constexpr int PROX_MAX_CHUNKS = FOLD_GROUP;  // (one level of k_fold_slabs: no scratch)
// a `kind` of the point steps (k_pds_dual_step, k_admm_aux_step) past the public SSSPY_PROX_* ones:
// Z to zout, the state untouched (the form_z entry points; the step entry points refuse it)
constexpr int PROX_KIND_FORM_Z = SSSPY_PROX_GIVEN + 1;

// z_n = d_n + sum_m W2[n][m] x_m for the N rows of one (bin, frame); Wn: row-major N x N
template <int G, typename WPtr>
__device__ __forceinline__ void pds_form_z(c128 (&z)[G], const c128 *__restrict__ Xb,
                                           const c128 *Db, WPtr Wn, int N, long long FT, int j) {
  c128 x[G];
#pragma unroll
  for (int m = 0; m < G; ++m) x[m] = m < N ? Xb[m * FT + j] : cmake(0.0, 0.0);
#pragma unroll
  for (int n = 0; n < G; ++n) {
    z[n] = cmake(0.0, 0.0);
    if (n < N) {
      c128 y = cmake(0.0, 0.0);
#pragma unroll
      for (int m = 0; m < G; ++m)
        if (m < N) cfma(y, Wn[n * N + m], x[m]);
      z[n] = cadd(Db[n * FT + j], y);
    }
  }
}

// z_n = relax (W x)_n + (1 - relax) a_n + d_n for the N rows of one (bin, frame); Wn: row-major N x N.
// mix == false (relaxation 1): a is not read, z_n = (W x)_n + d_n.
template <int G, typename WPtr>
__device__ __forceinline__ void admm_form_z(c128 (&z)[G], const c128 *__restrict__ Xb, const c128 *Ab,
                                            const c128 *Db, WPtr Wn, int N, long long FT, int j,
                                            double relax, bool mix) {
  c128 x[G];
#pragma unroll
  for (int m = 0; m < G; ++m) x[m] = m < N ? Xb[m * FT + j] : cmake(0.0, 0.0);
  const double om = 1.0 - relax;
#pragma unroll
  for (int n = 0; n < G; ++n) {
    z[n] = cmake(0.0, 0.0);
    if (n < N) {
      c128 y = cmake(0.0, 0.0);
#pragma unroll
      for (int m = 0; m < G; ++m)
        if (m < N) cfma(y, Wn[n * N + m], x[m]);
      if (mix) {
        const c128 a = Ab[n * FT + j];
        y = cmake(relax * y.x + om * a.x, relax * y.y + om * a.y);
      }
      z[n] = cadd(y, Db[n * FT + j]);
    }
  }
}

// the HVA mask of the N sources of one (bin, frame) from varrho (row n at Vb + n FT): the softmax of
// 2 varrho over sources with the maximum subtracted, to the power gamma,
// mask_n = exp(2 gamma (varrho_n - max)) / (sum_n' exp(2 (varrho_n' - max)))^gamma
// (ref: ssspy/bss/hva.py:112-115, :232-234).  A NaN in any source's varrho makes every mask NaN.
template <int G>
__device__ __forceinline__ void hva_mask(double (&mask)[G], const double *__restrict__ Vb, int N,
                                         long long FT, int j, double gamma) {
  double vr[G];
  double mx = -HUGE_VAL;
#pragma unroll
  for (int n = 0; n < G; ++n) {
    vr[n] = n < N ? Vb[n * FT + j] : 0.0;
    if (n < N) mx = fmax(mx, vr[n]);  // (a NaN is skipped here and poisons the sum below)
  }
  double sum = 0.0;
#pragma unroll
  for (int n = 0; n < G; ++n)
    if (n < N) sum += exp(2.0 * (vr[n] - mx));
  const double den = pow(sum, gamma);
#pragma unroll
  for (int n = 0; n < G; ++n) mask[n] = n < N ? exp(2.0 * gamma * (vr[n] - mx)) / den : 0.0;
}

// ---- R[b,i,n,m] = sum_j d[b,n,i,j] conj(X[b,m,i,j]); the operand d = op.at(off, j, Q, N FT) with off
// the start of row n of bin i in the first penalty's slice.  grid (F, B), 256 threads.
// G: the source count rounded up to a power of two.  Thread (n, jl) = (tid / FL, tid % FL), FL = 256 / G,
// walks frames jl, jl + FL, ... of row n with N accumulators; the frame lanes of a row are added by a
// butterfly inside a wave and over the waves of a row in wave order.
template <int G, typename Operand>
static __global__ __launch_bounds__(PROX_THREADS) void k_prox_contract(Operand op,
                                                                       const c128 *__restrict__ X,
                                                                       c128 *R, int Q, int N, int F,
                                                                       int T) {
  constexpr int FL = PROX_THREADS / G;
  constexpr int S = FL < 64 ? FL : 64;        // frame lanes of a row inside one wave
  constexpr int WPR = FL > 64 ? FL / 64 : 1;  // waves per row
  __shared__ c128 Ps[G * WPR * G];
  const int tid = threadIdx.x, n = tid / FL, jl = tid % FL;
  const int i = blockIdx.x, b = blockIdx.y;
  const bool src = n < N;
  const long long FT = (long long)F * T;
  const c128 *__restrict__ Xb = X + ((long long)b * N * F + i) * T;  // row m at Xb + m FT
  const long long off = (long long)b * Q * N * FT + ((long long)(src ? n : 0) * F + i) * T;
  c128 acc[G];
#pragma unroll
  for (int m = 0; m < G; ++m) acc[m] = cmake(0.0, 0.0);
  if (src) {
    for (int j = jl; j < T; j += FL) {
      const c128 d = op.at(off, j, Q, N * FT);
#pragma unroll
      for (int m = 0; m < G; ++m)
        if (m < N) {
          const c128 x = Xb[m * FT + j];
          // acc += d conj(x)
          acc[m].x = fma(d.x, x.x, acc[m].x);
          acc[m].x = fma(d.y, x.y, acc[m].x);
          acc[m].y = fma(d.y, x.x, acc[m].y);
          acc[m].y = fma(-d.x, x.y, acc[m].y);
        }
    }
  }
#pragma unroll
  for (int o = S / 2; o > 0; o >>= 1) {
#pragma unroll
    for (int m = 0; m < G; ++m) {
      acc[m].x += __shfl_xor(acc[m].x, o, 64);
      acc[m].y += __shfl_xor(acc[m].y, o, 64);
    }
  }
  if (jl % 64 == 0) {
    const int w = jl / 64;
#pragma unroll
    for (int m = 0; m < G; ++m) Ps[(n * WPR + w) * G + m] = acc[m];
  }
  __syncthreads();
  if (tid < N * N) {
    const int r = tid / N, m = tid % N;
    c128 s = Ps[(r * WPR) * G + m];
#pragma unroll
    for (int w = 1; w < WPR; ++w) s = cadd(s, Ps[(r * WPR + w) * G + m]);
    R[(((long long)b * F + i) * N + r) * N + m] = s;
  }
}

// bins per chunk and chunks of the l21-over-bins norm pass
static inline void prox_chunks(int F, int &FC, int &C) {
  const int want = F < PROX_MAX_CHUNKS ? F : PROX_MAX_CHUNKS;
  FC = (F + want - 1) / want;
  C = (F + FC - 1) / FC;
}

// max(1 - step / max(norm, step), 0): the factor of l1 / l21 (ref: ssspy/linalg/prox.py:6-33)
__device__ __forceinline__ double prox_shrink(double norm, double step) {
  norm = norm < step ? step : norm;
  const double s = 1.0 - step / norm;
  return s < 0.0 ? 0.0 : s;  // (NaN propagates, as through np.maximum)
}

static inline int pow2_group(int N) { return N <= 2 ? 2 : (N <= 4 ? 4 : (N <= 8 ? 8 : 16)); }

// `CALL` with GG = the source count rounded up to a power of two
#define SSSPY_PROX_DISPATCH_G(N_, CALL)              \
  switch (::ssspy::pow2_group(N_)) {                 \
    case 2: { constexpr int GG = 2; CALL; } break;   \
    case 4: { constexpr int GG = 4; CALL; } break;   \
    case 8: { constexpr int GG = 8; CALL; } break;   \
    default: { constexpr int GG = 16; CALL; } break; \
  }

// `CALL` with NN = the size at compile time (1..8) or 0 (9..16, the size at run time)
#define SSSPY_DISPATCH_N(N_, CALL)                  \
  switch (N_) {                                     \
    case 1: { constexpr int NN = 1; CALL; } break;  \
    case 2: { constexpr int NN = 2; CALL; } break;  \
    case 3: { constexpr int NN = 3; CALL; } break;  \
    case 4: { constexpr int NN = 4; CALL; } break;  \
    case 5: { constexpr int NN = 5; CALL; } break;  \
    case 6: { constexpr int NN = 6; CALL; } break;  \
    case 7: { constexpr int NN = 7; CALL; } break;  \
    case 8: { constexpr int NN = 8; CALL; } break;  \
    default: { constexpr int NN = 0; CALL; } break; \
  }

static inline bool prox_shape_ok(int B, int N, int F, int T) {
  return B > 0 && B <= 65535 && N >= 1 && N <= SSSPY_RT_MAX_SOURCES && F > 0 && T > 0;
}

// the batch stride of an entry point's state and what its messages call it ("dual" / "batch");
// {}: densely packed arguments, no stride to check
struct ProxStride {
  const char *word = nullptr;
  long long value = 0;
};

// the kind of a point step with what it may need: r2 for l21 over bins, the (B,N,F,T) array of
// MASK / GIVEN and the entry point's name of it; {}: an entry point without a kind
struct ProxKind {
  const char *given_word = nullptr;
  int kind = 0;
  const void *r2 = nullptr, *given = nullptr;
};

// ---- the argument check of a spectrogram-sized entry point `name`, in the order the entry points
// report: the pointers (`present`: they, and what else the entry point requires, hold), the kind with
// what it needs, the shape, the batch stride.
static inline int prox_check_args(const char *name, bool present, int B, int N, int F, int T,
                                  ProxStride stride = {}, ProxKind k = {}) {
  char msg[128];
  int code = SSSPY_ERR_BADARG;
  if (!(present && B > 0 && F > 0 && T > 0)) {
    std::snprintf(msg, sizeof(msg), "%s: bad argument", name);
  } else if (k.given_word && !(k.kind >= SSSPY_PROX_L1 && k.kind <= SSSPY_PROX_GIVEN)) {
    std::snprintf(msg, sizeof(msg), "%s: bad kind", name);
  } else if (k.given_word && k.kind == SSSPY_PROX_L21_BINS && !k.r2) {
    std::snprintf(msg, sizeof(msg), "%s: l21 over bins needs r2", name);
  } else if (k.given_word && (k.kind == SSSPY_PROX_MASK || k.kind == SSSPY_PROX_GIVEN) && !k.given) {
    std::snprintf(msg, sizeof(msg), "%s: this kind needs %s", name, k.given_word);
  } else if (!prox_shape_ok(B, N, F, T)) {
    code = SSSPY_ERR_UNSUPPORTED;
    std::snprintf(msg, sizeof(msg), "%s: 1..16 sources, up to 65535 mixtures", name);
  } else if (stride.word && stride.value < (long long)N * F * T) {
    std::snprintf(msg, sizeof(msg), "%s: bad %s stride", name, stride.word);
  } else {
    return SSSPY_OK;
  }
  return fail(code, msg);
}

}  // namespace ssspy
