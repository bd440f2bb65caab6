// Permutation alignment between frequency bins on gfx950 (fp64): the correlation solver of Murata
// et al. and the score solver of Sawada et al. with the decisions of the host solvers of
// ssspy_amd/algorithm/permutation_alignment.py -- the same permutation per bin, the same tie rule.
//
// Sequences are read where they lie: element (b, n, f, t) of a sequence is at
// b * stride_b + n * stride_n + f * stride_f + t (frames contiguous), which covers the library's
// (B, N, F, T) and the public functions' (B, F, N, T) without a transposed copy.  The workspaces of
// the solvers (envelopes, normalised sequences) are (B, F, N, T): the N rows of a bin are adjacent.
// The result is perm (B, F, N) int32: aligned component n of bin f is original component
// perm[b, f, n].
//
// Every sum runs in a fixed order (a thread's frames in increasing order, the lanes of a wave by a
// butterfly, the waves in wave order, bins in bin order); there are no fp64 atomics and no workgroup
// waits on another.  What is sequential -- the visiting order of the correlation solver, the bin
// walk of the score solver's local stage -- lives inside the one workgroup of a mixture.
#include "common.hpp"

#include <climits>

namespace ssspy {
namespace {

constexpr int PA_BIN_THREADS = 256;    // kernels with one workgroup per (mixture, bin)
constexpr int PA_SWEEP_THREADS = 512;  // kernels with one workgroup per mixture
constexpr int PA_MAX_WAVES = PA_SWEEP_THREADS / 64;
constexpr int PA_MAX_NEIGHBOURS = 13;  // 6 around f, 3 around f / 2, 3 around 2 f (+1: never reached)
// the criterion of the correlation sweep (N x T doubles) stays in LDS: 128 KB of the CU's 160 KB
constexpr int PA_MAX_CRITERION = 16384;

__host__ __device__ constexpr int pa_factorial(int n) { return n <= 1 ? 1 : n * pa_factorial(n - 1); }

// ---------------------------------------------------------------- block helpers
// sum over the block in a fixed order, in every thread.  scratch: PA_MAX_WAVES doubles of LDS.
__device__ __forceinline__ double pa_block_sum(double v, double *scratch) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // (the scratch of an earlier sum has been read)
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  const int nw = (blockDim.x + 63) >> 6;
  double total = 0.0;
  for (int w = 0; w < nw; ++w) total += scratch[w];
  return total;
}

// table[e] = sum over the block of acc[e], e < NN * NN.  part: waves * NN * NN doubles of LDS.
template <int NN>
__device__ __forceinline__ void pa_reduce_table(const double (&acc)[NN * NN], double *part,
                                                double *table) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // (part and table of the bin before have been read)
#pragma unroll
  for (int e = 0; e < NN * NN; ++e) {
    const double v = wave_sum(acc[e]);
    if (lane == 0) part[wave * NN * NN + e] = v;
  }
  __syncthreads();
  if (threadIdx.x < NN * NN) {
    const int nw = (blockDim.x + 63) >> 6;
    double s = 0.0;
    for (int w = 0; w < nw; ++w) s += part[w * NN * NN + threadIdx.x];
    table[threadIdx.x] = s;
  }
  __syncthreads();
}

// numpy's sum over a contiguous axis of NN <= 8 doubles: in order below 8, the tree of its
// eight-accumulator pairwise loop at 8
template <int NN>
__device__ __forceinline__ double pa_numpy_sum(const double (&t)[NN]) {
  if constexpr (NN == 8) {
    return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
  } else {
    double s = t[0];
#pragma unroll
    for (int i = 1; i < NN; ++i) s += t[i];
    return s;
  }
}

// ---------------------------------------------------------------- best permutation
// permutation number idx of itertools.permutations(range(NN)) (lexicographic): the factorial digits
// of idx pick from the components that are left, kept as nibbles of one word
template <int NN>
__device__ __forceinline__ void pa_decode(int idx, int (&p)[NN]) {
  unsigned long long avail = 0x76543210ull;
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    const int f = pa_factorial(NN - 1 - i);
    const int d = idx / f;
    idx -= d * f;
    const int sh = 4 * d;
    p[i] = (int)((avail >> sh) & 0xFull);
    const unsigned long long low = avail & ((1ull << sh) - 1ull);
    avail = low | ((avail >> (sh + 4)) << sh);
  }
}

// numpy.argmax's order on (score, index): the larger score, on equal scores the smaller index; a
// NaN beats every number (argmax returns the first NaN)
__device__ __forceinline__ bool pa_better(double s1, int i1, double s2, int i2) {
  const bool n1 = s1 != s1, n2 = s2 != s2;
  if (n1 || n2) return (n1 && n2) ? (i1 < i2) : n1;
  return s1 > s2 || (s1 == s2 && i1 < i2);
}

// Index of the first permutation p, in itertools.permutations(range(NN)) order, that maximises
// sum_i gain[p[i] * NN + i].  gain: NN * NN doubles of LDS, complete before the call.  Every thread
// of the block calls it and gets the index.  red_s / red_i: PA_MAX_WAVES entries of LDS each.
template <int NN>
__device__ __forceinline__ int pa_best_permutation(const double *gain, double *red_s, int *red_i) {
  constexpr int NPERM = pa_factorial(NN);
  double best_s = -HUGE_VAL;
  int best_i = INT_MAX;
  for (int idx = threadIdx.x; idx < NPERM; idx += blockDim.x) {
    int p[NN];
    pa_decode<NN>(idx, p);
    double t[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) t[i] = gain[p[i] * NN + i];
    const double s = pa_numpy_sum<NN>(t);
    if (pa_better(s, idx, best_s, best_i)) {
      best_s = s;
      best_i = idx;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double os = __shfl_xor(best_s, off, 64);
    const int oi = __shfl_xor(best_i, off, 64);
    if (pa_better(os, oi, best_s, best_i)) {
      best_s = os;
      best_i = oi;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // (red_* of the bin before have been read)
  if (lane == 0) {
    red_s[wave] = best_s;
    red_i[wave] = best_i;
  }
  __syncthreads();
  const int nw = (blockDim.x + 63) >> 6;
  best_s = red_s[0];
  best_i = red_i[0];
  for (int w = 1; w < nw; ++w)
    if (pa_better(red_s[w], red_i[w], best_s, best_i)) {
      best_s = red_s[w];
      best_i = red_i[w];
    }
  return best_i;  // (index 0 survives ties, so it is always a valid index)
}

// gain[a, i] = (2 table[a, i] - sum_j table[a, j]) / denom[i] of the score solver, in place on the
// table of sums over the frames (LDS); inv_frames is applied by division as the host does
template <int NN>
__device__ __forceinline__ void pa_score_gain(double *table, const double *denom, double n_frames) {
  double g = 0.0;
  if (threadIdx.x < NN * NN) {
    const int a = threadIdx.x / NN, i = threadIdx.x % NN;
    double row[NN];
#pragma unroll
    for (int j = 0; j < NN; ++j) row[j] = table[a * NN + j] / n_frames;
    const double total = pa_numpy_sum<NN>(row);
    double mine = row[0];
#pragma unroll
    for (int j = 1; j < NN; ++j) mine = (j == i) ? row[j] : mine;
    g = (2.0 * mine - total) / denom[i];
  }
  __syncthreads();
  if (threadIdx.x < NN * NN) table[threadIdx.x] = g;
  __syncthreads();
}

template <int NN>
static __global__ __launch_bounds__(PA_BIN_THREADS) void k_best_permutation(
    const double *__restrict__ tables, int *__restrict__ out) {
  __shared__ double gain[NN * NN];
  __shared__ double red_s[PA_MAX_WAVES];
  __shared__ int red_i[PA_MAX_WAVES];
  const long long m = blockIdx.x;
  if (threadIdx.x < NN * NN) gain[threadIdx.x] = tables[m * NN * NN + threadIdx.x];
  __syncthreads();
  const int idx = pa_best_permutation<NN>(gain, red_s, red_i);
  if (threadIdx.x == 0) out[m] = idx;
}

// ---------------------------------------------------------------- correlation solver
// envelope[b, f, n, t] = |y| / floor(sqrt(sum_n |y|^2)),  overlap[b, f] = sum_t (sum_n envelope)^2
// (= the sum of all entries of P P^T).  One workgroup per (bin, mixture).
template <int NN>
static __global__ __launch_bounds__(PA_BIN_THREADS) void k_envelope_overlap(
    const double *__restrict__ y, int is_complex, long long sb, long long sn, long long sf,
    double *__restrict__ envelope, double *__restrict__ overlap, int F, int T, int floor_kind,
    double floor_eps) {
  __shared__ double scratch[PA_MAX_WAVES];
  const int f = blockIdx.x, b = blockIdx.y;
  const int width = is_complex ? 2 : 1;  // (strides count elements of the sequence)
  const double *src = y + ((long long)b * sb + (long long)f * sf) * width;
  double *dst = envelope + ((long long)b * F + f) * NN * T;
  double acc = 0.0;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    double a[NN];
    double ss = 0.0;
#pragma unroll
    for (int n = 0; n < NN; ++n) {
      const double *p = src + ((long long)n * sn + t) * width;
      a[n] = is_complex ? hypot(p[0], p[1]) : fabs(p[0]);
      ss += a[n] * a[n];
    }
    const double norm = apply_floor(sqrt(ss), floor_kind, floor_eps);
    double col = 0.0;
#pragma unroll
    for (int n = 0; n < NN; ++n) {
      const double e = a[n] / norm;
      dst[(long long)n * T + t] = e;
      col += e;
    }
    acc += col * col;
  }
  const double total = pa_block_sum(acc, scratch);
  if (threadIdx.x == 0) overlap[(long long)b * F + f] = total;
}

// The sweep of the correlation solver: one workgroup per mixture visits the bins in `order`.  The
// criterion (NN x T) stays in LDS; column t of it belongs to the thread that owns frame t, so only
// the table and the choice cross threads.
template <int NN>
static __global__ __launch_bounds__(PA_SWEEP_THREADS) void k_correlation_sweep(
    const double *__restrict__ envelope, const int *__restrict__ order, int *__restrict__ perm,
    int F, int T) {
  extern __shared__ __attribute__((aligned(16))) double pa_lds[];
  double *crit = pa_lds;                          // NN * T
  double *part = crit + (size_t)NN * T;           // PA_MAX_WAVES * NN * NN
  double *table = part + PA_MAX_WAVES * NN * NN;  // NN * NN
  double *red_s = table + NN * NN;                // PA_MAX_WAVES
  int *red_i = reinterpret_cast<int *>(red_s + PA_MAX_WAVES);
  const int b = blockIdx.x;
  const double *env = envelope + (long long)b * F * NN * T;
  const int *ord = order + (long long)b * F;
  int *out = perm + (long long)b * F * NN;

  int f = min(max(ord[0], 0), F - 1);
  for (int t = threadIdx.x; t < T; t += blockDim.x)
#pragma unroll
    for (int i = 0; i < NN; ++i) crit[i * T + t] = env[((long long)f * NN + i) * T + t];
  if (threadIdx.x < NN) out[f * NN + threadIdx.x] = threadIdx.x;

  for (int k = 1; k < F; ++k) {
    f = min(max(ord[k], 0), F - 1);
    const double *P = env + (long long)f * NN * T;
    double acc[NN * NN];
#pragma unroll
    for (int e = 0; e < NN * NN; ++e) acc[e] = 0.0;
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
      double p[NN];
#pragma unroll
      for (int a = 0; a < NN; ++a) p[a] = P[(long long)a * T + t];
#pragma unroll
      for (int i = 0; i < NN; ++i) {
        const double c = crit[i * T + t];
#pragma unroll
        for (int a = 0; a < NN; ++a) acc[a * NN + i] += p[a] * c;
      }
    }
    pa_reduce_table<NN>(acc, part, table);
    const int idx = pa_best_permutation<NN>(table, red_s, red_i);
    int chosen[NN];
    pa_decode<NN>(idx, chosen);
    for (int t = threadIdx.x; t < T; t += blockDim.x)
#pragma unroll
      for (int i = 0; i < NN; ++i) crit[i * T + t] += P[(long long)chosen[i] * T + t];
#pragma unroll
    for (int i = 0; i < NN; ++i)
      if (threadIdx.x == i) out[f * NN + i] = chosen[i];
  }
}

// ---------------------------------------------------------------- score solver
// normalized[b, f, n, :] = (x - mean) / std (population), one workgroup per (bin * NN + n, mixture)
static __global__ __launch_bounds__(PA_BIN_THREADS) void k_score_normalize(
    const double *__restrict__ x, long long sb, long long sn, long long sf,
    double *__restrict__ normalized, int N, int F, int T) {
  __shared__ double scratch[PA_MAX_WAVES];
  const int f = blockIdx.x / N, n = blockIdx.x % N, b = blockIdx.y;
  const double *src = x + (long long)b * sb + (long long)n * sn + (long long)f * sf;
  double *dst = normalized + (((long long)b * F + f) * N + n) * T;
  double s = 0.0;
  for (int t = threadIdx.x; t < T; t += blockDim.x) s += src[t];
  const double mean = pa_block_sum(s, scratch) / T;
  double q = 0.0;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const double d = src[t] - mean;
    q += d * d;
  }
  const double sd = sqrt(pa_block_sum(q, scratch) / T);
  for (int t = threadIdx.x; t < T; t += blockDim.x) dst[t] = (src[t] - mean) / sd;
}

// centroid[b, n, t] = (sum_f normalized[b, f, perm[b, f, n], t]) / F, the bins folded in bin order
static __global__ __launch_bounds__(PA_BIN_THREADS) void k_score_centroid(
    const double *__restrict__ normalized, const int *__restrict__ perm,
    double *__restrict__ centroid, int N, int F, int T) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y, b = blockIdx.z;
  if (t >= T) return;
  const double *src = normalized + (long long)b * F * N * T + t;
  const int *pm = perm + (long long)b * F * N + n;
  double s = 0.0;
  for (int f = 0; f < F; ++f) {
    const int row = min(max(pm[(long long)f * N], 0), N - 1);
    s += src[((long long)f * N + row) * T];
  }
  centroid[((long long)b * N + n) * T + t] = s / F;
}

// centroid_std[b, n]: the population standard deviation of a centroid over the frames
static __global__ __launch_bounds__(PA_BIN_THREADS) void k_score_centroid_std(
    const double *__restrict__ centroid, double *__restrict__ centroid_std, int T) {
  __shared__ double scratch[PA_MAX_WAVES];
  const double *src = centroid + (long long)blockIdx.x * T;
  double s = 0.0;
  for (int t = threadIdx.x; t < T; t += blockDim.x) s += src[t];
  const double mean = pa_block_sum(s, scratch) / T;
  double q = 0.0;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const double d = src[t] - mean;
    q += d * d;
  }
  const double var = pa_block_sum(q, scratch) / T;
  if (threadIdx.x == 0) centroid_std[blockIdx.x] = sqrt(var);
}

// One step of the global stage for every bin on its own: the table against the centroids, the gain,
// the best permutation, composed into perm[b, f, :].  One workgroup per (bin, mixture).
template <int NN>
static __global__ __launch_bounds__(PA_BIN_THREADS) void k_score_global_assign(
    const double *__restrict__ normalized, const double *__restrict__ centroid,
    const double *__restrict__ centroid_std, int *perm, int F, int T, int floor_kind,
    double floor_eps) {
  __shared__ double part[(PA_BIN_THREADS / 64) * NN * NN];
  __shared__ double table[NN * NN];
  __shared__ double denom[NN];
  __shared__ double red_s[PA_MAX_WAVES];
  __shared__ int red_i[PA_MAX_WAVES];
  __shared__ int current[NN];
  const int f = blockIdx.x, b = blockIdx.y;
  int *pm = perm + ((long long)b * F + f) * NN;
  if (threadIdx.x < NN) {
    current[threadIdx.x] = min(max(pm[threadIdx.x], 0), NN - 1);
    denom[threadIdx.x] = apply_floor(centroid_std[b * NN + threadIdx.x], floor_kind, floor_eps);
  }
  __syncthreads();
  const double *rows = normalized + ((long long)b * F + f) * NN * T;
  const double *cen = centroid + (long long)b * NN * T;
  int cur[NN];
#pragma unroll
  for (int a = 0; a < NN; ++a) cur[a] = current[a];
  double acc[NN * NN];
#pragma unroll
  for (int e = 0; e < NN * NN; ++e) acc[e] = 0.0;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    double s[NN];
#pragma unroll
    for (int a = 0; a < NN; ++a) s[a] = rows[(long long)cur[a] * T + t];
#pragma unroll
    for (int j = 0; j < NN; ++j) {
      const double c = cen[(long long)j * T + t];
#pragma unroll
      for (int a = 0; a < NN; ++a) acc[a * NN + j] += s[a] * c;
    }
  }
  pa_reduce_table<NN>(acc, part, table);
  pa_score_gain<NN>(table, denom, (double)T);
  const int idx = pa_best_permutation<NN>(table, red_s, red_i);
  int chosen[NN];
  pa_decode<NN>(idx, chosen);
#pragma unroll
  for (int i = 0; i < NN; ++i)
    if (threadIdx.x == i) pm[i] = current[chosen[i]];
}

// The bins that bin f of the local stage looks at, increasing and without repeats: f-3..f+3 without
// f, f/2-1..f/2+1 and 2f-1..2f+1, clipped to the bins (the last two may contain f itself, as on
// the host).  Returns their number.
__device__ inline int pa_neighbours(int f, int F, int *nb) {
  int count = 0;
  auto add = [&](int g) {
    int pos = count;
    for (int k = 0; k < count; ++k) {
      if (nb[k] == g) return;
      if (nb[k] > g) {
        pos = k;
        break;
      }
    }
    for (int k = count; k > pos; --k) nb[k] = nb[k - 1];
    nb[pos] = g;
    ++count;
  };
  for (int g = max(0, f - 3); g <= min(F - 1, f + 3); ++g)
    if (g != f) add(g);
  for (int g = max(0, f / 2 - 1); g <= min(F - 1, f / 2 + 1); ++g) add(g);
  for (int g = max(0, 2 * f - 1); g <= min(F - 1, 2 * f + 1); ++g) add(g);
  return count;
}

// The local stage: one workgroup per mixture walks the bins in increasing order, local_iter times.
// The rows of a bin are addressed through perm, so a decision is visible to the bins after it as
// soon as the workgroup has passed its barrier; the permutations a bin needs (its own and its
// neighbours') are staged in LDS from there.
template <int NN>
static __global__ __launch_bounds__(PA_SWEEP_THREADS) void k_score_local(
    const double *__restrict__ normalized, const double *__restrict__ centroid_std, int *perm, int F,
    int T, int local_iter, int floor_kind, double floor_eps) {
  __shared__ double part[PA_MAX_WAVES * NN * NN];
  __shared__ double table[NN * NN];
  __shared__ double denom[NN];
  __shared__ double red_s[PA_MAX_WAVES];
  __shared__ int red_i[PA_MAX_WAVES];
  __shared__ int nb[PA_MAX_NEIGHBOURS];
  __shared__ int nb_count;
  __shared__ int nb_perm[PA_MAX_NEIGHBOURS * NN];
  __shared__ int current[NN];
  const int b = blockIdx.x;
  const double *base = normalized + (long long)b * F * NN * T;
  int *pm = perm + (long long)b * F * NN;
  if (threadIdx.x < NN)
    denom[threadIdx.x] = apply_floor(centroid_std[b * NN + threadIdx.x], floor_kind, floor_eps);

  for (int it = 0; it < local_iter; ++it) {
    for (int f = 0; f < F; ++f) {
      __syncthreads();  // (the choice of the bin before is stored; its staging has been read)
      if (threadIdx.x == 0) nb_count = pa_neighbours(f, F, nb);
      __syncthreads();
      const int count = nb_count;
      if (threadIdx.x < count * NN) {
        const int g = nb[threadIdx.x / NN];
        nb_perm[threadIdx.x] = min(max(pm[(long long)g * NN + threadIdx.x % NN], 0), NN - 1);
      }
      if (threadIdx.x >= 64 && threadIdx.x < 64 + NN)
        current[threadIdx.x - 64] = min(max(pm[(long long)f * NN + threadIdx.x - 64], 0), NN - 1);
      __syncthreads();
      int cur[NN];
#pragma unroll
      for (int a = 0; a < NN; ++a) cur[a] = current[a];
      const double *rows = base + (long long)f * NN * T;
      double acc[NN * NN];
#pragma unroll
      for (int e = 0; e < NN * NN; ++e) acc[e] = 0.0;
      for (int t = threadIdx.x; t < T; t += blockDim.x) {
        double anchor[NN];
#pragma unroll
        for (int j = 0; j < NN; ++j) anchor[j] = 0.0;
        for (int k = 0; k < count; ++k) {
          const double *other = base + (long long)nb[k] * NN * T + t;
#pragma unroll
          for (int j = 0; j < NN; ++j) anchor[j] += other[(long long)nb_perm[k * NN + j] * T];
        }
        double s[NN];
#pragma unroll
        for (int a = 0; a < NN; ++a) s[a] = rows[(long long)cur[a] * T + t];
#pragma unroll
        for (int j = 0; j < NN; ++j)
#pragma unroll
          for (int a = 0; a < NN; ++a) acc[a * NN + j] += s[a] * anchor[j];
      }
      pa_reduce_table<NN>(acc, part, table);
      pa_score_gain<NN>(table, denom, (double)T);
      const int idx = pa_best_permutation<NN>(table, red_s, red_i);
      int chosen[NN];
      pa_decode<NN>(idx, chosen);
#pragma unroll
      for (int i = 0; i < NN; ++i)
        if (threadIdx.x == i) pm[(long long)f * NN + i] = current[chosen[i]];
    }
  }
}

// ---------------------------------------------------------------- apply / amplitude
// dst = the sources of src gathered by perm, in 8-byte words.  layout BIN_SOURCE: dst (B, F, N,
// inner), SOURCE_BIN: dst (B, N, F, inner), both contiguous; word w of (b, f, n) of src is at
// b * sb + f * sf + n * sn + w.
static __global__ __launch_bounds__(256) void k_permute_sources(
    const unsigned long long *__restrict__ src, unsigned long long *__restrict__ dst,
    const int *__restrict__ perm, long long total, int N, int F, long long inner, int layout,
    long long sb, long long sf, long long sn) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const long long w = e % inner, r = e / inner;
  int n, f;
  long long b;
  if (layout == SSSPY_PERM_LAYOUT_BIN_SOURCE) {
    n = (int)(r % N);
    f = (int)((r / N) % F);
  } else {
    f = (int)(r % F);
    n = (int)((r / F) % N);
  }
  b = r / ((long long)N * F);
  const int from = min(max(perm[(b * F + f) * N + n], 0), N - 1);
  dst[e] = src[b * sb + f * sf + (long long)from * sn + w];
}

// out[b, n, i, j] = |posterior[b, n, i, j] X[b, reference_id, i, j]|
static __global__ __launch_bounds__(256) void k_amplitude(const double *__restrict__ posterior,
                                                          const c128 *__restrict__ X,
                                                          double *__restrict__ out, long long total,
                                                          int N, int M, long long FT,
                                                          int reference_id) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const long long ft = e % FT, b = e / (FT * N);
  const c128 x = X[(b * M + reference_id) * FT + ft];
  const double g = posterior[e];
  out[e] = hypot(g * x.x, g * x.y);
}

int pa_check(int B, int N, int F, int T, const char *what) {
  if (B <= 0 || F <= 0 || T <= 0 || N < 2) return fail(SSSPY_ERR_BADARG, what);
  if (N > SSSPY_MAX_SOURCES)
    return fail(SSSPY_ERR_UNSUPPORTED,
                "permutation alignment runs on the device for 2..8 sources (N! permutations are "
                "enumerated)");
  if (B > 65535 || (long long)F * N > 0x7fffffff)
    return fail(SSSPY_ERR_UNSUPPORTED, "permutation alignment: too many mixtures or bins for a launch");
  return SSSPY_OK;
}

bool pa_floor_known(int kind) {
  return kind == SSSPY_FLOOR_NONE || kind == SSSPY_FLOOR_MAX || kind == SSSPY_FLOOR_ADD;
}

#define PA_DISPATCH(N_, CALL)                          \
  switch (N_) {                                        \
    case 2: { constexpr int NN = 2; CALL; } break;     \
    case 3: { constexpr int NN = 3; CALL; } break;     \
    case 4: { constexpr int NN = 4; CALL; } break;     \
    case 5: { constexpr int NN = 5; CALL; } break;     \
    case 6: { constexpr int NN = 6; CALL; } break;     \
    case 7: { constexpr int NN = 7; CALL; } break;     \
    case 8: { constexpr int NN = 8; CALL; } break;     \
    default: return ::ssspy::fail(SSSPY_ERR_UNSUPPORTED, "n_sources must be in [2, 8]"); \
  }

}  // namespace
}  // namespace ssspy

using namespace ssspy;

extern "C" {

int ssspy_permutation_route(int N, int T, int solver, int floor_kind) {
  if (N < 1 || T < 1 ||
      (solver != SSSPY_PERM_SOLVER_CORRELATION && solver != SSSPY_PERM_SOLVER_SCORE))
    return -1;
  if (N < 2 || N > SSSPY_MAX_SOURCES || !pa_floor_known(floor_kind)) return SSSPY_PERM_ROUTE_HOST;
  if (solver == SSSPY_PERM_SOLVER_CORRELATION && (long long)N * T > PA_MAX_CRITERION)
    return SSSPY_PERM_ROUTE_HOST;
  return SSSPY_PERM_ROUTE_DEVICE;
}

int ssspy_best_permutation(const double *tables, int *index, long long n_tables, int N,
                           void *stream) {
  SSSPY_REQUIRE(tables && index && n_tables > 0 && n_tables <= 0x7fffffff,
                "best_permutation: bad argument");
  if (int rc = pa_check(1, N, 1, 1, "best_permutation: bad shape")) return rc;
  PA_DISPATCH(N, hipLaunchKernelGGL((k_best_permutation<NN>), dim3((unsigned)n_tables),
                                    dim3(PA_BIN_THREADS), 0, as_stream(stream), tables, index));
  return check_launch("k_best_permutation");
}

int ssspy_permutation_envelope_overlap(const void *sequence, int is_complex, long long stride_b,
                                       long long stride_n, long long stride_f, double *envelope,
                                       double *overlap, int B, int N, int F, int T, int floor_kind,
                                       double floor_eps, void *stream) {
  SSSPY_REQUIRE(sequence && envelope && overlap, "permutation_envelope_overlap: bad argument");
  SSSPY_REQUIRE(stride_b >= 0 && stride_n > 0 && stride_f > 0,
                "permutation_envelope_overlap: bad stride");
  if (int rc = pa_check(B, N, F, T, "permutation_envelope_overlap: bad shape")) return rc;
  if (!pa_floor_known(floor_kind))
    return fail(SSSPY_ERR_UNSUPPORTED, "permutation_envelope_overlap: unknown floor");
  PA_DISPATCH(N, hipLaunchKernelGGL((k_envelope_overlap<NN>), dim3(F, B), dim3(PA_BIN_THREADS), 0,
                                    as_stream(stream), (const double *)sequence,
                                    is_complex ? 1 : 0, stride_b, stride_n, stride_f, envelope,
                                    overlap, F, T, floor_kind, floor_eps));
  return check_launch("k_envelope_overlap");
}

int ssspy_permutation_correlation_sweep(const double *envelope, const int *order, int *perm, int B,
                                        int N, int F, int T, void *stream) {
  SSSPY_REQUIRE(envelope && order && perm, "permutation_correlation_sweep: bad argument");
  if (int rc = pa_check(B, N, F, T, "permutation_correlation_sweep: bad shape")) return rc;
  if ((long long)N * T > PA_MAX_CRITERION)
    return fail(SSSPY_ERR_UNSUPPORTED,
                "permutation_correlation_sweep: the criterion (n_sources x n_frames doubles) must "
                "fit in LDS, n_sources * n_frames <= 16384");
  const size_t smem = ((size_t)N * T + (size_t)PA_MAX_WAVES * N * N + (size_t)N * N + PA_MAX_WAVES) *
                          sizeof(double) + PA_MAX_WAVES * sizeof(int);
  PA_DISPATCH(N, {
    if (smem > 48 * 1024) {
      // (granted once per instantiation and device, not on every launch)
      static size_t granted[64] = {};
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
      if (smem > granted[dev]) {
        hipError_t e = hipFuncSetAttribute((const void *)k_correlation_sweep<NN>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return fail(SSSPY_ERR_HIP, hipGetErrorString(e));
        granted[dev] = smem;
      }
    }
    hipLaunchKernelGGL((k_correlation_sweep<NN>), dim3(B), dim3(PA_SWEEP_THREADS), smem,
                       as_stream(stream), envelope, order, perm, F, T);
  });
  return check_launch("k_correlation_sweep");
}

int ssspy_permutation_score_normalize(const double *sequence, long long stride_b, long long stride_n,
                                      long long stride_f, double *normalized, int B, int N, int F,
                                      int T, void *stream) {
  SSSPY_REQUIRE(sequence && normalized, "permutation_score_normalize: bad argument");
  SSSPY_REQUIRE(stride_b >= 0 && stride_n > 0 && stride_f > 0,
                "permutation_score_normalize: bad stride");
  if (int rc = pa_check(B, N, F, T, "permutation_score_normalize: bad shape")) return rc;
  hipLaunchKernelGGL(k_score_normalize, dim3((unsigned)(F * N), B), dim3(PA_BIN_THREADS), 0,
                     as_stream(stream), sequence, stride_b, stride_n, stride_f, normalized, N, F, T);
  return check_launch("k_score_normalize");
}

int ssspy_permutation_score_global(const double *normalized, int *perm, double *centroid,
                                   double *centroid_std, int B, int N, int F, int T, int global_iter,
                                   int floor_kind, double floor_eps, void *stream) {
  SSSPY_REQUIRE(normalized && perm && centroid && centroid_std && global_iter >= 0,
                "permutation_score_global: bad argument");
  if (int rc = pa_check(B, N, F, T, "permutation_score_global: bad shape")) return rc;
  if (!pa_floor_known(floor_kind))
    return fail(SSSPY_ERR_UNSUPPORTED, "permutation_score_global: unknown floor");
  hipStream_t st = as_stream(stream);
  // (with global_iter == 0 the centroid of the sequences as they are still gives the denominator)
  const int rounds = global_iter > 0 ? global_iter : 1;
  for (int it = 0; it < rounds; ++it) {
    hipLaunchKernelGGL(k_score_centroid, dim3((T + PA_BIN_THREADS - 1) / PA_BIN_THREADS, N, B),
                       dim3(PA_BIN_THREADS), 0, st, normalized, perm, centroid, N, F, T);
    if (int rc = check_launch("k_score_centroid")) return rc;
    hipLaunchKernelGGL(k_score_centroid_std, dim3(B * N), dim3(PA_BIN_THREADS), 0, st, centroid,
                       centroid_std, T);
    if (int rc = check_launch("k_score_centroid_std")) return rc;
    if (global_iter == 0) break;
    PA_DISPATCH(N, hipLaunchKernelGGL((k_score_global_assign<NN>), dim3(F, B), dim3(PA_BIN_THREADS),
                                      0, st, normalized, centroid, centroid_std, perm, F, T,
                                      floor_kind, floor_eps));
    if (int rc = check_launch("k_score_global_assign")) return rc;
  }
  return SSSPY_OK;
}

int ssspy_permutation_score_local(const double *normalized, const double *centroid_std, int *perm,
                                  int B, int N, int F, int T, int local_iter, int floor_kind,
                                  double floor_eps, void *stream) {
  SSSPY_REQUIRE(normalized && centroid_std && perm && local_iter >= 0,
                "permutation_score_local: bad argument");
  if (int rc = pa_check(B, N, F, T, "permutation_score_local: bad shape")) return rc;
  if (!pa_floor_known(floor_kind))
    return fail(SSSPY_ERR_UNSUPPORTED, "permutation_score_local: unknown floor");
  if (local_iter == 0) return SSSPY_OK;
  PA_DISPATCH(N, hipLaunchKernelGGL((k_score_local<NN>), dim3(B), dim3(PA_SWEEP_THREADS), 0,
                                    as_stream(stream), normalized, centroid_std, perm, F, T,
                                    local_iter, floor_kind, floor_eps));
  return check_launch("k_score_local");
}

int ssspy_permute_sources(const void *src, void *dst, const int *perm, int B, int N, int F,
                          long long inner_words, int layout, long long stride_b, long long stride_f,
                          long long stride_n, void *stream) {
  SSSPY_REQUIRE(src && dst && perm && src != dst, "permute_sources: bad argument (out of place only)");
  SSSPY_REQUIRE(B > 0 && N > 0 && F > 0 && inner_words > 0, "permute_sources: bad shape");
  SSSPY_REQUIRE(layout == SSSPY_PERM_LAYOUT_BIN_SOURCE || layout == SSSPY_PERM_LAYOUT_SOURCE_BIN,
                "permute_sources: bad layout");
  SSSPY_REQUIRE(stride_b >= 0 && stride_f > 0 && stride_n > 0, "permute_sources: bad stride");
  const long long total = (long long)B * N * F * inner_words;
  const long long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return fail(SSSPY_ERR_UNSUPPORTED, "permute_sources: array too large");
  hipLaunchKernelGGL(k_permute_sources, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                     (const unsigned long long *)src, (unsigned long long *)dst, perm, total, N, F,
                     inner_words, layout, stride_b, stride_f, stride_n);
  return check_launch("k_permute_sources");
}

int ssspy_permutation_amplitude(const double *posterior, const void *X, double *out, int B, int N,
                                int M, int F, int T, int reference_id, void *stream) {
  SSSPY_REQUIRE(posterior && X && out && B > 0 && N > 0 && M > 0 && F > 0 && T > 0,
                "permutation_amplitude: bad argument");
  SSSPY_REQUIRE(reference_id >= 0 && reference_id < M, "permutation_amplitude: bad reference_id");
  const long long FT = (long long)F * T, total = (long long)B * N * FT;
  const long long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return fail(SSSPY_ERR_UNSUPPORTED, "permutation_amplitude: array too large");
  hipLaunchKernelGGL(k_amplitude, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), posterior,
                     (const c128 *)X, out, total, N, M, FT, reference_id);
  return check_launch("k_amplitude");
}

}  // extern "C"
