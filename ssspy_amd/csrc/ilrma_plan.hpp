// The launch plan of the ILRMA entry points (ilrma_api.hip): which kernels every pass of a call
// takes, decided once from (B, N, F, T, K, domain, source_model) by make_ilrma_plan() -- with the size
// helpers the only caller of the predicates -- and the scratch layout the entry points share.  Host
// only; validates nothing.  The table of routes is in DESIGN.md, section 4.
#pragma once

#include <cstdlib>

#include "common.hpp"
#include "ilrma_params.hpp"
#include "tail_plan.hpp"
#include "wide_n.hpp"

namespace ssspy {

// ------------------------------------------------------------------ 1. per-N launchers, dispatch
#define DECL_N(n)                                                                               \
  int ilrma_basis_n##n(const void *, const void *, const double *, double *, const double *,   \
                       IlrmaDims, hipStream_t);                                                \
  int ilrma_activation_n##n(const void *, const void *, const double *, const double *, double *, \
                            int, IlrmaDims, hipStream_t);                                      \
  int ilrma_wcov_n##n(const void *, const void *, const double *, const double *, void *,       \
                      IlrmaDims, hipStream_t);                                                 \
  size_t ilrma_loss_ws_bytes_n##n(int, int);                                                   \
  int ilrma_loss_n##n(const void *, const void *, const double *, const double *, double *,     \
                      void *, IlrmaDims, hipStream_t);
DECL_N(2) DECL_N(3) DECL_N(4) DECL_N(5) DECL_N(6) DECL_N(7) DECL_N(8)
#undef DECL_N

// throughput variants (ilrma_fast.hip): n_basis <= 64 (two / four k tiles above 16 / 32), n_sources <= 4, models
// of fast_model_id()
#define DECL_FAST(n)                                                                           \
  int ilrma_fast_basis_n##n(const void *, const void *, const double *, double *, const double *, \
                            int, int, int, int, int, double, double *, int, double, int,        \
                            double *, void *, int, hipStream_t, long long);                     \
  int ilrma_fast_basis_loss_slots_n##n(int, int, int);                                          \
  size_t ilrma_fast_loss_ws_bytes_n##n(int, int);                                               \
  int ilrma_fast_activation_n##n(const void *, const void *, const double *, double *,         \
                                 double *, int, int, int, int, int, int, double, int,           \
                                 hipStream_t, int *, int, int, double);                         \
  int ilrma_fast_wcov_n##n(const void *, const void *, const double *, const double *, void *, \
                           int, int, int, int, void *, int, double, int, double, hipStream_t,  \
                           int *, int *);                                                      \
  int ilrma_fast_loss_n##n(const void *, const void *, const double *, const double *, double *, \
                           void *, int, int, int, int, int, double, hipStream_t);
DECL_FAST(2) DECL_FAST(3) DECL_FAST(4)
#undef DECL_FAST

// latency variants for a handful of mixtures (ilrma_small.hip): n_basis <= 16, n_sources <= 4
#define DECL_SMALL(n)                                                                           \
  size_t ilrma_small_scratch_n##n(int, int, int, int);                                            \
  int ilrma_small_activation_n##n(const void *, const void *, const double *, double *, int, int, \
                                  int, int, int, double, double *, int, double, int,              \
                                  hipStream_t);                                                   \
  int ilrma_small_ip1_n##n(const void *, int, int, long long, const void *, void *, int, int, int, \
                           double, double *, int *, hipStream_t);                                 \
  int ilrma_small_ip1_logdet_n##n(const void *, int, int, long long, const void *, void *, int,   \
                                  int, int, double, double *, int *, double *, long long,         \
                                  hipStream_t);                                                   \
  int ilrma_small_norm_n##n(void *, double *, const double *, int, int, int, double, int, double, \
                            hipStream_t);
DECL_SMALL(2) DECL_SMALL(3) DECL_SMALL(4)
#undef DECL_SMALL

// wide_cov.hip: weighted covariance of 6..8 channels on the matrix cores
bool wide_weighted_cov_ok(int N, int S, int F, int T, int kind);
int wide_weighted_cov(const void *A, const double *weight, int kind, void *U, int B, int N, int S,
                      int F, int T, hipStream_t st);
size_t wb_loss_ws_bytes(int B, int N, int F, int T);  // wide_basis.hip

// `return fn_n<N>(...)`.  The tuned and latency units exist for 2..4 sources: their callers have
// a plan that says so (or test the range themselves).
#define ILRMA_FAST_DISPATCH(N_, fn, ...)             \
  switch (N_) {                                      \
    case 2: return fn##_n2(__VA_ARGS__);             \
    case 3: return fn##_n3(__VA_ARGS__);             \
    default: return fn##_n4(__VA_ARGS__);            \
  }
#define ILRMA_DISPATCH_OR(N_, otherwise, fn, ...)                                    \
  switch (N_) {                                                                      \
    case 2: return fn##_n2(__VA_ARGS__);                                             \
    case 3: return fn##_n3(__VA_ARGS__);                                             \
    case 4: return fn##_n4(__VA_ARGS__);                                             \
    case 5: return fn##_n5(__VA_ARGS__);                                             \
    case 6: return fn##_n6(__VA_ARGS__);                                             \
    case 7: return fn##_n7(__VA_ARGS__);                                             \
    case 8: return fn##_n8(__VA_ARGS__);                                             \
    default: return otherwise;                                                       \
  }
#define ILRMA_DISPATCH(N_, fn, ...)                                                               \
  ILRMA_DISPATCH_OR(N_, fail(SSSPY_ERR_UNSUPPORTED, "ILRMA: n_sources must be in [2, 8]"), fn, \
                    __VA_ARGS__)

static inline bool tuned_sources(int N) { return N >= 2 && N <= 4; }
static inline size_t small_scratch(int B, int N, int F, int T, int K) {
  if (!tuned_sources(N)) return 0;
  ILRMA_FAST_DISPATCH(N, ilrma_small_scratch, B, F, T, K);
}
static inline size_t tuned_loss_ws_bytes(int B, int N, int F) {
  if (!tuned_sources(N)) return 0;
  ILRMA_FAST_DISPATCH(N, ilrma_fast_loss_ws_bytes, B, F);
}
static inline int tuned_basis_loss_slots(int B, int N, int F, int T) {
  if (!tuned_sources(N)) return 0;
  ILRMA_FAST_DISPATCH(N, ilrma_fast_basis_loss_slots, B, F, T);
}
static inline size_t generic_loss_ws_bytes(int B, int N, int F) {
  ILRMA_DISPATCH_OR(N, 0, ilrma_loss_ws_bytes, B, F);
}

// ------------------------------------------------------------------------------- 2. predicates
// the tuned kernels: n_sources <= 4, n_basis <= 16 and one of the models ilrma_fast.hip carries
// (its FM_* ids): Gauss at domain 2 (MM or ME), 1 or any other value in (0, 2), Student-t and GGD
// at domain 2;
// `source_model` may carry the SSSPY_SOURCE_ME flag.  -1: generic kernels.
static inline int fast_model_id(double domain, int source_model) {
  const int base = source_model & 0xff;
  const bool me = (source_model & SSSPY_SOURCE_ME) != 0;
  if (domain == 2.0) {
    if (base == SSSPY_SOURCE_GAUSS) return 0;
    if (base == SSSPY_SOURCE_T) return 1;
    if (base == SSSPY_SOURCE_GGD) return 2;
  }
  if (domain == 1.0 && base == SSSPY_SOURCE_GAUSS && !me) return 3;
  // Gauss at any other domain in (0, 2): the powers R^((p+2)/p), R^(2/p) as exp2(e log2 R)
  if (base == SSSPY_SOURCE_GAUSS && !me && domain > 0.0 && domain < 2.0) return 4;
  return -1;
}
// (one channel of a mixture must fit the 32-bit offset of a buffer descriptor: F T 16 bytes < 4 GiB)
static inline bool fast_path(int N, int F, int T, int K, double domain,
                             int source_model = SSSPY_SOURCE_GAUSS) {
  static const bool disabled = std::getenv("SSSPY_AMD_NO_FAST") != nullptr;
  return !disabled && fast_model_id(domain, source_model) >= 0 && tuned_sources(N) && K <= 64 &&
         (long long)F * T * 16 < (1ll << 32);
}

// The latency kernels (ilrma_small.hip) serve batches whose bin tiles do not fill the chip with the
// throughput kernels' 64-bin work items: B * ceil(F / 16) <= 350, i.e. up to 5 mixtures of 1025 bins --
// round 4: with the cost-based tail plan the throughput kernels win from 6 mixtures on, 29.7 k
// against 27.4 k mixture-iterations/s at 9, benchmarks/batch_sweep.py; it was 640:
// up to 9 mixtures of 1025 bins).
static inline bool small_path(int B, int N, int F, int T, int K, double domain,
                              int source_model = SSSPY_SOURCE_GAUSS) {
  const long long max_items = 350;
  return K <= 16 && fast_path(N, F, T, K, domain, source_model) &&
         (long long)B * ((F + 15) / 16) <= max_items;
}

// More than 4 sources on the tuned NMF passes: the multiplicative updates of source n need only
// |y_n|^2 and (T_n, V_n), and (B, N, ...) tensors are (B N / G, G, ...) tensors in memory, so a wide
// mixture is walked as N / G "mixtures" of G sources over the separated spectrogram y = W x (formed
// once by ssspy_separate; the ISS / IPA state is y already).  Returns the group size G (4, 3 or 2)
// or 0 when the shape has none (N <= 4, N = 5 or 7, or the model / n_basis is off the tuned path).
static inline int source_group(int N, int F, int T, int K, double domain, int source_model) {
  if (N <= 4) return 0;
  for (int G = 4; G >= 2; --G)
    if (N % G == 0 && fast_path(G, F, T, K, domain, source_model)) return G;
  return 0;
}

// shapes that may take the wide-basis path of wide_basis.hip (its buffers are sized for them; the
// source model, which the workspace query does not know, decides at the call)
// The register-tiled passes win up to 32 bases (16: 1.0 ms, 32: 1.6 ms per iteration at 32 mixtures of
// the configs[1] shape); from 33 on their four-k-tile form (4.1-4.7 ms) loses to the dense products
// (3.1-3.2 ms; 80: 4.1, 128: 4.6, 256: 7.1, 1024: 22.8 -- benchmarks/wide_basis.py, round 4).
static inline bool wide_basis_shape(int N, int K) {
  return K >= 33 || N > SSSPY_MAX_SOURCES;
}
// The general form (any source count above 4, e.g. 5 or 7): the B N sources of the batch, in memory
// order, are cut into at most three runs of `count` groups of G sources each -- groups of 4 and one
// or two closing groups of 3 / 2 sources -- and every run is one launch of the tuned kernels on its
// slice of y, T and V.  Returns the number of runs (0: not on the grouped path).
struct SourceRun {
  long long first;  // first source of the run in the flat (B N) order
  int count, G;     // `count` groups of G sources
};
static inline int source_runs(int B, int N, int F, int T, int K, double domain, int source_model,
                              SourceRun (&run)[3]) {
  if (N <= 4) return 0;
  if (K > 32) return 0;  // the dense products win from 33 bases on (wide_basis_shape)
  if (const int G = source_group(N, F, T, K, domain, source_model)) {
    run[0] = SourceRun{0, B * (N / G), G};
    return 1;
  }
  for (int G = 2; G <= 4; ++G)
    if (!fast_path(G, F, T, K, domain, source_model)) return 0;
  const long long S = (long long)B * N;  // >= 5
  const int r = (int)(S % 4);
  const int tail = r == 0 ? 0 : (r == 1 ? 5 : r);  // 5 = 3 + 2
  int n = 0;
  if (S - tail > 0) run[n++] = SourceRun{0, (int)((S - tail) / 4), 4};
  if (tail == 5) {
    run[n++] = SourceRun{S - 5, 1, 3};
    run[n++] = SourceRun{S - 2, 1, 2};
  } else if (tail) {
    run[n++] = SourceRun{S - tail, 1, tail};
  }
  return n;
}

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline int ngroups_of(int N) { return N <= 4 ? 1 : (N + 1) / 2; }

// number of bin chunks the activation pass splits into (partials are summed by the finalize
// kernel): enough blocks to occupy the chip for small batches, one chunk for large ones.
static inline int act_chunks(int B, int N, int F, int T, int K) {
  const long long blocks0 = (long long)B * ngroups_of(N) * ((T + 63) / 64) * ((K + 15) / 16);
  const int ntiles = (F + 15) / 16;
  // (round 4: chunk count by the cost search of tail_plan.hpp instead of "just fill one round";
  //  24 mixtures of the configs[1] shape: 5 chunks in two short rounds instead of 3 in two long ones)
  const int want = best_split(blocks0, ntiles, 512, 16, 2048);
  // a single chunk finishes in place (no partial sums): keep it whenever the batch fills the chip
  return blocks0 >= 2048 ? 1 : want;
}

// ---------------------------------------------------------------------------------- 3. the plan
enum class NmfRoute { Grouped, Tuned, WideBasis, Generic };
enum class LossRoute { Tuned, WideBasis, Generic };
enum class CovRoute { RuntimeN, WideBasis, MatrixCore, Tuned, Generic };

struct IlrmaPlan {
  int N, K;
  // the model as the tuned kernels take it: id (-1: none), parameter -- dof (t), beta (GGD), the
  // domain (id 4) -- and the ME switch; `gauss`: the base model, with or without ME
  int fm_id, me;
  double fm_param;
  bool gauss;
  // basis and activation passes share one route; Grouped: one launch of the tuned kernels per run
  NmfRoute nmf;
  SourceRun runs[3];
  int nruns;
  int act_chunks;           // bin chunks of the activation pass (1: no partial sums)
  bool act_latency;         // Tuned, a handful of mixtures: ilrma_small.hip and its own fold
  bool act_in_place;        // Tuned, one chunk, n_basis <= 16: the pass may apply the update itself
  bool basis_out_of_place;  // above 16 bases several items per bin group read the old basis
  TailPlan basis_tail;      // frame splits of the Tuned basis pass ({0, 0, 1} elsewhere)
  LossRoute loss;
  bool loss_byproduct;  // the Tuned basis pass can leave the data term (not Student-t: its term is
                        // not linear in the pass's accumulators)
  int loss_slots, logdet_slots;  // raw slots per mixture of that by-product (0: none)
  // covariance: cov_route() decides with what the call has at hand
  bool runtime_n;        // 9..16 sources: covariance, IP1, normalisation and loss of wide_n.hip
  bool cov_matrix_core;  // 6..8 sources: weights + wide_cov.hip
  bool cov_tuned;        // 2..4 sources on a model of the tuned kernels
  // ip1_update
  bool power_once;   // Grouped or WideBasis: |W x|^2 once for the NMF passes and covariance weights
  bool ip1_latency;  // covariance records, IP1 and the output power in one latency kernel
  // what the workspace is sized by, the same for every model (IlrmaWs)
  bool weights_buf;  // ybuf, wbuf: more than 4 sources or wide-basis shape
  bool dense_buf;    // gb, gnd: wide-basis shape
  int summary;       // SSSPY_ROUTE_*: what ssspy_ilrma_route() answers
};

// fast_path implies at most 4 sources, so "tuned" and "grouped" exclude each other, and n_basis >= 33
// always leaves both for the dense products: one NMF route, first match of
// grouped, tuned (n_basis <= 32), wide-basis shape, generic
static inline IlrmaPlan make_ilrma_plan(int B, int N, int F, int T, int K, double domain,
                                        int source_model, double model_param = 0.0) {
  IlrmaPlan p;
  p.N = N;
  p.K = K;
  p.fm_id = fast_model_id(domain, source_model);
  p.fm_param = p.fm_id == 4 ? domain : model_param;
  p.me = (source_model & SSSPY_SOURCE_ME) ? 1 : 0;
  p.gauss = (source_model & 0xff) == SSSPY_SOURCE_GAUSS;
  const bool fast = fast_path(N, F, T, K, domain, source_model);
  const bool small = small_path(B, N, F, T, K, domain, source_model);
  const bool wide = wide_basis_shape(N, K);
  p.nruns = source_runs(B, N, F, T, K, domain, source_model, p.runs);
  p.nmf = p.nruns               ? NmfRoute::Grouped
          : (fast && K <= 32)   ? NmfRoute::Tuned
          : wide                ? NmfRoute::WideBasis
                                : NmfRoute::Generic;
  const bool tuned = p.nmf == NmfRoute::Tuned;
  p.act_chunks = act_chunks(B, N, F, T, K);
  p.act_latency = small;
  // (-DSSSPY_NO_ACT_INPLACE: the record and the fold throughout, for A / B runs)
#ifdef SSSPY_NO_ACT_INPLACE
  p.act_in_place = false;
#else
  p.act_in_place = tuned && p.act_chunks == 1 && K <= 16;
#endif
  p.basis_out_of_place = K > 16;
  p.basis_tail = tuned ? ilrma_basis_plan(B, F, T, K) : TailPlan{0, 0, 1, 0};
  p.runtime_n = rt_sources_ok(N);
  p.loss = (fast && K <= 16)           ? LossRoute::Tuned
           : (K > 16 || p.runtime_n)   ? LossRoute::WideBasis
                                       : LossRoute::Generic;
  p.loss_byproduct = p.loss == LossRoute::Tuned && p.fm_id != 1;
  p.loss_slots = p.loss_byproduct ? tuned_basis_loss_slots(B, N, F, T) : 0;
  p.logdet_slots = p.loss_byproduct ? (small ? (F + 15) / 16 : 1) : 0;
  p.cov_matrix_core = N > 4 && wide_weighted_cov_ok(N, N, F, T, SSSPY_WEIGHT_BIN_FRAME);
  p.cov_tuned = fast;
  p.power_once = p.nmf == NmfRoute::Grouped || p.nmf == NmfRoute::WideBasis;
  p.ip1_latency = small;
  p.weights_buf = N > 4 || wide;
  p.dense_buf = wide;
  p.summary = p.runtime_n                      ? SSSPY_ROUTE_RUNTIME_N
              : p.nmf == NmfRoute::Grouped     ? SSSPY_ROUTE_GROUPED
              : small                          ? SSSPY_ROUTE_LATENCY
              : p.nmf == NmfRoute::WideBasis   ? SSSPY_ROUTE_WIDE_BASIS
              : tuned                          ? SSSPY_ROUTE_THROUGHPUT
                                               : SSSPY_ROUTE_GENERIC;
  return p;
}

// The covariance pass of a call.  ysep: a separated spectrogram, or its power (that only picks the
// operand), is at hand; filter: W was given (without one, X is that spectrogram).  The weight kernels
// of the first three routes need |y|^2 unless the model is Gauss; RuntimeN has no kernel to fall to.
static inline CovRoute cov_route(const IlrmaPlan &p, bool ysep, bool filter) {
  const bool weights_ok = p.gauss || ysep || !filter;
  if (p.runtime_n) return CovRoute::RuntimeN;
  if (p.K > 32 && weights_ok) return CovRoute::WideBasis;  // weights + the shared operator
  if (p.cov_matrix_core && weights_ok) return CovRoute::MatrixCore;
  if (p.cov_tuned && (p.gauss || filter)) return CovRoute::Tuned;
  return CovRoute::Generic;
}

// --------------------------------------------------------------------- 4. scratch layout, sizes
// The workspace queries do not know the model: Gauss at domain 2 stands for "any model of the
// tuned path"; the routes the sizes name below are the same shapes for every model.
static inline IlrmaPlan shape_plan(int B, int N, int F, int T, int K) {
  return make_ilrma_plan(B, N, F, T, K, 2.0, SSSPY_SOURCE_GAUSS);
}

// scratch of the deterministic loss sums: the larger of what the tuned kernels (by-product of the
// basis pass, loss pass), the generic and the run-time-N loss kernels need.  The wide-basis loss
// route (the same shapes for every model) parks one slot per 64 x 64 tile of every source and, when
// a filter is given, |W x|^2 (B N F T doubles) -- only then (round 4 added both terms for every
// shape: 2.1 GB idle at the headline batch, twice)
static inline size_t loss_slots_bytes(const IlrmaPlan &p, int B, int F, int T, bool with_filter) {
  const int N = p.N;
  const size_t a = generic_loss_ws_bytes(B, N, F), b = tuned_loss_ws_bytes(B, N, F);
  size_t c = p.runtime_n ? rt_ilrma_loss_ws_bytes(B, N, F) : 0;
  if (p.loss == LossRoute::WideBasis) {
    const size_t g = align256(wb_loss_ws_bytes(B, N, F, T)) +
                     (with_filter ? align256((size_t)B * N * F * T * sizeof(double)) : 0);
    c = c > g ? c : g;
  }
  return align256(a > b ? (a > c ? a : c) : (b > c ? b : c));
}

// One scratch layout for every ILRMA entry point: callers pass the same buffer everywhere.
struct IlrmaWs {
  size_t act_part, btmp, qbuf, psi, lslots, bpart, upart, praw, ybuf, wbuf, gb, gnd, total;
};
static inline size_t qbuf_bytes(int B, int N, int F) {
  return align256((size_t)B * F * N * sizeof(double));
}
static inline IlrmaWs ilrma_ws(int B, int N, int F, int T, int K) {
  const IlrmaPlan p = shape_plan(B, N, F, T, K);
  const size_t bnft = (size_t)B * N * F * T * sizeof(double);
  IlrmaWs w;
  size_t off = 0;
  w.act_part = off;  // partial sums of the activation chunks, or the latency kernel's
  const size_t ap = p.act_latency ? small_scratch(B, N, F, T, K) : 0;
  const size_t base = (size_t)B * p.act_chunks * N * 2 * K * T * sizeof(double);
  off += align256(base > ap ? base : ap);
  w.btmp = off;  // the new basis of an out-of-place update
  off += p.basis_out_of_place ? align256((size_t)B * N * F * K * sizeof(double)) : 0;
  w.qbuf = off;
  off += qbuf_bytes(B, N, F);
  w.psi = off;
  off += align256((size_t)B * N * sizeof(double));
  w.lslots = off;  // per-wave shares of a loss, folded in a fixed order (no fp64 atomics)
  off += loss_slots_bytes(p, B, F, T, true);
  // bin-major tuned kernels (basis, covariance): partial sums of the at most 1024 split blocks of the
  // closing scheduling rounds (TailPlan), in groups of at most 4 sources (the variants of
  // 16 < n_basis <= 64: at most 256 split blocks, each leaving one 16-k record per k tile -- up to 4)
  w.bpart = off;
  off += align256((size_t)1024 * (N < 4 ? N : 4) * 64 * 16 * 2 * sizeof(double));
  w.upart = off;
  off += N <= 4 ? align256((size_t)1024 * 64 * N * N * N * 2 * sizeof(double)) : 0;
  w.praw = off;  // (num, den) basis sums of the partitioned updates
  off += align256((size_t)B * N * F * K * 2 * sizeof(double));
  w.ybuf = off;  // |W x|^2 or y = W x of the grouped and wide-basis NMF routes
  off += p.weights_buf ? align256(2 * bnft) : 0;
  w.wbuf = off;  // covariance weights varphi (B, N, F, T); a of the wide-basis NMF route
  off += p.weights_buf ? align256(bnft) : 0;
  w.gb = off;    // wide-basis NMF route: b = 1 / R (B, N, F, T)
  off += p.dense_buf ? align256(bnft) : 0;
  w.gnd = off;   // wide-basis NMF route: (num, den) of the products
  off += p.dense_buf ? align256((size_t)2 * B * N * (F > T ? F : T) * K * sizeof(double)) : 0;
  w.total = off;
  return w;
}

}  // namespace ssspy
