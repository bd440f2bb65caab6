// The launch plan of the GaussMNMF entry points (gmnmf_kernels.hip): which kernel form every pass of
// a call takes, how its launches are cut, how much LDS they ask for and where the pieces of the
// workspace lie, as a function of (B, N, M, F, T, K) and `partitioning` alone.  make_gmnmf_plan() is
// the only place these decisions are taken: ssspy_gmnmf_update / _loss / _separate build the plan once
// per call and their launch code reads it, ssspy_gmnmf_workspace_bytes returns its `ws.total` and
// ssspy_gmnmf_route() projects it (a few dozen integer operations: host time far below a launch).
// Host only; launches nothing and touches no device state.
#pragma once

#include <climits>

#include "common.hpp"

namespace ssspy {

// gmnmf_rows.hip: the 8-lane spatial update (7 and 8 channels)
bool gmnmf_spatial_update_rows_wanted(int M);

constexpr int GM_NMAX = SSSPY_MAX_SOURCES;
// 9..16 sources: the per-point kernels take the source bound NX as a template parameter, GM_NMAX
// (every shape up to 8 sources) or GM_NWIDE (only when N > 8)
constexpr int GM_NWIDE = SSSPY_RT_MAX_SOURCES;
static_assert(GM_NWIDE == 2 * GM_NMAX, "the wide forms walk the sources in two groups of GM_NMAX");

constexpr int GM_PB = 64;             // points per chunk (= block size of k_gmnmf_spatial_acc)
constexpr int GM_POINT_BLOCK = 128;   // points per block of the traces / loss / separate kernels
constexpr int GM_MATRIX_BLOCK = 64;   // matrices per block of the spatial update kernels
constexpr int GMB_LDS = 4096;         // activation values k_gmnmf_basis stages at a time (32 KB)
constexpr int GMB_REG_FRAMES = 512;   // frames up to which it keeps a row of A / Bt in registers
constexpr int GM_ACT_KSLAB = 8;       // basis indices per launch of k_gmnmf_activation_sums
constexpr int GM_SPLIT_FROM = 4;      // channels from which the two matrices of a point take turns
                                      // in the LDS rows of k_gmnmf_spatial_acc_p
constexpr int GSU_LD = 65;            // k_gmnmf_spatial_update_p: lanes per staged entry + 1 (the
                                      // transposing copies hit distinct banks)
constexpr size_t GM_LDS_MAX = 160 * 1024;        // LDS a workgroup may take on gfx950
constexpr size_t GM_LDS_DEFAULT = 48 * 1024;     // dynamic LDS a kernel gets without the attribute

// source slots of the point kernels and of the packed spatial parts Hq
static inline int gm_source_slots(int N) { return N > GM_NMAX ? GM_NWIDE : GM_NMAX; }

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// byte offsets into the workspace of ssspy_gmnmf_update
struct GmnmfWs {
  size_t a, bt, pq, vacc, teff, vrep, raw, vslabs, flags, hq, total;
};

enum class GmSpatialForm { Literal = 0, Packed = 1, Rows8 = 2 };
enum class GmBasisForm { Registers = 0, LdsTile = 1, Memory = 2 };

struct GmnmfPlan {
  // SSSPY_OK, or the status the entry points return for this shape before they touch anything
  int status;
  const char *why;
  // ---- per-point kernels (traces, loss, separate, spatial sums)
  // 4..8 channels: the packed *_p kernels run first and the full-storage kernels of the same name
  // redo the flagged blocks; 2 and 3 channels keep the full-storage kernels alone (nothing spills
  // there and the packed route's extra launches -- packing, the flag-gated repair kernels -- cost
  // 10 % of a 0.15-0.25 ms iteration)
  bool packed;
  int nx;             // source slots of the point kernels and of Hq: GM_NMAX, or GM_NWIDE above 8
  bool wide;          // nx == GM_NWIDE: two groups of 8 sources, lambda_n formed again
  int trace_sources;  // sources k_gmnmf_traces_p is compiled for: 4, 8, or 0 (not packed)
  int acc_sources;    // sources per pass of k_gmnmf_spatial_acc (gm_acc_sources)
  GmSpatialForm spatial_form;
  // ---- k_gmnmf_basis
  GmBasisForm basis_form;
  int basis_kc;   // basis indices staged at a time (LDS forms), 0 from memory
  int basis_bpw;  // bins per wave, 1..16
  // ---- activation sums
  int act_chunks;          // bin chunks (slabs folded in order), 1..16
  int act_bins_per_chunk;  // ceil(F / chunks): trailing chunks may hold fewer bins, or none
  int act_kslabs;          // launches of GM_ACT_KSLAB basis indices
  // ---- dynamic LDS
  size_t bin_lds;     // traces / loss / separate: the bin's N spatial matrices and N basis rows
  size_t acc_lds;     // k_gmnmf_spatial_acc: bin_lds and a row per frame of the chunk
  size_t acc_p_lds;   // k_gmnmf_spatial_acc_p: 64 rows of gm_acc_p_row() doubles (0: not packed)
  size_t update_p_lds;  // k_gmnmf_spatial_update_p: M M staged entries of GSU_LD lanes (0: other forms)
  size_t latent_lds;  // k_gm_part_latent: N K doubles (0 without partitioning)
  // the LATENT step takes this shape (the latent variables of all sources sit in the LDS of one
  // workgroup: n_basis up to SSSPY_MAX_PARTITION_BASIS); the other steps do not depend on it
  bool latent_ok;
  // ---- flag words
  long long point_blocks;   // ceil(T / 128) F B
  long long matrix_blocks;  // ceil(B N F / 64)
  size_t loss_flags_offset;  // byte offset of the flag words in the loss workspace
  size_t loss_ws_total;
  GmnmfWs ws;
};

// bins per wave of k_gmnmf_basis: up to 16, fewer while that leaves the launch under ~2048 workgroups
static inline int gmb_bins_per_wave(int B, int N, int F) {
  const long long rows = (long long)B * N * F;
  long long bpw = rows / (4 * 2048);
  if (bpw < 1) bpw = 1;
  if (bpw > 16) bpw = 16;
  return (int)bpw;
}

// bin chunks of the activation sums: enough blocks for the chip at small batches, at most 16
static inline int gm_act_chunks(int B, int N, int F, int T) {
  const long long blocks0 = (long long)((T + 63) / 64) * N * B;
  long long want = (1024 + blocks0 - 1) / blocks0;
  if (want > 16) want = 16;
  if (want > (F + 7) / 8) want = (F + 7) / 8;  // at least 8 bins per chunk
  return want < 1 ? 1 : (int)want;
}

// doubles per point of k_gmnmf_spatial_acc_p in LDS: the value slots (both packed matrices, or from
// GM_SPLIT_FROM channels one at a time, padded to even), nx weights, one more (odd rows)
constexpr int gm_acc_p_values(int M) { return M >= GM_SPLIT_FROM ? ((M * M + 1) & ~1) : 2 * M * M; }
constexpr int gm_acc_p_row(int M, int nx) { return gm_acc_p_values(M) + nx + 1; }

// the workspace of ssspy_gmnmf_loss: the loss slots, then one flag per block (packed path)
struct GmnmfLossWs {
  size_t flags, total;
};
static inline GmnmfLossWs gmnmf_loss_ws(int B, int F, int T) {
  const int tb = (T + GM_POINT_BLOCK - 1) / GM_POINT_BLOCK;
  GmnmfLossWs w;
  w.flags = align256(scalar_slots_bytes(B, tb * F));
  w.total = w.flags + align256((size_t)tb * F * B * sizeof(int));
  return w;
}

static inline size_t gm_bin_smem(int N, int M, int K) {
  return (size_t)N * M * M * sizeof(c128) + (size_t)(((size_t)N * K + 1) & ~(size_t)1) * sizeof(double);
}

static inline GmnmfWs gmnmf_ws(int B, int N, int M, int F, int T, int K, int nx, int chunks) {
  GmnmfWs w;
  size_t off = 0;
  w.a = off;
  off += align256((size_t)B * N * F * T * sizeof(double));
  w.bt = off;
  off += align256((size_t)B * N * F * T * sizeof(double));
  w.pq = off;  // packed Hermitian sums of the spatial update
  off += align256((size_t)B * N * F * M * M * 2 * sizeof(double));
  w.vacc = off;  // activation sums (num, den)
  off += align256((size_t)B * N * 2 * K * T * sizeof(double));
  w.teff = off;  // partitioning: expanded pair and the (num, den) basis sums
  off += align256((size_t)B * N * F * K * sizeof(double));
  w.vrep = off;
  off += align256((size_t)B * N * K * T * sizeof(double));
  w.raw = off;
  off += align256((size_t)B * N * F * K * 2 * sizeof(double));
  w.vslabs = off;  // per-chunk slabs of the activation sums + the scratch of their fold
  {
    const long long vtotal = 2ll * B * N * K * T;
    off += chunks > 1 ? align256((size_t)chunks * vtotal * sizeof(double) +
                                 fold_scratch_bytes(vtotal, chunks))
                      : 0;
  }
  w.flags = off;  // one int per block of the per-point kernels: left the fast route (packed path)
  off += align256((size_t)((T + GM_POINT_BLOCK - 1) / GM_POINT_BLOCK) * F * B * sizeof(int));
  w.hq = off;  // packed symmetric parts of the spatial matrices, [b][i][nx][M M] (packed path)
  off += align256((size_t)B * F * nx * M * M * sizeof(double));
  w.total = off;
  return w;
}

// `partitioning`: the caller passes latent variables (the LATENT step keeps N K doubles in LDS)
static inline GmnmfPlan make_gmnmf_plan(int B, int N, int M, int F, int T, int K, bool partitioning) {
  GmnmfPlan p{};
  p.status = SSSPY_OK;
  p.why = "";
  auto reject = [&](int code, const char *msg) {
    p.status = code;
    p.why = msg;
    return p;
  };
  if (!(B > 0 && F > 0 && T > 0)) return reject(SSSPY_ERR_BADARG, "GaussMNMF: bad shape");
  if (N < 1) return reject(SSSPY_ERR_BADARG, "GaussMNMF: n_sources must be in [1, 16]");
  if (N > GM_NWIDE) return reject(SSSPY_ERR_UNSUPPORTED, "GaussMNMF: n_sources must be in [1, 16]");
  if (!(K >= 1 && K <= SSSPY_MAX_BASIS))
    return reject(SSSPY_ERR_BADARG, "GaussMNMF: n_basis must be in [1, 65536]");
  if (M < 2 || M > 8) return reject(SSSPY_ERR_UNSUPPORTED, "GaussMNMF: n_channels must be in [2, 8]");

  p.packed = M >= 4;
  p.wide = N > GM_NMAX;
  p.nx = gm_source_slots(N);
  p.trace_sources = !p.packed ? 0 : (N <= 4 ? 4 : 8);
  p.acc_sources = (M >= 4 && p.wide) ? GM_NMAX : p.nx;
  p.spatial_form = !p.packed                              ? GmSpatialForm::Literal
                   : gmnmf_spatial_update_rows_wanted(M) ? GmSpatialForm::Rows8
                                                         : GmSpatialForm::Packed;

  p.basis_form = T <= GMB_REG_FRAMES ? GmBasisForm::Registers
                 : T <= GMB_LDS      ? GmBasisForm::LdsTile
                                     : GmBasisForm::Memory;
  p.basis_kc = T <= GMB_LDS ? GMB_LDS / T : 0;
  p.basis_bpw = gmb_bins_per_wave(B, N, F);

  p.act_chunks = gm_act_chunks(B, N, F, T);
  p.act_bins_per_chunk = (F + p.act_chunks - 1) / p.act_chunks;
  p.act_kslabs = (K + GM_ACT_KSLAB - 1) / GM_ACT_KSLAB;

  // The full-storage kernels stage the bin's N spatial matrices and N basis rows in LDS; the spatial
  // sums add a row per frame of the chunk (k_gmnmf_spatial_acc).  All of it must fit the 160 KB of a
  // workgroup -- at any source count: n_basis is bounded by that, not by SSSPY_MAX_BASIS alone.
  p.bin_lds = gm_bin_smem(N, M, K);
  p.acc_lds = p.bin_lds + (size_t)GM_PB * (2 * M * M + p.acc_sources) * sizeof(double);
  p.acc_p_lds = p.packed ? (size_t)GM_PB * gm_acc_p_row(M, p.nx) * sizeof(double) : 0;
  p.update_p_lds = p.spatial_form == GmSpatialForm::Packed ? (size_t)M * M * GSU_LD * sizeof(c128) : 0;
  p.latent_lds = partitioning ? (size_t)N * K * sizeof(double) : 0;
  if (p.acc_lds > GM_LDS_MAX)
    return reject(SSSPY_ERR_UNSUPPORTED,
                  "GaussMNMF: n_basis is bounded by the 160 KB of LDS of a workgroup (the bin's "
                  "spatial matrices and basis rows)");
  p.latent_ok = partitioning && K <= SSSPY_MAX_PARTITION_BASIS;

  const int tb = (T + GM_POINT_BLOCK - 1) / GM_POINT_BLOCK;
  p.point_blocks = (long long)tb * F * B;
  p.matrix_blocks = ((long long)B * N * F + GM_MATRIX_BLOCK - 1) / GM_MATRIX_BLOCK;
  const GmnmfLossWs lw = gmnmf_loss_ws(B, F, T);
  p.loss_flags_offset = lw.flags;
  p.loss_ws_total = lw.total;
  p.ws = gmnmf_ws(B, N, M, F, T, K, p.nx, p.act_chunks);
  return p;
}

// a size as a plan int: -1 when it does not fit one
static inline int gm_plan_int(unsigned long long v) { return v > (unsigned long long)INT_MAX ? -1 : (int)v; }

}  // namespace ssspy
