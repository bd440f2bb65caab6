// The launch plan of the FastGaussMNMF entry points (mnmf_api.hip) and of the per-N launchers of the
// tiled kernels (mnmf_kernels.hip): which kernel form every pass of a call takes, as a function of
// (B, N, M, F, T, K) alone.  make_mnmf_plan() and the workspace size helpers of mnmf_api.hip are the
// only callers of the predicates below.  ssspy_fastmnmf_update builds the plan once per call, branches
// on its family and hands it to its step helpers; the other entry points build it where they branch.
// The per-N launchers keep their (B, M, F, T, K) signatures and rebuild the same plan from them (a
// few dozen integer operations and two tail-plan searches of at most 16 candidates: host time far
// below a launch), so what they launch and what ssspy_fastmnmf_route() reports are one function of
// the shape.  Host only; validates nothing.  The table of routes is in DESIGN.md, section 4.
#pragma once

#include <cstdlib>

#include "common.hpp"
#include "tail_plan.hpp"

namespace ssspy {

bool ip1_small_shape(int B, int F, int N);  // spatial_kernels.hip: IP1's latency form
bool fmnmf_rt_shape(int N, int M);          // fmnmf_rt.hip: 9..16 channels or sources

#ifndef SSSPY_MNMF_PBASIS_WAVES
#define SSSPY_MNMF_PBASIS_WAVES 2
#endif
constexpr int PBASIS_WAVES = SSSPY_MNMF_PBASIS_WAVES;  // waves per SIMD of the P_READ basis pass

// ------------------------------------------------------------------------------- 1. predicates
// the MFMA-tile kernels (mnmf_kernels.hip) are compiled for 2..4 sources and channels
static inline bool mnmf_tiled(int N, int M) { return N >= 2 && N <= 4 && M >= 2 && M <= 4; }

// The bin-split variants run on the two-level schedule of tail_plan.hpp: whole rounds of 512
// workgroups unsplit, the remainder (or a small batch) split along the frames.
static inline bool mnmf_fast_ok(int B, int F, int T, int K) {
  static const bool disabled = std::getenv("SSSPY_AMD_NO_FAST") != nullptr;
  // one mixture must fit a 32-bit buffer descriptor (up to 4 channels of complex128)
  return !disabled && K <= 16 && (long long)4 * F * T * 16 < (1ll << 32);
}

// number of bin chunks the activation pass splits into (partials are summed by the finalize kernel)
static inline int mnmf_chunks(int B, int F, int T, int K) {
  const long long blocks0 = (long long)B * ((T + 63) / 64) * ((K + 15) / 16);
  const int ntiles = (F + 15) / 16;
  long long want = (512 + blocks0 - 1) / blocks0;
  if (want < 1) want = 1;
  if (want > 16) want = 16;
  if (want > ntiles) want = ntiles;
  return (int)want;
}

// ---------------------------------------------------------------------------------- 2. the plan
enum class MnmfFamily { None = -1, Tiled = 0, Generic = 1, Runtime = 2 };

struct MnmfPlan {
  MnmfFamily family;  // Tiled: mnmf_kernels.hip; Generic: fmnmf_generic.hip; Runtime: fmnmf_rt.hip
  // ---- the rest describes the Tiled family (false / 0 / {0, 0, 1, 0} elsewhere)
  bool fast;  // the throughput forms (k_mnmf_binmajor_*, k_mnmf_activation_fast) of the basis,
              // activation, covariance and spatial passes; false: k_mnmf_*<M, KSMALL>
  bool ksmall;           // n_basis <= 16: KSMALL = true of those kernels and of the loss pass
  bool basis_via_copy;   // n_basis > 16: the basis pass writes btmp and the result is copied back
  // the LDS-DMA form of the two x-reading passes (k_mnmf_binmajor_glds): whole tiles of frames (the
  // spatial pass takes it only when it writes the hand-over)
  bool glds;
  // k-slabs of 4 the throughput instances carry: 2 (n_basis <= 8), 4 (9..16), 0.  At 2 the covariance
  // pass keeps private activation tiles per wave (the barrier-free form of k_mnmf_binmajor_glds).
  // Measured (benchmarks/tools/mnmf_steps.py, configs[3] shape): the covariance pass gains at every
  // batch (32 mixtures: 267 -> 253 us, 128: 964 -> 908); the spatial pass, bound by its read + write
  // stream, does not (401 -> 400, 1259 -> 1309) -- so only the covariance pass takes it.  (The A / B
  // switches of round 5 -- private tiles in both passes, |Q x|^2 stores transposed through LDS,
  // register-fed passes at tile-aligned frame counts -- went in round 6 with their instantiations.)
  int kq;
  bool handover;  // the |Q x|^2 hand-over (P, pscale) is taken by the passes of this shape
  // these kernels hold one workgroup per CU (x prefetch in registers, > 256 VGPR + AGPR): 256 slots;
  // two workgroups per CU with the hand-over (no x tiles, no Q in registers): the P_READ basis and
  // loss passes
  TailPlan tail, tail_handover;
  int act_chunks;  // bin chunks of the activation pass
  bool ip1_small;  // IP1's latency form is offered the partial covariance records
  bool all_split;  // every item of `tail` is split: a following kernel may fold the records itself
  int loss_slots;    // raw shares per mixture of the hand-over loss (0: no hand-over)
  int logdet_slots;  // shares per mixture of the deferred log-determinant
};

static inline MnmfPlan make_mnmf_plan(int B, int N, int M, int F, int T, int K) {
  MnmfPlan p;
  p.family = fmnmf_rt_shape(N, M)                                           ? MnmfFamily::Runtime
             : mnmf_tiled(N, M)                                             ? MnmfFamily::Tiled
             : (N >= 1 && N <= SSSPY_MAX_SOURCES && M >= 2 && M <= SSSPY_MAX_SOURCES)
                 ? MnmfFamily::Generic
                 : MnmfFamily::None;
  const bool tiled = p.family == MnmfFamily::Tiled;
  p.fast = tiled && mnmf_fast_ok(B, F, T, K);
  p.ksmall = tiled && K <= 16;
  p.basis_via_copy = tiled && K > 16;
  p.glds = p.fast && T % 16 == 0;
  p.kq = !tiled ? 0 : (K <= 8 ? 2 : (K <= 16 ? 4 : 0));
  p.handover = p.fast && T % 2 == 0;
  const TailPlan none{0, 0, 1, 0};
  p.tail = p.fast ? make_tail_plan(B, (F + 63) / 64, (T + 15) / 16, 256) : none;
  p.tail_handover =
      p.handover ? make_tail_plan(B, (F + 63) / 64, (T + 15) / 16, 256 * PBASIS_WAVES) : none;
  p.act_chunks = mnmf_chunks(B, F, T, K);
  p.ip1_small = tiled && ip1_small_shape(B, F, M);
  p.all_split = p.fast && p.tail.full == 0 && p.tail.tail > 0;
  p.loss_slots = p.handover ? p.tail_handover.groups *
                                  (p.tail_handover.split > 1 ? p.tail_handover.split : 1) * 4
                            : 0;
  p.logdet_slots = p.ip1_small ? (F + 15) / 16 : 1;
  return p;
}

}  // namespace ssspy
