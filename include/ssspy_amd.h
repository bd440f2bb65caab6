/*
 * ssspy_amd.h -- C ABI of the MI355X (gfx950) hot-path library libssspy_amd.so
 *
 * Drop-in boundary for the iterative frequency-domain demixing path of
 * tky823/ssspy v0.2.0.  The reference has no FFI layer:
 * the "operators" below are the NumPy expression groups inside the reference's
 * separator methods, and each entry point cites the reference lines it replaces.
 *
 * Conventions
 *  - every array argument is a DEVICE pointer to C-contiguous fp64 / complex128
 *    data (complex128 = two doubles, re then im, as numpy.complex128);
 *  - shapes carry a leading batch axis B of independent mixtures; the reference
 *    shapes follow it unchanged, e.g. X is (B, N, F, T), W is (B, F, N, N),
 *    basis (B, N, F, K), activation (B, N, K, T);
 *    N = n_sources = n_channels, F = n_bins, T = n_frames, K = n_basis;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); every
 *    call only enqueues work and returns; nothing here synchronises;
 *  - the callee never allocates or frees device memory: scratch is passed in
 *    (`*_workspace_bytes` tells how much) and outputs are caller-allocated;
 *  - return value: 0 on success, an SSSPY_ERR_* code otherwise
 *    (ssspy_last_error() gives the message); no C++ exception crosses the ABI;
 *  - singular per-bin systems (reference: numpy.linalg.LinAlgError from
 *    np.linalg.solve / inv) are counted into the caller's `int *info` device
 *    word; the host reads it when it next synchronises.
 *  - flooring (reference: ssspy/special/flooring.py:6-18) is named by
 *    (floor_kind, floor_eps): NONE = identity, MAX = max(x, eps), ADD = x + eps.
 */
#ifndef SSSPY_AMD_H
#define SSSPY_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SSSPY_OK = 0,
  SSSPY_ERR_BADARG = 1,      /* shape / enum outside what the kernels support */
  SSSPY_ERR_HIP = 2,         /* a HIP runtime call failed */
  SSSPY_ERR_UNSUPPORTED = 3, /* valid reference configuration not built here */
  SSSPY_ERR_INTERNAL = 4,    /* an invariant of the library itself was violated (a bug) */
};

enum { SSSPY_FLOOR_NONE = 0, SSSPY_FLOOR_MAX = 1, SSSPY_FLOOR_ADD = 2 };

/* weight layouts accepted by ssspy_weighted_covariance */
enum {
  SSSPY_WEIGHT_UNIT = 0,       /* weight == 1, one weight set                    */
  SSSPY_WEIGHT_FRAME = 1,      /* weight (B, S, T): broadcast over bins (AuxIVA) */
  SSSPY_WEIGHT_BIN_FRAME = 2,  /* weight (B, S, F, T)                            */
};

/* contrast functions of AuxIVA (reference: iva.py:3093-3115, :3256-3289) */
enum {
  SSSPY_CONTRAST_LAPLACE = 0,
  SSSPY_CONTRAST_GAUSS = 1,       /* refreshes variance = r2 / F, then G' = 2r / variance  */
  SSSPY_CONTRAST_GAUSS_FIXED = 2, /* uses the given variance unchanged (AuxGaussIVA IP2)   */
};

/* source models of ILRMA (reference classes GaussILRMA / TILRMA / GGDILRMA); `model_param` is
 * unused, the degree of freedom nu, or the shape beta respectively */
enum { SSSPY_SOURCE_GAUSS = 0, SSSPY_SOURCE_T = 1, SSSPY_SOURCE_GGD = 2 };
/* OR-ed into `source_model`: source_algorithm="ME" -- the same numerator / denominator sums with
 * exponent 1 (domain must be 2; Gauss and t models; ssspy/bss/ilrma.py:1249-1401, :2659-2830) */
enum { SSSPY_SOURCE_ME = 0x100 };

#define SSSPY_MAX_SOURCES 8 /* kernels compiled per source count (everything in registers) */
/* Above that, up to SSSPY_RT_MAX_SOURCES, the shared operators, the AuxIVA entry points and the ILRMA
 * iteration on the Gauss model's tuned passes run with the source count at run time (wide_n.hip:
 * correct, not tuned; the reference has no limit: ssspy/bss/ilrma.py:180, iva.py:152), IPA included
 * (ssspy_ipa_sweep, ipa_rt.hip, round 6), and so do the Hermitian operators / ssspy_solve (to
 * 16 x 16) and the standalone ssspy_lqpqm2 (to dimension 15; hermitian_rt.hip).  The
 * ssspy_fastmnmf_* entry points take n_channels in [2, 16] and n_sources in [1, 16] (9..16 of either
 * on the run-time forms of fmnmf_rt.hip; SSSPY_ERR_UNSUPPORTED above 16).  The ssspy_gmnmf_* entry
 * points take n_sources in [1, 16] at n_channels 2..8 (9..16 sources on the 16-source instantiations
 * of gmnmf_kernels.hip; SSSPY_ERR_UNSUPPORTED above 16).  The ssspy_ilrma_partition_* entry points
 * (partitioning=True) stay at SSSPY_MAX_SOURCES (SSSPY_ERR_UNSUPPORTED above). */
#define SSSPY_RT_MAX_SOURCES 16
/* n_basis: the kernels walk any number of bases (dense products above 32; checked against the
 * oracle at 1500 and 3000); the bound only keeps 32-bit index arithmetic safe.  Up to round 5: 1024.
 * The ssspy_gmnmf_* entry points are bounded further by a workgroup's LDS (see there). */
#define SSSPY_MAX_BASIS 65536
#define SSSPY_MAX_PARTITION_BASIS 1024 /* partitioning=True: the latent update keeps N x n_basis in LDS */
#define SSSPY_MAX_PAIRS 128 /* every pair of 16 sources: 120 */

const char *ssspy_amd_version(void);

/* Bumped whenever an entry point changes its argument list (a caller built against another header
 * would pass a stream where a workspace is expected): the binding compares it with the value of
 * the header it was written against and refuses to load a library that disagrees.
 * 2: round 6 (ssspy_covariance_congruence_tracked added; round-5 signatures of
 *    ssspy_ilrma_loss_workspace_bytes / ssspy_fastmnmf_diagonalizer_covariance).
 * 3: round 6 (ssspy_ilrma_ip1_update_loss_slots: `logdet` became slots,
 *    ssspy_ilrma_deferred_logdet_slots added).
 * 4: the ssspy_cacgmm_* entry points added.
 * 5: ssspy_fastmnmf_route added (additive: no existing argument list changed).
 * 6: ssspy_gmnmf_route added (additive).
 * 7: the FastIVA / FasterIVA entry points and ssspy_whitening_filter added (additive).
 * 8: the IPSDTA entry points and ssspy_matmul3 added (additive).
 * 9: the FDICA entry points added (additive).
 * 10: ssspy_prox_neg_logdet and the PDSBSS entry points added (additive).
 * 11: the HVA entry points added (additive). */
#define SSSPY_ABI_VERSION 11
int ssspy_abi_version(void);
const char *ssspy_last_error(void);

/* ------------------------------------------------------------------ shared operators */

/* Y[b,n,i,j] = sum_m W[b,i,n,m] X[b,m,i,j].   X (B,N,F,T), W (B,F,N,N), Y (B,N,F,T).
 * In-place (Y == X) is allowed: every (bin, frame) column is read before it is written.
 * replaces: ssspy/bss/ilrma.py:272-295, ssspy/bss/iva.py:171-194 (separate). */
int ssspy_separate(const void *X, const void *W, void *Y, int B, int N, int F, int T,
                   void *stream);

/* Cout (B,F,N,N) = G C G^H per bin (C != Cout): the covariance of y' = G y from the covariance of y.
 * ILRMA's ISS2 / IPA iterations keep C_i = (1/T) sum_j y y^H of the separated spectrogram alongside it
 * (round 5): the power normalisation psi_n^2 = mean_i g_n^H C_i g_n of the UPDATED spectrogram is
 * then known before y <- G y runs, its scale goes into the rows of G, and the two extra passes of
 * ssspy/bss/ilrma.py:412-444 (mean |y|^2, y / psi) disappear.  n_sources <= 16. */
int ssspy_covariance_congruence(const void *C, const void *G, void *Cout, int B, int F, int N,
                                void *stream);

/* The same with S matrices per bin sharing its G: C, Cout (B,F,S,N,N), G (B,F,N,N).  The statistics
 * of the separated spectrogram from those of the mixture, mean phi y y^H = W (mean phi x x^H) W^H:
 * the ISS / ISS2 / IPA iterations of ILRMA then read the mixture through the filters they imply
 * (ssspy_compose_filters) like the IP iterations do, and y <- G y (ssspy/bss/ilrma.py:1635-1908)
 * is carried out once, when the output is read. */
int ssspy_covariance_congruence_sets(const void *C, const void *G, void *Cout, int B, int F, int S,
                                     int N, void *stream);

/* ssspy_covariance_congruence_sets for 2..4 sources that also reports how far the product can round
 * from the sum over the samples it replaces.  The direct mean phi |y_r|^2 of
 * ssspy/bss/_update_spatial_model.py:176-194 / :283-395 adds positive terms; the product cancels,
 * eps * S_rr (S_rr = sum_kl |g_rk| |c_kl| |g_rl|) bounds its error and kappa_r = S_rr / (G C G^H)_rr
 * is the loss of relative accuracy of that entry (infinite for a non-positive diagonal).  S == N:
 * set n of a bin holds the statistics under source n's weights, which steer output row n only
 * (y_n <- y_n - (V_n[n,r] / V_n[r,r]) y_r), so kappa_n = max_r kappa_r of set n weighs with that
 * row's power p_n = g_n P g_n^H.  power (B,F,N,N): the unweighted covariance of the data G applies
 * to.  amplification: 2 x (B,2) device doubles, zero before the first launch; the launch with
 * `phase` adds { sum kappa_n^2 p_n, sum p_n } over bins and sets to amplification[phase & 1][b] and
 * clears the other half for the next launch (alternate phase).
 * eps * sqrt([b][0] / [b][1]) estimates the relative Frobenius error the route adds to mixture b's
 * spectrogram per iteration; the separators poll the slots without waiting and return to the
 * reference's on-Y iteration past their bound. */
int ssspy_covariance_congruence_tracked(const void *C, const void *G, void *Cout, int B, int F,
                                        int S, int N, const void *power, void *amplification,
                                        int phase, void *stream);

/* out (B,F,N,N) = G W per bin (out aliases neither): the filters implied by y <- G y with y = W x. */
int ssspy_compose_filters(const void *G, const void *W, void *out, int B, int F, int N,
                          void *stream);

/* U[b,i,s,a,c] = (1/T) sum_j weight[...] A[b,a,i,j] conj(A[b,c,i,j]), s < S.
 * A (B,N,F,T) complex, U (B,F,S,N,N) complex, weight per `weight_kind`.
 * replaces: the (F,N,N,N,T) broadcast + mean of ssspy/bss/ilrma.py:1500-1505,
 * ssspy/bss/iva.py:1785-1791, ssspy/bss/mnmf.py:1504-1512. */
int ssspy_weighted_covariance(const void *A, const double *weight, int weight_kind, void *U,
                              int B, int N, int S, int F, int T, void *stream);

/* C[b,i,a,c] = (1/T) sum_j A[b,a,i,j] conj(Bm[b,c,i,j]).  A, Bm (B,N,F,T), C (B,F,N,N).  replaces the X Y^H / Y Y^H / X X^H products of
 * ssspy/algorithm/projection_back.py:104-110, ssspy/bss/ilrma.py:1941-1944,
 * ssspy/bss/iva.py:2182-2185 (up to the 1/T factor, which cancels there). */
int ssspy_cross_covariance(const void *A, const void *Bm, void *C, int B, int N, int F, int T,
                           void *stream);

/* One iterative-projection sweep, in place on W.  W (B,F,N,N), U (B,F,N,N,N).
 * `info` (device int, may be NULL) is incremented once per singular bin.
 * replaces: ssspy/bss/_update_spatial_model.py:17-78 (update_by_ip1, overwrite=True). */
int ssspy_update_by_ip1(void *W, const void *U, int B, int F, int N, int floor_kind,
                        double floor_eps, int *info, void *stream);

/* The same for a record_loss loop: the call also leaves sum_i log|det W_i| of the filters AS THEY
 * COME IN (the log-determinant term of the loss of the state the update starts from,
 * ssspy/bss/iva.py:200-222) as ssspy_update_by_ip1_logdet_slots() shares per mixture at
 * logdet[s * logdet_stride + b], to be added in slot order (ssspy_fold_scalar_slots): 1 where the
 * finished sums are stored, ceil(F / 16) for a handful of mixtures of up to 4 sources, where the
 * latency form of the kernel reads the filters anyway (shares the call does not write stay as the
 * caller zeroed them). */
int ssspy_update_by_ip1_logdet_slots(int B, int F, int N);
int ssspy_update_by_ip1_logdet(void *W, const void *U, int B, int F, int N, int floor_kind,
                               double floor_eps, int *info, double *logdet,
                               long long logdet_stride, void *stream);

/* The same sweep one source at a time, for a flooring_fn that is an arbitrary Python callable (the
 * reference accepts any, ssspy/bss/ilrma.py:70-89) and so cannot run in a kernel: the solve of source
 * `source_idx` leaves the unnormalised row conj(w) in W and denom (B,F) = sqrt(max(Re(w^H U_n w), 0));
 * the caller applies its callable to denom and divides the row by the result.
 * replaces: ssspy/bss/_update_spatial_model.py:63-76 (one iteration of the source loop). */
int ssspy_ip1_source_solve(void *W, const void *U, double *denom, int source_idx, int B, int F,
                           int N, int *info, void *stream);
int ssspy_scale_filter_row(void *W, const double *denom, int source_idx, int B, int F, int N,
                           void *stream);

/* One iterative-source-steering sweep expressed on per-bin statistics:
 * given Vc[b,i,s] = (1/T) sum_j varphi_s y y^H (B,F,N,N,N) it runs the N rank-1
 * steps of the reference on the N x N matrices and returns the accumulated
 * transform G (B,F,N,N) such that Y_new[:,i,:] = G_i Y[:,i,:].
 * replaces: ssspy/bss/_update_spatial_model.py:146-194 (update_by_iss1). */
int ssspy_iss1_transform(const void *Vc, void *G, int B, int F, int N, int floor_kind,
                         double floor_eps, void *stream);

/* Pairwise iterative projection, in place on W (B,F,N,N).  `pairs` is a HOST array of 2*n_pairs
 * ints (m0,n0,m1,n1,...), walked in order inside the kernel.  pair_only == 0: U (B,F,N,N,N) holds
 * one covariance per source; pair_only != 0: U (B,F,2,N,N) holds the pair's own two covariances and
 * n_pairs must be 1 (the AuxIVA form, where the weights are recomputed for every pair).  Rows come out with the arbitrary
 * phase of the 2x2 eigenvectors (fixed by scale restoration).
 * replaces: ssspy/bss/_update_spatial_model.py:81-143 (update_by_ip2), :317-395 (one pair). */
int ssspy_update_by_ip2(void *W, const void *U, int pair_only, const int *pairs, int n_pairs, int B,
                        int F, int N, int floor_kind, double floor_eps, int *info, void *stream);

/* Pairwise iterative source steering on per-bin statistics Vc (B,F,N,N,N) (as ssspy_iss1_transform):
 * returns G (B,F,N,N) with Y_new[:,i,:] = G_i Y[:,i,:].
 * replaces: ssspy/bss/_update_spatial_model.py:197-314 (update_by_iss2). */
int ssspy_iss2_transform(const void *Vc, void *G, const int *pairs, int n_pairs, int B, int F,
                         int N, int floor_kind, double floor_eps, int *info, void *stream);

/* The pairwise updates for a flooring callable that cannot run in a kernel (the reference takes any
 * callable: ssspy/bss/_update_spatial_model.py:81-143, :197-314).  ONE pair per call, rows left
 * UNNORMALISED, denom (B, F, 2) f64 <- sqrt(max(h^H G h, 0)) of the pair's two members; the caller
 * applies its callable to each (n_bins,) slice on the host and divides the rows with
 * ssspy_scale_filter_row (IP2: rows pair[0], pair[1] of W; ISS2: the same rows of the transform G,
 * which `accumulate` continues from its current value instead of the identity). */
int ssspy_update_by_ip2_deferred(void *W, const void *U, int pair_only, const int *pair, int B,
                                 int F, int N, double *denom, int *info, void *stream);
int ssspy_iss2_transform_deferred(const void *Vc, void *G, const int *pair, int accumulate, int B,
                                  int F, int N, double *denom, int *info, void *stream);

/* Largest n_frames the fused ISS kernel holds in registers for N sources (0 if N unsupported). */
int ssspy_iss1_fused_max_frames(int N);

/* One whole update_by_iss1 sweep set, in place on Y (B,N,F,T): a bin's N x T slab stays in the
 * registers of one workgroup through the N rank-1 steps (one read + one write of Y).
 * weight: (B,N,T) for SSSPY_WEIGHT_FRAME, (B,N,F,T) for SSSPY_WEIGHT_BIN_FRAME.
 * r2_next (B,N,T), optional: receives sum_i |y_new|^2 -- the frame powers the next AuxIVA iteration
 * needs, saving its separate pass.  They are summed without atomics (every block leaves its bins' sums
 * in `workspace`, a second kernel adds them in block order), so the result -- and with it the
 * trajectory -- is the same on every run; `workspace` (ssspy_iss1_fused_workspace_bytes) is needed
 * with r2_next (and by the tracked form below).
 * replaces: ssspy/bss/_update_spatial_model.py:146-194 (update_by_iss1). */
size_t ssspy_iss1_fused_workspace_bytes(int B, int N, int F, int T);
int ssspy_iss1_fused(void *Y, const double *weight, int weight_kind, double *r2_next, int B, int N,
                     int F, int T, int floor_kind, double floor_eps, void *workspace,
                     size_t workspace_bytes, void *stream);

/* The same sweep set, also tracking the log-determinant of the demixing filter the ISS state never
 * forms: the sweep of source n multiplies W_i by (I - v e_n^T), det = d_in^(-1/2), so
 * logdet[b] += -1/2 sum_i sum_n log d_in (logdet: B doubles holding sum_i log|det W_i| of the Y
 * passed in; NOT zeroed by the call; the blocks' shares go through `workspace` and are added in
 * block order: no atomics).  Lets compute_loss() (ssspy/bss/iva.py:2177-2192) skip the
 * reconstruction of W from Y X^H -- two more passes per recorded loss. */
int ssspy_iss1_fused_tracked(void *Y, const double *weight, int weight_kind, double *r2_next, int B,
                             int N, int F, int T, int floor_kind, double floor_eps, double *logdet,
                             void *workspace, size_t workspace_bytes, void *stream);

/* W <- W * (W^-1)[ref,:]^T.  W (B,F,N,N) in place.  G (B,F,N,N), optional: receives
 * diag((W^-1)[ref, :]), the scales (projection-back normalisation needs them for the basis).
 * replaces: ssspy/algorithm/projection_back.py:87-99. */
int ssspy_projection_back_filter(void *W, void *G, int B, int F, int N, int reference_id, int *info,
                                 void *stream);

/* minimal distortion principle: G[b,i] = diag(conj(z_n)), z_n = sum_j y_n conj(x_ref) / sum_j |y_n|^2,
 * from YX = ssspy_cross_covariance(Y, X) and YY = ssspy_cross_covariance(Y, Y); apply with
 * ssspy_separate(Y, G).   replaces: ssspy/algorithm/minimal_distortion_principle.py:6-43. */
int ssspy_mdp_scale(const void *YX, const void *YY, void *G, int B, int F, int N, int reference_id,
                    void *stream);

/* basis[b,n,i,:] *= |G[b,i,n,n]|^domain, the basis side of normalization="projection_back".
 * replaces: ssspy/bss/ilrma.py:518-522. */
int ssspy_ilrma_scale_basis(double *basis, const void *G, int B, int N, int F, int K, double domain,
                            void *stream);

/* scale[b,i,n] = ((X Y^H)(Y Y^H)^-1)[ref, n] from XY (B,F,N,N) and YY (B,F,N,N);
 * G[b,i] = diag(scale) so that ssspy_separate(Y, G) applies it.
 * replaces: ssspy/algorithm/projection_back.py:100-121. */
int ssspy_projection_back_scale(const void *XY, const void *YY, void *G, int B, int F, int N,
                                int reference_id, int *info, void *stream);

/* W[b,i] = YX[b,i] (XX[b,i])^-1.   replaces: ssspy/bss/ilrma.py:1941-1944, iva.py:2182-2185 */
int ssspy_demix_from_covariance(const void *YX, const void *XX, void *W, int B, int F, int N,
                                int *info, void *stream);

/* out[b] = sum_i log|det W[b,i]|.   W (B,F,N,N), out (B) doubles.
 * replaces: np.linalg.slogdet at ssspy/bss/ilrma.py:534, iva.py:234, mnmf.py:1274. */
int ssspy_sum_logdet(const void *W, double *out, int B, int F, int N, void *stream);

/* out[i] = log|det W_i| of n matrices (n, N, N), 1 <= N <= 16: LU with partial pivoting, a lane per
 * matrix; -inf for an exactly singular matrix, as numpy.linalg.slogdet.  The per-bin values behind
 * compute_logdet (ssspy/bss/iva.py:224-236, ilrma.py:524-536) for a filter that is on the device.
 * (Added at SSSPY_ABI_VERSION 11 without a bump: no existing argument list changed.) */
int ssspy_logdet(const void *W, double *out, long long n, int N, void *stream);

/* ------------------------------------------------------------------ batched small linear algebra */
/* Device counterparts of ssspy.linalg / ssspy.special.psd: `n` independent matrices, one per lane.
 * Sizes up to 8 x 8 are instantiated per size; 9 x 9 .. SSSPY_RT_MAX_SOURCES (16) take the size at
 * run time (csrc/hermitian_rt.hip: correct, not tuned); larger ones are SSSPY_ERR_UNSUPPORTED. */

/* X = A^-1 B.  A (n,N,N), B (n,N,nrhs), X (n,N,nrhs) complex128; N <= 16; LU with partial pivoting.
 * replaces: ssspy/linalg/_solve.py:9-21 (np.linalg.solve). */
int ssspy_solve(const void *A, const void *Bm, void *X, long long n, int N, int nrhs, int *info,
                void *stream);

/* closed-form 2x2 inverse.  replaces: ssspy/linalg/inv.py:4-54 (inv2). */
int ssspy_inv2(const void *A, void *out, long long n, void *stream);

/* Hermitian eigen-decomposition (cyclic complex Jacobi) of the Hermitian part (A + A^H) / 2 at every
 * size: lamb (n,M) ascending, V (n,M,M) unit eigenvectors in columns (phase convention differs from
 * LAPACK; A V = V diag(lamb) holds).
 * M = 2 (and ssspy_eigh2 below): the eigenvectors carry the phases reference LAPACK's zheevd gives
 * them (zhetd2 + dlaev2, restated in csrc/eigh2.hpp) -- what np.linalg.eigh returns in the
 * reference's eigh2 and pairwise updates (ssspy/linalg/eigh.py:155-157, :198).
 * replaces: np.linalg.eigh at ssspy/linalg/eigh.py:77,157,198 and ssspy/special/psd.py:54. */
int ssspy_eigh(const void *A, double *lamb, void *V, long long n, int M, void *stream);

/* Hermitise, floor the eigenvalues, rebuild, Hermitise.  replaces: ssspy/special/psd.py:11-71. */
int ssspy_to_psd(const void *A, void *out, long long n, int M, int floor_kind, double floor_eps,
                 void *stream);
/* out = P diag(w) P^H, Hermitised when `hermitise`: the rebuild half of to_psd / invsqrtmh for an
 * eigenvalue map the kernels cannot run (any flooring callable: ssspy_eigh -> the callable on the
 * (n, M) eigenvalues on the host -> this).  P (n, M, M) c128, w (n, M) f64, any M.
 * replaces: ssspy/special/psd.py:54-69, ssspy/linalg/sqrtm.py:58-64. */
int ssspy_herm_rebuild(const void *P, const double *w, void *out, long long n, int M, int hermitise,
                       void *stream);

/* generalised 2x2 Hermitian eigenproblem via Cholesky of B; type 1: A z = l B z, 2: A B z = l z,
 * 3: B A z = l z.  lamb (n,2) ascending, Z (n,2,2).  `info` counts non-positive-definite B.
 * replaces: ssspy/linalg/eigh.py:84-207 (eigh2 / _eigh). */
int ssspy_eigh2(const void *A, const void *Bm, double *lamb, void *Z, long long n, int type,
                int *info, void *stream);

/* ------------------------------------------------------------------ GaussILRMA (IP1/ISS1, MM) */

/* Scratch (bytes) for the ILRMA entry points below: one buffer of this size serves all of them
 * (each uses its own region: bin-chunk partials of the activation pass, frame-chunk partials of
 * the basis / covariance passes for small batches, per-bin powers for the normalisation). */
size_t ssspy_ilrma_workspace_bytes(int B, int N, int F, int T, int K);

/* The ILRMA entry points take the source model as (source_model, model_param):
 *   GAUSS: numerator P/R^((p+2)/p), exponent p/(p+2), varphi = 1/R^(2/p)       (ilrma.py:582-1989)
 *   T    : numerator P/(R~ R), R~ = nu/(nu+2) R^(2/p) + 2/(nu+2) P, varphi = 1/R~  (:1992-3334)
 *   GGD  : numerator (beta/2) P^(beta/2)/R^((beta+p)/p), exponent p/(beta+p),
 *          varphi = 1/((2/beta) floor(P^((2-beta)/2)) R^(beta/p))                (:3337-4410)
 * with R = (T V)_nij, P = |y_nij|^2, p = domain. */

/* basis update: T <- floor(T * (sum_j V num / sum_j V/R)^expo).  y = W x, or y = X when W == NULL
 * (the ISS state passes the separated spectrogram).
 * replaces: ssspy/bss/ilrma.py:1051-1128, :2470-2521, :3745-3824 (update_basis_mm, no partitioning). */
int ssspy_ilrma_update_basis(const void *X, const void *W, double *basis, const double *activation,
                             int B, int N, int F, int T, int K, double domain, int source_model,
                             double model_param, int floor_kind, double floor_eps, void *workspace,
                             size_t workspace_bytes, void *stream);

/* activation update (sum over bins with the NEW basis).
 * replaces: ssspy/bss/ilrma.py:1130-1204, :2523-2600, :3826-3905 (update_activation_mm). */
int ssspy_ilrma_update_activation(const void *X, const void *W, const double *basis,
                                  double *activation, int B, int N, int F, int T, int K,
                                  double domain, int source_model, double model_param,
                                  int floor_kind, double floor_eps, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* U[b,i,n] = (1/T) sum_j varphi_nij x x^H  ->  U (B,F,N,N,N).  W is read only by the heavy-tailed
 * models (varphi depends on |w x|^2); the floor only by GGD.
 * replaces: ssspy/bss/ilrma.py:1494-1505, :2915-2942, :3990-4018 (weights + covariance broadcast). */
int ssspy_ilrma_weighted_covariance(const void *X, const void *W, const double *basis,
                                    const double *activation, void *U, int B, int N, int F, int T,
                                    int K, double domain, int source_model, double model_param,
                                    int floor_kind, double floor_eps, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* power normalisation from the static covariance C (B,F,N,N) = (1/T) sum_j x x^H:
 * psi_n = floor(sqrt(mean_i w_in^H C_i w_in)); W[:,n,:] /= psi_n; basis[n] /= psi_n^p.
 * replaces: ssspy/bss/ilrma.py:365-444 (normalize_by_power, demix-filter branch). */
int ssspy_ilrma_normalize_filter(void *W, const void *C, double *basis, int B, int N, int F, int K,
                                 double domain, int floor_kind, double floor_eps, void *workspace,
                                 size_t workspace_bytes, void *stream);

/* same for the ISS state: psi from |Y|^2 directly, Y /= psi, basis /= psi^p.
 * frame_power (B,N,T), optional: sum_i |y_nij|^2 of the CURRENT Y, as ssspy_iss1_fused leaves it in
 * r2_next -- saves the pass over Y that computes the power; NULL: computed here (one partial sum
 * per 16 bin rows, added in order: no atomics).  workspace: B * N * ceil(F / 16) doubles (B * N with
 * frame_power); the buffer of ssspy_ilrma_workspace_bytes is large enough.
 * replaces: ssspy/bss/ilrma.py:365-444 (normalize_by_power, demix_filter is None branch). */
int ssspy_ilrma_normalize_output(void *Y, double *basis, const double *frame_power, int B, int N,
                                 int F, int T, int K, double domain, int floor_kind,
                                 double floor_eps, void *workspace, size_t workspace_bytes,
                                 void *stream);

/* The same, also moving the tracked sum_i log|det W_i| of the ISS state (ssspy_iss1_fused_tracked):
 * dividing source n by psi_n divides row n of every implied filter, logdet[b] -= F sum_n log psi_n.
 * replaces: ssspy/bss/ilrma.py:365-444 (normalize_by_power) + the filter rebuild of :1946-1965. */
int ssspy_ilrma_normalize_output_tracked(void *Y, double *basis, const double *frame_power, int B,
                                         int N, int F, int T, int K, double domain, int floor_kind,
                                         double floor_eps, void *workspace, size_t workspace_bytes,
                                         double *logdet, void *stream);

/* varphi[b,n,i,j] (B,N,F,T) doubles for the ISS paths; Y (the separated spectrogram) is read only
 * by the heavy-tailed models.
 * replaces: ssspy/bss/ilrma.py:1690-1694, :3125-3143, :4202-4220. */
int ssspy_ilrma_iss_weight(const void *Y, const double *basis, const double *activation,
                           double *varphi, int B, int N, int F, int T, int K, double domain,
                           int source_model, double model_param, int floor_kind, double floor_eps,
                           void *stream);

/* The same from the POWER of the separated spectrogram, Ypow (B,N,F,T) f64 = |y|^2, instead of y.
 * Also the seam for a flooring callable the kernels do not know on GGD's weights (round 6): the
 * reference floors |y|^(2 - beta) per element (ssspy/bss/ilrma.py:3993-3995, :4123-4125); the
 * binding evaluates q = |y|^(2 - beta) and the callable on the host and hands in
 * Ypow = callable(q)^(2 / (2 - beta)) with SSSPY_FLOOR_NONE. */
int ssspy_ilrma_iss_weight_power(const double *Ypow, const double *basis, const double *activation,
                                 double *varphi, int B, int N, int F, int T, int K, double domain,
                                 int source_model, double model_param, int floor_kind,
                                 double floor_eps, void *stream);

/* out[b] = sum_{n,i} mean_j ( data term of the model + (2/p) log R ), y = W x (or x when
 * W == NULL); `out` (B doubles) is overwritten.  The caller adds -2 * ssspy_sum_logdet.
 * The per-workgroup shares are parked in `workspace` (ssspy_ilrma_loss_workspace_bytes for this
 * n_basis, with_filter = (W != NULL); the workspace of ssspy_ilrma_workspace_bytes is large enough
 * too) and added up in a fixed order:
 * no fp64 atomics, the same bits on every run.
 * replaces: ssspy/bss/ilrma.py:1946-1965, :3291-3310, :4367-4386. */
size_t ssspy_ilrma_loss_workspace_bytes(int B, int N, int F, int T, int K, int with_filter);
int ssspy_ilrma_loss_data(const void *X, const void *W, const double *basis,
                          const double *activation, double *out, int B, int N, int F, int T, int K,
                          double domain, int source_model, double model_param, void *workspace,
                          size_t workspace_bytes, void *stream);

/* One whole update_once() of an ILRMA with spatial_algorithm="IP1", source_algorithm="MM": basis,
 * activation, weighted covariance, IP1, power normalisation -- the launches the host would otherwise
 * issue one by one.  U (B,F,N,N,N) is caller-provided scratch.
 * replaces: ssspy/bss/ilrma.py:900-922 (and the TILRMA / GGDILRMA equivalents). */
int ssspy_ilrma_ip1_update(const void *X, const void *C, void *W, double *basis, double *activation,
                           void *U, int B, int N, int F, int T, int K, double domain,
                           int source_model, double model_param, int normalize, int floor_kind,
                           double floor_eps, void *workspace, size_t workspace_bytes, int *info,
                           void *stream);

/* The same update_once(), which also leaves the negative log-likelihood of the state AT ENTRY:
 * loss_data[b] (B doubles, overwritten) = the data term ssspy_ilrma_loss_data would give,
 * logdet[b] = ssspy_sum_logdet(W) before W is rewritten; loss = loss_data - 2 logdet.  The data term
 * is a by-product of the basis pass (which forms |y|^2 and R under the same parameters), so a loop
 * with record_loss=True costs three passes over X per iteration, not four: the loss after iteration t
 * comes out of iteration t + 1, and only the last one needs ssspy_ilrma_loss_data.  Returns
 * SSSPY_ERR_UNSUPPORTED (before touching any state) where the tuned kernels have no such
 * by-product: n_basis > 16, n_sources > 4, domains other than 1 and 2 (and domain 1 with a model
 * other than Gauss / MM), the Student-t model (its data term is not linear in the pass's
 * accumulators), and mixtures with n_bins * n_frames * 16 bytes >= 4 GiB.
 * replaces: ssspy/bss/base.py:68-77 around ssspy/bss/ilrma.py:900-922 and :1946-1965. */
/* 1 when ssspy_ilrma_ip1_update_deferred_loss has the by-product for this shape and model, else 0. */
int ssspy_ilrma_deferred_loss_supported(int N, int F, int T, int K, double domain,
                                        int source_model);
int ssspy_ilrma_ip1_update_deferred_loss(const void *X, const void *C, void *W, double *basis,
                                         double *activation, void *U, int B, int N, int F, int T,
                                         int K, double domain, int source_model, double model_param,
                                         int normalize, int floor_kind, double floor_eps,
                                         void *workspace, size_t workspace_bytes, int *info,
                                         double *loss_data, double *logdet, void *stream);

/* The same with the by-product left as RAW slots (round 5): slot s of mixture b at
 * slots[s * slot_stride + b], s < ssspy_ilrma_deferred_loss_slots() (0: no by-product for this shape).
 * A run of n_iter iterations allocates one zeroed array of slots x (n_iter + 1) B doubles, passes
 * slots + t B with slot_stride = (n_iter + 1) B in iteration t, and folds all iterations' slots in
 * slot order with one ssspy_fold_scalar_slots(slots, (n_iter + 1) B, n_slots, out, ...) at the end --
 * instead of a memset, a counter memset and a fold launch per iteration.
 * logdet (round 6) is laid out the same way: ssspy_ilrma_deferred_logdet_slots() shares per mixture
 * at logdet[s * slot_stride + b], to be folded in slot order like the data slots -- 1 where the
 * call leaves the finished sums (logdet[b]), ceil(F / 16) for a handful of mixtures, where the IP1
 * kernel of the latency path leaves the log-determinants of the filters it reads, per tile of 16
 * bins, instead of a dedicated one-block launch per iteration (0: no by-product for this shape). */
int ssspy_ilrma_deferred_loss_slots(int B, int N, int F, int T, int K, double domain,
                                    int source_model);
int ssspy_ilrma_deferred_logdet_slots(int B, int N, int F, int T, int K, double domain,
                                      int source_model);
int ssspy_ilrma_ip1_update_loss_slots(const void *X, const void *C, void *W, double *basis,
                                      double *activation, void *U, int B, int N, int F, int T,
                                      int K, double domain, int source_model, double model_param,
                                      int normalize, int floor_kind, double floor_eps,
                                      void *workspace, size_t workspace_bytes, int *info,
                                      double *slots, long long slot_stride, double *logdet,
                                      void *stream);
/* out[e] = sum over s < nslots of slots[s * total + e], e < total, in slot order (deterministic) */
size_t ssspy_fold_scalar_slots_workspace_bytes(long long total, int nslots);
int ssspy_fold_scalar_slots(const double *slots, long long total, int nslots, double *out,
                            void *workspace, size_t workspace_bytes, void *stream);

/* Which kernels the ILRMA passes above take for a shape and model (host only, launches nothing): for
 * tests and tools that must know which launcher branch a case exercises.  The value names the route
 * of the basis / activation updates, first match in this order:
 *   RUNTIME_N   more than SSSPY_MAX_SOURCES sources: covariance, IP1, normalisation and loss take the
 *               source count at run time (wide_n.hip); the NMF passes walk the sources in groups of
 *               the tuned kernels where the model has them, else as dense products
 *   GROUPED     5..8 sources on the tuned kernels in runs of 4 / 3 / 2 sources
 *   LATENCY     a handful of mixtures of 2..4 sources, n_basis <= 16 (ilrma_small.hip)
 *   WIDE_BASIS  dense products on the matrix cores (wide_basis.hip): n_basis >= 33
 *   THROUGHPUT  the tuned kernels of 2..4 sources (ilrma_fast.hip), n_basis <= 32
 *   GENERIC     the per-source-count kernels of any model (ilrma_kernels.hip)
 * (the basis update has no latency form: LATENCY shapes run the THROUGHPUT basis kernel.)
 * The value is a summary of the launch plan every pass obeys (csrc/ilrma_plan.hpp), not a pass's own
 * route: RUNTIME_N says that covariance, IP1, normalisation and loss run the run-time-N kernels; the
 * basis / activation updates of such a shape run GROUPED (n_basis <= 32, a model of the tuned
 * kernels) or WIDE_BASIS.  LATENCY covers the activation update, covariance fold, IP1 and
 * normalisation.  The loss pass has its own split: tuned to 16 bases, dense products above.
 * *act_chunks (may be NULL): the number of bin chunks the activation pass of the THROUGHPUT, GROUPED
 * and GENERIC routes folds (1: no partial sums).
 * basis_plan (may be NULL): three ints on the frame splits of the basis pass on the LATENCY and
 * THROUGHPUT routes -- work items (bin groups of 64 bins) that walk all frames and finish in place,
 * items whose frames are split, and the number of frame chunks of a split item (1: none is split;
 * 0, 0, 1 on the other routes).  Returns -1 for arguments the passes reject. */
enum {
  SSSPY_ROUTE_LATENCY = 0,
  SSSPY_ROUTE_THROUGHPUT = 1,
  SSSPY_ROUTE_GROUPED = 2,
  SSSPY_ROUTE_GENERIC = 3,
  SSSPY_ROUTE_WIDE_BASIS = 4,
  SSSPY_ROUTE_RUNTIME_N = 5,
};
int ssspy_ilrma_route(int B, int N, int F, int T, int K, double domain, int source_model,
                      int *act_chunks, int *basis_plan);

/* IPA (iterative projection with adjustment): a whole sweep on per-bin statistics (round 5; the
 * per-source entry point ssspy_ipa_transform of rounds 3-5 went in round 6 with its 81 kernel
 * instantiations).  n_sources in [2, 16]: a lane per bin up to 6 sources, a bin on 8 lanes at 7 / 8,
 * and above 8 a lane per bin with the source count at run time and its working set in scratch
 * memory (ipa_rt.hip, round 6: correct, not tuned).  Vc (B,F,N,N,N) = ssspy_weighted_covariance(Y,
 * weight) of the spectrogram BEFORE the sweep (overwritten: after source step s it holds
 * G_s Vc G_s^H, the covariances of the spectrogram the reference would have formed by then); G
 * (B,F,N,N) <- G_{N-1} ... G_0.  The caller applies ssspy_separate(Y, G) once: three passes over Y per
 * sweep (weights, covariance, separate) instead of 3 N.  The weights are those of the sweep's start
 * for every source, as in the reference (_update_spatial_model.py:436-445: varphi is an argument).
 * newton_ws: ssspy_ipa_sweep_newton_words(B, N) 64-bit words of scratch.  The reference's Newton loop
 * runs over all bins of a mixture at once and stops at the first step at which every bin has
 * converged (linalg/lqpqm.py:196-213); with the scratch the bins of a mixture vote and make exactly
 * as many steps (max_iter <= 62); with NULL every bin makes max_iter steps.  not_converged
 * (optional): incremented once per mixture whose bins had not all converged after max_iter steps
 * (the reference's UserWarning).  info: incremented per singular per-bin system.
 * replaces: ssspy/bss/_update_spatial_model.py:398-513 (update_by_ipa), linalg/lqpqm.py:13-352
 * (lqpqm2, solve_equation). */
int ssspy_ipa_sweep(void *Vc, void *G, int B, int F, int N, int normalization, int max_iter,
                    int floor_kind, double floor_eps, int *info, void *newton_ws,
                    int *not_converged, void *stream);
/* 64-bit words ssspy_ipa_sweep's newton_ws must hold: a vote word and an arrival counter per
 * (mixture, source step).  Up to 4 sources the sweep is ONE launch (round 6): a workgroup walks
 * the N source steps of its 64 bins and meets the mixture's other workgroups at every Newton vote
 * instead of ending the kernel there (4 launches per source step before). */
size_t ssspy_ipa_sweep_newton_words(int B, int N);
/* Development aid: how many of those in-kernel meetings gave up waiting since the library was
 * loaded (0 unless a launch is broken; synchronises).  -1: the query itself failed. */
int ssspy_debug_barrier_timeouts(void);

/* ---- partitioning (latent variables): basis (B,F,K), activation (B,K,T), latent (B,N,K) with
 * R_nij = sum_k z_nk t_ik v_kj (ssspy/bss/ilrma.py:297-327).  Every entry point above that takes
 * (basis, activation) runs unchanged on the expanded pair
 *   Teff[b,n,i,k] = z_nk t_ik (B,N,F,K),  Vrep[b,n,k,j] = v_kj (B,N,K,T). */
int ssspy_ilrma_partition_expand(const double *basis, const double *activation,
                                 const double *latent, double *Teff, double *Vrep, int B, int N,
                                 int F, int T, int K, void *stream);

enum { SSSPY_PARTITION_LATENT = 1, SSSPY_PARTITION_BASIS = 2, SSSPY_PARTITION_ACTIVATION = 4 };

/* The selected source-model updates in the reference's order (latent, basis, activation), each
 * from fresh sums; Teff / Vrep are scratch on entry and hold the expansion of the final
 * parameters on return.  y = W x, or X itself when W == NULL.
 * replaces: ssspy/bss/ilrma.py:1007-1049 (update_latent_mm), :1051-1128, :1130-1204 with
 * partitioning=True, their ME forms (:1206-1401) and the TILRMA / GGDILRMA equivalents. */
int ssspy_ilrma_partition_update(const void *X, const void *W, double *basis, double *activation,
                                 double *latent, double *Teff, double *Vrep, int B, int N, int F,
                                 int T, int K, double domain, int source_model, double model_param,
                                 int steps, int floor_kind, double floor_eps, void *workspace,
                                 size_t workspace_bytes, void *stream);

/* power normalisation with partitioning: psi_n as above from (W, C) -- pass Y == NULL -- or from
 * the separated spectrogram Y (W == C == NULL); W rows (or Y) /= psi_n;
 * z_nk <- (z_nk / psi_n^p) / s_k, t_ik <- t_ik s_k with s_k = sum_n z_nk / psi_n^p.
 * replaces: ssspy/bss/ilrma.py:365-444 (normalize_by_power, partitioning branch). */
int ssspy_ilrma_partition_normalize(void *W, const void *C, void *Y, double *basis, double *latent,
                                    int B, int N, int F, int T, int K, double domain,
                                    int floor_kind, double floor_eps, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ AuxIVA (IP1/ISS1) */

/* r2[b,n,j] = sum_i |y_nij|^2 with y = W x (or y = X when W == NULL).   r2 (B,N,T).
 * Summed without atomics (bin chunks leave partial sums in `workspace`, folded in chunk order): the
 * same bits on every run.  workspace: ssspy_iva_frame_power_workspace_bytes (0 for large batches).
 * replaces: np.linalg.norm(Y, axis=1) at ssspy/bss/iva.py:1787,1962 (squared). */
size_t ssspy_iva_frame_power_workspace_bytes(int B, int N, int F, int T);
int ssspy_iva_frame_power(const void *X, const void *W, double *r2, int B, int N, int F, int T,
                          void *workspace, size_t workspace_bytes, void *stream);

/* Y = W X (Y may be X: in place) AND r2[b,n,j] = sum_i |y_nij|^2 of the result in one walk (round 5):
 * the separate() that ends an AuxIVA ISS2 / IPA step and the frame-power pass of the next iteration's
 * weights (ssspy/bss/iva.py:1968-2066 followed by :1917-1935).  Workspace as ssspy_iva_frame_power.
 * n_sources <= 8. */
int ssspy_separate_frame_power(const void *X, const void *W, void *Y, double *r2, int B, int N,
                               int F, int T, void *workspace, size_t workspace_bytes,
                               void *stream);

/* weight[b,n,j] = G'(r)/floor(2 r), r = sqrt(r2); Gauss also refreshes variance = r2 / F.
 * replaces: ssspy/bss/iva.py:1788-1789, :1963-1964, :3105-3115, :3273-3289, :3465-3473. */
int ssspy_iva_weight(const double *r2, double *weight, double *variance, int B, int N, int F, int T,
                     int contrast, int floor_kind, double floor_eps, void *stream);

/* out[b] = sum_n mean_j G(y_nj) from r2 (and variance for Gauss).
 * replaces: ssspy/bss/iva.py:216-219, :2181-2187 (contrast part of the loss). */
int ssspy_iva_loss_data(const double *r2, const double *variance, double *out, int B, int N, int F,
                        int T, int contrast, void *stream);

/* ------------------------------------------------- gradient / natural-gradient IVA */

/* Score weights phi[b,n,j] of the Laplace / Gauss gradient classes from the frame powers r2 (B,N,T):
 * SSSPY_CONTRAST_LAPLACE 1 / floor(r), r = sqrt(r2) (the floor acts on r, not on 2 r as in
 * ssspy_iva_weight); SSSPY_CONTRAST_GAUSS refreshes variance = r2 / F and gives 1 / variance (no
 * floor, as in the reference); SSSPY_CONTRAST_GAUSS_FIXED gives 1 / variance of the variance as it
 * stands.  The score is phi_nj y_inj.  Up to SSSPY_RT_MAX_SOURCES (16) sources.
 * replaces: ssspy/bss/iva.py:2441-2451, :2610-2611, :2646-2651, :2745-2760, :2924-2935, :2969-2973. */
int ssspy_iva_score_weight(const double *r2, double *weight, double *variance, int B, int N, int F,
                           int T, int contrast, int floor_kind, double floor_eps, void *stream);

/* One gradient step on the filters W (B,F,N,N), in place:
 *   P_i[n,m] = mean_j phi(y)_inj conj(y_imj),  D = P - I (holonomic) or offdiag(P),
 *   W <- W - step_size D W (natural != 0) or W <- W - step_size D W^-H (LU with partial pivoting; a
 *   singular bin bumps info[0] -- the reference raises LinAlgError from np.linalg.inv).
 * stats: the frame-weighted covariances U (B,F,N,N,N) of the mixture under the score weights
 * (ssspy_weighted_covariance, SSSPY_WEIGHT_FRAME), row n of P being (W U_n W^H)[n,:]; or, with
 * stats_ready != 0, P itself (B,F,N,N) (ssspy_cross_covariance of the scores and the estimate: user
 * score functions).  logdet (may be NULL): the launch also leaves sum_i log|det W_i| of the filters
 * it STARTS from, as ssspy_iva_grad_step_logdet_slots() shares per mixture at
 * logdet[s * logdet_stride + b], to be added in slot order (ssspy_fold_scalar_slots); no atomics.
 * 2..8 sources are compiled per source count (a bin on 2 / 4 / 8 lanes, registers only), 9..16 take
 * the count at run time (correct, not tuned); SSSPY_ERR_UNSUPPORTED above 16.
 * replaces: ssspy/bss/iva.py:797-818, :969-988 (and np.linalg.slogdet at :234 for the loss). */
int ssspy_iva_grad_step_logdet_slots(int B, int F, int N);
int ssspy_iva_grad_step(void *W, const void *stats, int stats_ready, int B, int F, int N,
                        int natural, int holonomic, double step_size, int *info, double *logdet,
                        long long logdet_stride, void *stream);

/* ------------------------------------------------- FDICA (Laplace model) */

/* `algorithm` of the FDICA entry points */
enum {
  SSSPY_FDICA_GRAD = 0,         /* W <- W - step_size D W^-H */
  SSSPY_FDICA_NATURAL_GRAD = 1, /* W <- W - step_size D W    */
  SSSPY_FDICA_AUX_IP1 = 2,      /* one iterative-projection sweep */
  SSSPY_FDICA_AUX_IP2 = 3,      /* pairwise sweep: per-iteration operators only */
};

/* what the route function returns */
enum {
  SSSPY_FDICA_ROUTE_RESIDENT = 0,  /* one launch, the bin's slab of the mixture in LDS          */
  SSSPY_FDICA_ROUTE_STREAMING = 1, /* the same kernel, the slab re-read from memory every step  */
  SSSPY_FDICA_ROUTE_COMPOSED = 2,  /* per-iteration operators (separate, weight, covariance...) */
};

/* The per-element weight of the Laplace model on the estimate Y (B,S,F,T) (all N rows, or the two
 * rows of an IP2 pair): aux_form == 0 the score weight 1 / floor(|y|) (phi(y) = weight * y),
 * aux_form != 0 the auxiliary weight 2 / floor(2 |y|); weight (B,S,F,T) f64 (may be NULL when only
 * the contrast is wanted).  contrast (may be NULL): sum_s mean_j 2 |y_sij| of bin i of mixture b at
 * contrast[i * contrast_stride + b], to be added over the bins in slot order
 * (ssspy_fold_scalar_slots with F slots); no atomics.
 * replaces: ssspy/bss/fdica.py:1109-1112, :1231-1234, :1342, :1354-1355, :1628-1640. */
int ssspy_fdica_weight(const void *Y, double *weight, int B, int S, int F, int T, int aux_form,
                       int floor_kind, double floor_eps, double *contrast,
                       long long contrast_stride, void *stream);

/* Which route a shape takes: the bins of FDICA are independent, so a workgroup can own one
 * (mixture, bin) for a whole run.  2..4 sources: RESIDENT while the N x T slab fits 48 KiB of LDS
 * (N T <= 3072), STREAMING above.  COMPOSED for 5 sources and more (measured slower in the kernel,
 * profiles/fdica.txt), for IP2 and for more than 65535 mixtures.  -1 on a bad argument.  Host only. */
int ssspy_fdica_route(int B, int N, int F, int T, int algorithm);

/* n_steps >= 1 whole iterations of GradLaplaceFDICA / NaturalGradLaplaceFDICA / AuxLaplaceFDICA-IP1
 * on W (B,F,N,N) in place, X (B,N,F,T), in one launch; the estimate, the weights and the
 * covariances stay on chip.  loss_data and logdet (both or neither): step s leaves the contrast
 * term sum_n mean_j 2 |y| of bin i of the state it STARTS from at
 * loss_data[i * slot_stride + s * B + b] and log|det W_i| of that state in logdet likewise; entry
 * n_steps is the final state (slot_stride >= (n_steps + 1) B; add over the bins in slot order with
 * ssspy_fold_scalar_slots, F slots).  A singular bin bumps info[0].  fp64, no atomics on doubles,
 * every sum in a fixed order.  2..8 sources (compiled per count; the slab in LDS when it fits 48 KiB,
 * else re-read every step), SSSPY_ERR_UNSUPPORTED outside, for IP2 and above 65535 mixtures.
 * replaces: ssspy/bss/fdica.py:629-650, :824-843, :1104-1116 and the loss at :216-223. */
int ssspy_fdica_steps(const void *X, void *W, int B, int N, int F, int T, int algorithm,
                      int holonomic, double step_size, int floor_kind, double floor_eps,
                      int n_steps, double *loss_data, double *logdet, long long slot_stride,
                      int *info, void *stream);

/* ------------------------------------------------------------- time-domain ICA (real fp64 waveforms) */

/* `kind` of ssspy_ica_stats: the nonlinearity applied to y = W x in registers. */
enum {
  SSSPY_ICA_LAPLACE = 0,  /* G = |y|, phi = sign(y) (sign(0) = 0), phi' = 0                          */
  SSSPY_ICA_LOGISTIC = 1, /* G = max(y,0) + log1p(exp(-|y|)), phi = 1 / (1 + exp(-y)), phi' = s(1-s) */
  SSSPY_ICA_LOGCOSH = 2,  /* G = |y| + log1p(exp(-2|y|)) - log 2, phi = tanh(y), phi' = 1 - tanh^2   */
  SSSPY_ICA_IDENTITY = 3, /* G = 0, phi = y, phi' = 0 (with W = I and right = X: the Gram matrix)    */
  SSSPY_ICA_GIVEN = 4,    /* phi (and phi') are read from memory: the closures' route                */
};

/* `right` of ssspy_ica_stats: the right factor of the N x N sums. */
enum {
  SSSPY_ICA_RIGHT_Y = 0, /* sum_t phi(y_n) y_m (the gradient classes) */
  SSSPY_ICA_RIGHT_X = 1, /* sum_t phi(y_n) x_m (FastICA; the Gram matrix) */
};

/* `algorithm` of ssspy_ica_step. */
enum {
  SSSPY_ICA_FOLD_ONLY = 0,    /* fold the records (means, loss terms), leave W alone */
  SSSPY_ICA_GRAD = 1,         /* W <- W - eta D W^-T, LU with partial pivoting        */
  SSSPY_ICA_NATURAL_GRAD = 2, /* W <- W - eta D W                                     */
  SSSPY_ICA_FAST = 3,         /* fixed point, Gram-Schmidt in row order, unit rows    */
};

/* Samples of one partial record of ssspy_ica_stats.  A function of the shape only (today a constant),
 * never of the device: the records, and so every bit of the result, are the same on every run.
 * Host only. */
int ssspy_ica_chunk_samples(int N, long long T);

/* Bytes of the workspace ssspy_ica_stats fills and ssspy_ica_step folds: one record of
 * N N + 2 N doubles per (mixture, chunk).  0 on a bad argument.  Host only. */
size_t ssspy_ica_workspace_bytes(int B, int N, long long T);

/* The statistics pass.  X (B,N,T) real fp64 waveforms, W (B,N,N).  Lanes take consecutive samples
 * (coalesced loads of every channel row), form y = W x, apply the nonlinearity `kind` in registers
 * and add up, per (mixture, chunk), the record
 *   [n N + m]   sum_t phi(y_n) r_m   (r = y or x, `right`)
 *   [N N + n]   sum_t G(y_n)
 *   [N N + N + n] sum_t phi'(y_n)
 * at ws + (b chunks + chunk) (N N + 2 N).  y and phi never reach memory.  kind == SSSPY_ICA_GIVEN:
 * phi (B,N,T) is read instead (dphi (B,N,T) too when not NULL; G = 0).  Lane -> wave (butterfly) ->
 * workgroup (waves in order): a fixed order, no atomics.  2..8 sources compiled per count, 9..16
 * with the count at run time and the rows in groups of four (grid z), so that no lane holds more
 * than 80 accumulators.  SSSPY_ERR_UNSUPPORTED outside 2..16 sources and above 65535 mixtures.
 * replaces: ssspy/bss/ica.py:536-539, :691-694, :825-827 and the data term of :171-175, :397-401. */
int ssspy_ica_stats(const double *X, const double *W, const double *phi, const double *dphi,
                    void *ws, size_t ws_bytes, int B, int N, long long T, int kind, int right,
                    void *stream);

/* The step, one wave per mixture: adds the chunk records of ws in chunk order, divides by T, and
 * updates W (B,N,N) in place by `algorithm`.  loss_data (B, may be NULL): sum_n mean_t G(y_n) of
 * the state the records were formed from; logdet (B, may be NULL): log|det W| of that state (-inf
 * for a singular one); means (B, N N + 2 N, may be NULL): the folded record over T.  SSSPY_ICA_GRAD
 * bumps info[0] and leaves W alone where a pivot is exactly zero (numpy.linalg.inv raises there).
 * replaces: ssspy/bss/ica.py:540-549, :695-702, :826-836, :191. */
int ssspy_ica_step(const void *ws, size_t ws_bytes, double *W, int B, int N, long long T,
                   int algorithm, int holonomic, double step_size, double *loss_data,
                   double *logdet, double *means, int *info, void *stream);

/* Y (B,N,T) = W (B,N,N) X (B,N,T), real fp64 (ssspy/bss/ica.py:152, :379; whitening: W = P). */
int ssspy_ica_separate(const double *X, const double *W, double *Y, int B, int N, long long T,
                       void *stream);

/* ------------------------------------------------- PDSBSS (primal-dual splitting), prox of -log|det| */

/* prox_{-step_size log|det|}(X) = U diag(f(sigma)) V^H, f(s) = (s + sqrt(s^2 + 4 step_size)) / 2, for n
 * complex N x N matrices X = U diag(sigma) V^H; out (n,N,N) may be X.  One-sided (Hestenes) complex
 * Jacobi on X itself (error eps * kappa, not the eps * kappa^2 of an eigen-decomposition of X X^H),
 * a lane per matrix.  The result does not depend on phases, order or the basis inside a repeated
 * singular value; where a singular value is exactly zero it is not determined, and the kernel
 * returns finite numbers whose singular values are f(sigma).  N in [1, SSSPY_RT_MAX_SOURCES]: 1..8
 * compiled per size, 9..16 with the size at run time; SSSPY_ERR_UNSUPPORTED outside.
 * replaces: ssspy/linalg/prox.py:62-91. */
int ssspy_prox_neg_logdet(const void *X, void *out, long long n, int N, double step_size,
                          void *stream);

/* `kind` of ssspy_pdsbss_dual_step: how Yt = Z - prox(Z, step_size) is formed from
 * Z = dual_q + W2 x (ref: ssspy/linalg/prox.py:6-33, ssspy/bss/pdsbss.py:211-214, :408-409) */
enum {
  SSSPY_PROX_L1 = 0,          /* l1: the shrinkage per element                                     */
  SSSPY_PROX_L21_SOURCES = 1, /* l21, the group norm over sources (axis2 = 0): inside a lane       */
  SSSPY_PROX_L21_BINS = 2,    /* l21 over bins (axis2 = 1, the IVA penalty): r2 of ..._bin_norms   */
  SSSPY_PROX_L21_FRAMES = 3,  /* l21 over frames (axis2 = 2): inside the workgroup of a bin        */
  SSSPY_PROX_MASK = 4,        /* Yt = Z - aux Z, aux (B,N,F,T) complex128: a mask from the host    */
  SSSPY_PROX_GIVEN = 5,       /* Yt = aux (B,N,F,T) complex128, formed on the host                 */
};

/* The PDSBSS entry points: X (B,N,F,T), W and W2 (B,F,N,N), the dual variable (B,Q,N,F,T) with Q
 * penalties, all complex128; N in [1, 16], B <= 65535, SSSPY_ERR_UNSUPPORTED outside.  A penalty's
 * slice of the dual variable is passed as dual_q = dual + q N F T with dual_batch_stride = Q N F T
 * elements between mixtures.  No atomics, every sum in a fixed order. */

/* XY[b,i] = (sum_q dual[b,q])_i X[b]_i^H, (B,F,N,N): the contraction over penalties and frames.
 * replaces: ssspy/bss/pdsbss.py:205-206, :404. */
int ssspy_pdsbss_contract(const void *dual, const void *X, void *XY, int B, int Q, int N, int F,
                          int T, void *stream);

/* Per bin Wt = prox_{-mu1 log|det|}(W - mu1 mu2 XY), W2 = 2 Wt - W (the filter the dual step reads) and
 * W <- relaxation Wt + (1 - relaxation) W in place.
 * replaces: ssspy/bss/pdsbss.py:207-208, :218. */
int ssspy_pdsbss_filter_step(void *W, const void *XY, void *W2, int B, int F, int N, double mu1,
                             double mu2, double relaxation, void *stream);

/* r2[b,n,j] = sum_i |Z[b,n,i,j]|^2 (B,N,T) f64 with Z = dual_q + W2 x: partial sums over chunks of
 * bins in the workspace, added in chunk order. */
size_t ssspy_pdsbss_bin_norms_workspace_bytes(int B, int N, int F, int T);
int ssspy_pdsbss_bin_norms(const void *X, const void *W2, const void *dual_q,
                           long long dual_batch_stride, double *r2, int B, int N, int F, int T,
                           void *workspace, size_t workspace_bytes, void *stream);

/* dual_q <- relaxation Yt + (1 - relaxation) dual_q with Yt by `kind` (SSSPY_PROX_L1 .. _GIVEN);
 * r2: SSSPY_PROX_L21_BINS only; aux: SSSPY_PROX_MASK / _GIVEN only (else NULL).
 * replaces: ssspy/bss/pdsbss.py:211-214, :219, :408-412. */
int ssspy_pdsbss_dual_step(const void *X, const void *W2, void *dual_q, long long dual_batch_stride,
                           int kind, double step_size, double relaxation, const double *r2,
                           const void *aux, int B, int N, int F, int T, void *stream);

/* Z = dual_q + W2 x into Z (B,N,F,T), for proximal operators and masks that run on the host. */
int ssspy_pdsbss_form_z(const void *X, const void *W2, const void *dual_q,
                        long long dual_batch_stride, void *Z, int B, int N, int F, int T,
                        void *stream);

/* ------------------------------------------------- ADMMBSS / MaskingADMMBSS
 * (additive to ABI version 11: no existing argument list changed)
 *
 * X (B,N,F,T), W, Ainv, R, auxiliary1 and dual1 (B,F,N,N), auxiliary2 and dual2 (B,Q,N,F,T) with Q
 * penalties, all complex128; N in [1, 16], B <= 65535, SSSPY_ERR_UNSUPPORTED outside.  A penalty's
 * slices are passed as aux2_q = auxiliary2 + q N F T and dual2_q = dual2 + q N F T with batch_stride =
 * Q N F T elements between mixtures.  `kind` is SSSPY_PROX_*.  No atomics, every sum in a fixed
 * order. */

/* Once per call: Ainv[b,i] = (Q conj(X_i) X_i^T + I)^-1, Hermitian positive definite, by a Cholesky
 * factorisation per bin (the Gram matrix in the order of ssspy_admmbss_contract).
 * replaces: ssspy/bss/admmbss.py:230-231, :236 (the left-hand side), :424-425, :430. */
int ssspy_admmbss_gram_inverse(const void *X, void *Ainv, int B, int Q, int N, int F, int T,
                               void *stream);

/* R[b,i] = (sum_q (auxiliary2[b,q] - dual2[b,q]))_i X[b]_i^H, (B,F,N,N).
 * replaces: ssspy/bss/admmbss.py:233-234, :427-428 (transposed as :236 / :430 read it). */
int ssspy_admmbss_contract(const void *aux2, const void *dual2, const void *X, void *R, int B, int Q,
                           int N, int F, int T, void *stream);

/* Per bin W = Ainv (auxiliary1 - dual1 + R), U = relaxation W + (1 - relaxation) auxiliary1,
 * auxiliary1 <- prox_{-log|det| / rho}(U + dual1), dual1 <- dual1 + U - auxiliary1; W is written,
 * aux1 and dual1 in place.  An argument U + dual1 that is exactly zero gives sqrt(1 / rho) I (what the
 * reference returns there: LAPACK's U = V = I).
 * replaces: ssspy/bss/admmbss.py:232, :236, :239, :242, :252, :426, :430, :433, :435, :437. */
int ssspy_admmbss_filter_step(const void *Ainv, const void *R, void *W, void *aux1, void *dual1, int B,
                              int F, int N, double rho, double relaxation, void *stream);

/* r2[b,n,j] = sum_i |Z[b,n,i,j]|^2 (B,N,T) f64 with Z = relaxation W x + (1 - relaxation) aux2_q +
 * dual2_q: partial sums over chunks of bins in the workspace, added in chunk order. */
size_t ssspy_admmbss_bin_norms_workspace_bytes(int B, int N, int F, int T);
int ssspy_admmbss_bin_norms(const void *X, const void *W, const void *aux2_q, const void *dual2_q,
                            long long batch_stride, double relaxation, double *r2, int B, int N, int F,
                            int T, void *workspace, size_t workspace_bytes, void *stream);

/* aux2_q <- prox(Z, step_size) by `kind` (SSSPY_PROX_L1 .. _GIVEN) and dual2_q <- Z - aux2_q in place;
 * Z as above, formed in registers (aux2_q is not read when relaxation == 1).  r2: SSSPY_PROX_L21_BINS
 * only; given (B,N,F,T): SSSPY_PROX_MASK (the mask: aux2_q <- given Z) / _GIVEN (prox(Z) itself).
 * replaces: ssspy/bss/admmbss.py:237, :240, :246-250, :253, :431, :434, :436, :438. */
int ssspy_admmbss_aux_step(const void *X, const void *W, void *aux2_q, void *dual2_q,
                           long long batch_stride, int kind, double step_size, double relaxation,
                           const double *r2, const void *given, int B, int N, int F, int T,
                           void *stream);

/* Z into Z (B,N,F,T), for proximal operators and masks that run on the host. */
int ssspy_admmbss_form_z(const void *X, const void *W, const void *aux2_q, const void *dual2_q,
                         long long batch_stride, double relaxation, void *Z, int B, int N, int F,
                         int T, void *stream);

/* ------------------------------------------------- HVA (harmonic vector analysis): the mask of
 * MaskingPDSHVA inside the dual step of MaskingPDSBSS */

/* `route` of the HVA entry points: which transform the cepstral pass runs along the bins */
enum {
  SSSPY_HVA_ROUTE_AUTO = 0,   /* FFT where it exists, else DIRECT                                   */
  SSSPY_HVA_ROUTE_FFT = 1,    /* F - 1 a power of two, F <= 4097: a radix-2 FFT of length 2 (F - 1)
                                 resident in LDS, two frames per complex transform                  */
  SSSPY_HVA_ROUTE_DIRECT = 2, /* any 2 <= F <= 8192: the O(F^2) sum from the cosine table           */
};

/* The route `route` (SSSPY_HVA_ROUTE_*) resolves to for F bins: _FFT or _DIRECT; -1 where the
 * request cannot be served (F < 2, F > 8192, _FFT for an F it does not exist for).  Host only. */
int ssspy_hva_route(int F, int route);

/* table[j] = cos(pi j / (F - 1)), j < 2 (F - 1), f64: the argument is reduced to [0, pi / 2] in
 * integers first.  Both routes read it (the direct sum at (j k) mod 2 (F - 1), the FFT as twiddles). */
int ssspy_hva_cos_table(double *table, int F, void *stream);

/* The cepstral pass: per (mixture, source, frame) column of Z = dual_q + W2 x, along the bins
 *   a = floor(|Z|), zeta = log a, m = mean_f zeta, rho = zeta - m,
 *   nu = D(rho) / (2 (F - 1)), sigma = min(1, nu), mask_iter times sigma <- (1 - cos(pi sigma)) / 2,
 *   varrho = D(sigma nu) + m,
 * D(c)_k = c_0 + (-1)^k c_{F-1} + 2 sum_{0<j<F-1} c_j cos(pi j k / (F - 1)) (the DCT-I: both irfft
 * calls of the reference on a real length-F input).  varrho (B,N,F,T) f64.  A column whose mean is not
 * finite (log 0 without a floor) comes out as NaN, as from the reference.  A workgroup holds the
 * F x (tile of frames) slab of one source in LDS; no atomics, every sum in a fixed order.
 * N in [1, 16], B <= 65535, F and route as ssspy_hva_route allows; SSSPY_ERR_UNSUPPORTED outside.
 * replaces: ssspy/bss/hva.py:91-111. */
int ssspy_hva_cepstrum(const void *X, const void *W2, const void *dual_q,
                       long long dual_batch_stride, const double *table, double *varrho, int B,
                       int N, int F, int T, int floor_kind, double floor_eps, int mask_iter,
                       int route, void *stream);

/* The masked dual step: per (b, f, t) Z again, mask_n = exp(2 g (varrho_n - max)) /
 * (sum_n' exp(2 (varrho_n' - max)))^g with g = attenuation (the reference's (v / sum v)^g,
 * v = exp(2 varrho), wherever its exp neither overflows nor underflows to 0 / 0), Yt = Z - mask Z and
 * dual_q <- relaxation Yt + (1 - relaxation) dual_q in place.
 * replaces: ssspy/bss/hva.py:112-115 with ssspy/bss/pdsbss.py:408-412. */
int ssspy_hva_dual_step(const void *X, const void *W2, void *dual_q, long long dual_batch_stride,
                        const double *varrho, double attenuation, double relaxation, int B, int N,
                        int F, int T, void *stream);

/* MaskingADMMHVA: the same mask inside the auxiliary step of MaskingADMMBSS, on ADMM's operand
 * Z = relaxation W x + (1 - relaxation) aux2_q + dual2_q (aux2_q is not read when relaxation == 1).
 * (Added at SSSPY_ABI_VERSION 11 without a bump: no existing argument list changed.) */

/* The cepstral pass of ssspy_hva_cepstrum over that Z: one kernel body, the other former of Z.
 * W (B,F,N,N) the demixing filters of ssspy_admmbss_filter_step; aux2_q != dual2_q, batch_stride at
 * least N F T; table, varrho, the floor, mask_iter, route and the limits as ssspy_hva_cepstrum.
 * replaces: ssspy/bss/admmbss.py:415-442 (its Z) with ssspy/bss/hva.py:202-232. */
int ssspy_hva_admm_cepstrum(const void *X, const void *W, const void *aux2_q, const void *dual2_q,
                            long long batch_stride, const double *table, double *varrho, int B, int N,
                            int F, int T, double relaxation, int floor_kind, double floor_eps,
                            int mask_iter, int route, void *stream);

/* The masked auxiliary step: per (b, f, t) Z again, the mask of ssspy_hva_dual_step from varrho,
 * aux2_q <- mask Z and dual2_q <- Z - aux2_q in place, both from the registers that hold Z.  A NaN
 * in varrho (a log 0 column without a floor) gives NaN in both for every source of that frame, as the
 * reference's sum over sources does.  Checks as ssspy_admmbss_aux_step.
 * replaces: ssspy/bss/admmbss.py:415-442 (:436, :438) with ssspy/bss/hva.py:233-236. */
int ssspy_hva_aux_step(const void *X, const void *W, void *aux2_q, void *dual2_q,
                       long long batch_stride, const double *varrho, double attenuation,
                       double relaxation, int B, int N, int F, int T, void *stream);

/* ------------------------------------------------- FastIVA / FasterIVA, whitening, PCA */

/* The fixed-point IVA classes work on the whitened mixture Z (B,N,F,T) with unitary filters W
 * (B,F,N,N); 2..16 sources (2..8 compiled per count, 9..16 with the count at run time; correct, not
 * tuned), SSSPY_ERR_UNSUPPORTED outside.  fp64 / complex128, no atomics on doubles, every sum in a
 * fixed order.  info (device int, may be NULL) is bumped once per bin a step cannot finish. */

/* phi[b,n,j] = d_contrast / floor(2 r), psi[b,n,j] = (2 phi - dd_contrast) / floor(2 r) with
 * r = sqrt(r2); r2, d_contrast = G'(r), dd_contrast = G''(r) (NULL: zero) and the outputs (B,N,T);
 * psi may be NULL (FasterIVA needs none).  The closures of the reference run on the host on the norms; this is
 * the arithmetic around them.   replaces: ssspy/bss/iva.py:1187-1188, :1196, :1390-1391. */
int ssspy_fast_iva_weights(const double *r2, const double *d_contrast, const double *dd_contrast,
                           double *phi, double *psi, int B, int N, int T, int floor_kind,
                           double floor_eps, void *stream);

/* One pass over Z with y = W z formed in registers: c[b,i,n,m] = sum_j phi_nj conj(y_inj) z_imj
 * (B,F,N,N), b[b,i,n] = sum_j psi_nj |y_inj|^2 and a[b,i,n] = sum_j phi_nj (both (B,F,N), a the same
 * for every bin).  mean_j phi_nj y*_inj z_ij = U_in w_in, so these three
 * moments stand for the N weighted covariances per bin.
 * replaces: the (N,N,F,T) broadcasts and means of ssspy/bss/iva.py:1190-1198. */
int ssspy_fast_iva_stats(const void *Z, const void *W, const double *phi, const double *psi,
                         void *c, double *b, double *a, int B, int N, int F, int T, void *stream);

/* The FastIVA update from the moments, in place: row n of W_i <- ((a_n - b_in) / T) w_in -
 * conj(c_in) / T, then ssspy_orthonormalize_rows.   replaces: ssspy/bss/iva.py:1200-1207. */
int ssspy_fast_iva_step(void *W, const void *c, const double *b, const double *a, int B, int F,
                        int N, int T, int *info, void *stream);

/* The FasterIVA update, in place: row n of W_i <- conj of the eigenvector of the largest eigenvalue of
 * U[b,i,n] (B,F,N,N,N) = ssspy_weighted_covariance(Z, phi, SSSPY_WEIGHT_FRAME, S = N), then
 * ssspy_orthonormalize_rows.  The eigenvector's phase is the decomposition's (as with LAPACK,
 * arbitrary): a unit factor on row n that the algorithm is blind to.
 * replaces: ssspy/bss/iva.py:1395-1400. */
int ssspy_faster_iva_step(void *W, const void *U, int B, int F, int N, int *info, void *stream);

/* W_i <- (W_i W_i^H)^-1/2 W_i in place: u v^H of the singular value decomposition W = u s v^H.  A
 * Hermitian eigen-decomposition of W W^H and one Newton-Schulz step V <- V - (V V^H - I) V / 2 (forming
 * W W^H squares the conditioning of W).  A
 * W W^H whose smallest eigenvalue is not above 1e-14 of the largest, or that is not finite, bumps
 * info[0] -- the reference's np.linalg.svd never raises and returns some unitary matrix there.
 * replaces: ssspy/bss/iva.py:1204-1205, :1397-1398. */
int ssspy_orthonormalize_rows(void *W, int B, int F, int N, int *info, void *stream);

/* P (B,F,N,N) from the covariances C (B,F,N,N) = V Lambda V^H (eigenvalues ascending):
 * mode 0: Lambda^-1/2 V^H (whiten); mode 1: V^H (pca, ascend=False); mode 2: V^H with the rows in
 * descending order of the eigenvalues (pca, ascend=True).  The transform is ssspy_separate(X, P).  A
 * non-finite eigenvalue, or with mode 0 one that is not positive, bumps info[0] (the reference
 * returns inf / nan).   replaces: ssspy/transform/whiten.py:51-86, ssspy/transform/pca.py:55-88. */
int ssspy_whitening_filter(const void *C, void *P, int B, int F, int N, int mode, int *info,
                           void *stream);

/* ------------------------------------------------------------------ cACGMM */

/* The EM iteration of CACGMM (complex angular central Gaussian mixture model) for B mixtures of M
 * = 2..8 channels, N = 1..16 components (the count at run time), F bins, T frames; SSSPY_ERR_UNSUPPORTED
 * outside.  Layouts: X, Z (B,M,F,T) complex; mixing (B,N,F); covariance (B,N,F,M,M) complex; posterior
 * (B,N,F,T) real; binv (B,N,F,M*M) real: the inverse covariance packed as [M diagonal][re, im of the
 * upper triangle, row-major]; logp (B,N,F) = log mixing - log det covariance.  Nothing here uses
 * atomics on doubles: every sum has a fixed order and the results are the same bits on every run.
 * replaces: ssspy/bss/cacgmm.py:141-145, :207-222, :561-601, :629-738. */

/* Z = X / floor(||x_ij||_2) */
int ssspy_cacgmm_unit_input(const void *X, void *Z, int B, int M, int F, int T, int floor_kind,
                            double floor_eps, void *stream);

/* binv and logp of the given parameters (Cholesky on the upper triangle; a pivot that is not positive
 * bumps info[0], which may be NULL) */
int ssspy_cacgmm_prepare(const void *covariance, const double *mixing, double *binv, double *logp,
                         int B, int N, int F, int M, int *info, void *stream);

/* One pass over Z with the parameters staged by ssspy_cacgmm_prepare:
 *   q_nij = floor(max(Re z^H B_in^-1 z, 0)),  gamma = softmax_n(logp_in - M log q_nij)
 *   sum_gamma[b,n,i] = sum_j gamma,  num[b,n,i] = sum_j (gamma / q) z z^H   (both or neither)
 *   loss[b,i] = -(1/T) sum_j logsumexp_n(logp_in - M log q_nij)   (sum over i: CACGMM.compute_loss)
 *   posterior[b,n,i,j] = gamma
 * Each output may be NULL and is then not computed / not written.  posterior_in (may be NULL): the
 * sums take these posteriors instead of the pass's own softmax. */
int ssspy_cacgmm_frame_pass(const void *Z, const double *binv, const double *logp, int B, int M,
                            int N, int F, int T, int floor_kind, double floor_eps,
                            double *sum_gamma, void *num, double *loss, double *posterior,
                            const double *posterior_in, void *stream);

/* mixing = sum_gamma / T; covariance = to_psd(M num / sum_gamma) with the floor on the eigenvalues
 * (ssspy_to_psd), divided by its real trace when normalize != 0.  num is overwritten. */
int ssspy_cacgmm_parameter_step(const double *sum_gamma, void *num, double *mixing, void *covariance,
                                int B, int N, int F, int M, int T, int floor_kind, double floor_eps,
                                int normalize, void *stream);

/* covariance <- covariance / Re tr covariance, in place */
int ssspy_cacgmm_normalize(void *covariance, int B, int N, int F, int M, void *stream);

/* out[r] = sum_i terms[r * F + i], r < rows, in a fixed order (the per-bin losses of the pass) */
int ssspy_cacgmm_fold_loss(const double *terms, double *out, long long rows, int F, void *stream);

/* out[b,n,i,j] = posterior[b,n,i,j] X[b,reference_id,i,j] */
int ssspy_cacgmm_separate(const double *posterior, const void *X, void *out, int B, int N, int M,
                          int F, int T, int reference_id, void *stream);

/* ------------------------------------------------------------------ FastGaussMNMF (IP1) */

/* steps of FastGaussMNMF.update_once, OR-ed into `steps` of ssspy_fastmnmf_update */
enum {
  SSSPY_MNMF_BASIS = 1,
  SSSPY_MNMF_ACTIVATION = 2,
  SSSPY_MNMF_DIAGONALIZER = 4,
  SSSPY_MNMF_SPATIAL = 8,
  SSSPY_MNMF_NORMALIZE = 16,
  SSSPY_MNMF_ALL = 31,
};

size_t ssspy_fastmnmf_workspace_bytes(int B, int N, int M, int F, int T, int K);

/* The selected steps of update_once(), in the reference's order: basis, activation,
 * diagonaliser (IP1), spatial, power normalisation.
 * X (B,M,F,T), Q (B,F,M,M), D (B,F,N,M), basis (B,N,F,K), activation (B,N,K,T),
 * C (B,F,M,M) static covariance of X (needed by the normalisation step only).
 * replaces: ssspy/bss/mnmf.py:1278-1303 and :1305-1360, :1362-1417, :1449-1514, :1635-1675,
 * :632-678. */
int ssspy_fastmnmf_update(const void *X, const void *C, void *Q, double *D, double *basis,
                          double *activation, int B, int N, int M, int F, int T, int K, int steps,
                          int floor_kind, double floor_eps, void *workspace, size_t workspace_bytes,
                          int *info, void *stream);

/* The same steps with the |(Q x)_m|^2 hand-over: the reference recomputes Q x in every one of
 * update_basis / update_activation / update_spatial (mnmf.py:1329-1331, :1386-1388, :1659-1661);
 * here the spatial pass stores |Q x|^2 and the next iteration's basis and activation passes read
 * it (half the bytes of x, no M x M products).  `handover`: ssspy_fastmnmf_handover_doubles()
 * doubles owned by the caller -- |Q x|^2 (B,M,F,T) followed by a per-(mixture, channel) scale
 * (B,M) that absorbs the power normalisation.  *handover_valid (host): on entry, whether the
 * buffer matches the Q and X passed in (0 on the first call or after the caller changed Q or X:
 * it is then rebuilt when a step needs it); on return, whether it matches Q on exit.
 * ssspy_fastmnmf_handover_doubles() is 0 for shapes without the hand-over (use
 * ssspy_fastmnmf_update). */
size_t ssspy_fastmnmf_handover_doubles(int B, int N, int M, int F, int T, int K);
int ssspy_fastmnmf_update_handover(const void *X, const void *C, void *Q, double *D, double *basis,
                                   double *activation, int B, int N, int M, int F, int T, int K,
                                   int steps, int floor_kind, double floor_eps, void *workspace,
                                   size_t workspace_bytes, int *info, double *handover,
                                   int *handover_valid, void *stream);

/* The same (handover / handover_valid both NULL: as ssspy_fastmnmf_update) for a record_loss loop:
 * `steps` must hold SSSPY_MNMF_DIAGONALIZER, and the call also leaves sum_i log|det Q_i| of the
 * diagonalisers AS THEY COME IN -- the log-determinant term of the loss of the state the call
 * starts from (ssspy/bss/mnmf.py:1219-1261) -- as ssspy_fastmnmf_deferred_logdet_slots() shares per
 * mixture at logdet[s * logdet_stride + b], to be added in slot order (ssspy_fold_scalar_slots; a
 * run keeps one zeroed array of slots x (n_iter + 1) B doubles and passes logdet + t B): 1 where
 * the finished sums are stored, ceil(F / 16) for a handful of mixtures of up to 4 channels, where
 * the latency form of IP1 reads the diagonalisers anyway and leaves one share per tile of 16 bins
 * instead of a one-block ssspy_sum_logdet launch per iteration (shares the call does not write
 * stay as the caller zeroed them). */
int ssspy_fastmnmf_deferred_logdet_slots(int B, int N, int M, int F, int T, int K);
int ssspy_fastmnmf_update_handover_logdet(const void *X, const void *C, void *Q, double *D,
                                          double *basis, double *activation, int B, int N, int M,
                                          int F, int T, int K, int steps, int floor_kind,
                                          double floor_eps, void *workspace, size_t workspace_bytes,
                                          int *info, double *handover, int *handover_valid,
                                          double *logdet, long long logdet_stride, void *stream);

/* The data term of the loss (as ssspy_fastmnmf_loss_data) from a VALID hand-over buffer instead of
 * X and Q: half the bytes, no M x M products.  The caller guarantees that the buffer matches the
 * current Q and X (ssspy_fastmnmf_update_handover returned *handover_valid = 1 and neither moved
 * since).  out: B doubles, overwritten; workspace: ssspy_fastmnmf_loss_workspace_bytes (the
 * per-wave shares, added up in a fixed order: no fp64 atomics).
 * replaces: ssspy/bss/mnmf.py:1240-1258. */
int ssspy_fastmnmf_loss_data_handover(const double *D, const double *basis,
                                      const double *activation, const double *handover,
                                      double *out, int B, int N, int M, int F, int T, int K,
                                      void *workspace, size_t workspace_bytes, void *stream);

/* The same with the per-wave shares left RAW: share s of mixture b at slots[s * slot_stride + b],
 * s < ssspy_fastmnmf_loss_handover_slots() (0: no hand-over for the shape).  A record_loss run
 * zeroes one array of slots x (n_iter + 1) B doubles, passes slots + t B with slot_stride =
 * (n_iter + 1) B for the state after iteration t, and folds all of them in slot order with one
 * ssspy_fold_scalar_slots at the end -- instead of two memsets and a fold launch per recorded loss
 * (shares a launch does not write stay as the caller zeroed them). */
int ssspy_fastmnmf_loss_handover_slots(int B, int N, int M, int F, int T, int K);
int ssspy_fastmnmf_loss_data_handover_slots(const double *D, const double *basis,
                                            const double *activation, const double *handover,
                                            double *slots, long long slot_stride, int B, int N,
                                            int M, int F, int T, int K, void *stream);

/* Which kernels the FastGaussMNMF entry points take for a shape (host only, launches nothing; ABI
 * version 5): for tests and tools that must know which launcher branch a case exercises.  A
 * projection of the launch plan the entry points and launchers obey (csrc/mnmf_plan.hpp).  The value
 * names the kernel family:
 *   TILED    2..4 sources and channels (mnmf_kernels.hip)
 *   GENERIC  up to 8 of either (fmnmf_generic.hip)
 *   RUNTIME  9..16 of either (fmnmf_rt.hip)
 * `handover`: whether the caller passes a hand-over buffer (ssspy_fastmnmf_update_handover).
 * plan (may be NULL): SSSPY_MNMF_PLAN_INTS ints on the TILED family (0, and 0 0 1 0 for the frame
 * splits, elsewhere), at the SSSPY_MNMF_PLAN_* indices:
 *   FAST           basis, activation, covariance and spatial passes take the throughput form (0: the
 *                  k_mnmf_*<M, KSMALL> kernels -- n_basis > 16, or SSSPY_AMD_NO_FAST in the environment)
 *   KSMALL         n_basis <= 16 (the KSMALL = true instances of those kernels and of the loss)
 *   BASIS_COPY     the basis pass writes scratch and the result is copied back (n_basis > 16)
 *   GLDS_COV, GLDS_SPATIAL   the covariance / spatial pass takes the LDS-DMA form (whole frame tiles;
 *                  the spatial pass only when it writes the hand-over), else the register-fed form
 *   KQ             k-slabs of 4 of the throughput instances and of the closed-form Wiener filter:
 *                  2 (n_basis <= 8), 4 (9..16), 0 (above)
 *   HANDOVER       ssspy_fastmnmf_handover_doubles() > 0
 *   TAIL_FULL, _TAIL, _SPLIT, _GROUPS      frame splits of the 256-slot passes (basis without
 *                  hand-over, covariance, spatial): work items (mixture, 64-bin group) that walk all
 *                  frames, items whose frames are split, frame chunks of a split item, bin groups
 *   HTAIL_FULL, ...                        the same of the 512-slot hand-over basis and loss passes
 *   ACT_CHUNKS     bin chunks the activation pass folds
 *   IP1_RECORDS    the diagonaliser step hands IP1 the partial covariance records (every item split,
 *                  latency form of IP1) instead of folding them
 *   SPATIAL_FOLD_IN_NORM   with SSSPY_MNMF_SPATIAL | SSSPY_MNMF_NORMALIZE in one call the fold of
 *                  the spatial pass is left to the normalisation (every item split)
 *   LOSS_SLOTS     ssspy_fastmnmf_loss_handover_slots()
 *   LOGDET_SLOTS   ssspy_fastmnmf_deferred_logdet_slots()
 * Returns -1 for arguments the passes reject (a hand-over for a shape without one included). */
enum {
  SSSPY_MNMF_ROUTE_TILED = 0,
  SSSPY_MNMF_ROUTE_GENERIC = 1,
  SSSPY_MNMF_ROUTE_RUNTIME = 2,
};
enum {
  SSSPY_MNMF_PLAN_FAST = 0,
  SSSPY_MNMF_PLAN_KSMALL = 1,
  SSSPY_MNMF_PLAN_BASIS_COPY = 2,
  SSSPY_MNMF_PLAN_GLDS_COV = 3,
  SSSPY_MNMF_PLAN_GLDS_SPATIAL = 4,
  SSSPY_MNMF_PLAN_KQ = 5,
  SSSPY_MNMF_PLAN_HANDOVER = 6,
  SSSPY_MNMF_PLAN_TAIL_FULL = 7,
  SSSPY_MNMF_PLAN_TAIL_TAIL = 8,
  SSSPY_MNMF_PLAN_TAIL_SPLIT = 9,
  SSSPY_MNMF_PLAN_TAIL_GROUPS = 10,
  SSSPY_MNMF_PLAN_HTAIL_FULL = 11,
  SSSPY_MNMF_PLAN_HTAIL_TAIL = 12,
  SSSPY_MNMF_PLAN_HTAIL_SPLIT = 13,
  SSSPY_MNMF_PLAN_HTAIL_GROUPS = 14,
  SSSPY_MNMF_PLAN_ACT_CHUNKS = 15,
  SSSPY_MNMF_PLAN_IP1_RECORDS = 16,
  SSSPY_MNMF_PLAN_SPATIAL_FOLD_IN_NORM = 17,
  SSSPY_MNMF_PLAN_LOSS_SLOTS = 18,
  SSSPY_MNMF_PLAN_LOGDET_SLOTS = 19,
  SSSPY_MNMF_PLAN_INTS = 20,
};
int ssspy_fastmnmf_route(int B, int N, int M, int F, int T, int K, int handover, int *plan);

/* U[b,i,m] = (1/T) sum_j x x^H / R~_ijm  -> (B,F,M,M,M): the covariances the diagonaliser update
 * (IP1 inside ssspy_fastmnmf_update, or ssspy_update_by_ip2 for diagonalizer_algorithm="IP2") needs.
 * workspace: NULL, or ssspy_fastmnmf_workspace_bytes() of scratch -- with it the tuned pass of the
 * fused update runs (its split work items park partial sums there).  N, M <= 4, or 9..16 channels or
 * sources (one fused pass on the matrix cores that forms the weights itself; the workspace is not
 * used); 5..8 return SSSPY_ERR_UNSUPPORTED (use ssspy_fastmnmf_weights + ssspy_weighted_covariance).
 * replaces: ssspy/bss/mnmf.py:1504-1512, :1621-1629. */
int ssspy_fastmnmf_diagonalizer_covariance(const void *X, const double *D, const double *basis,
                                           const double *activation, void *U, int B, int N, int M,
                                           int F, int T, int K, void *workspace,
                                           size_t workspace_bytes, void *stream);

/* weights[b,m,i,j] = 1 / R~_ijm, R~ = sum_n lambda_nij d_inm (B,M,F,T): the per-channel weights of the
 * diagonaliser covariance, U = ssspy_weighted_covariance(X, weights, SSSPY_WEIGHT_BIN_FRAME, S = M).
 * Any n_sources <= 16, n_channels in [2, 16].  replaces: ssspy/bss/mnmf.py:1489-1512 (the weight part). */
int ssspy_fastmnmf_weights(const void *X, const void *Q, const double *D, const double *basis,
                           const double *activation, double *weights, int B, int N, int M, int F,
                           int T, int K, void *stream);

/* out[b] = sum_i mean_j sum_m ( |q x|^2 / R~ + log R~ ) (overwritten); caller adds
 * -2 sum logdet Q.  The per-block shares go through `workspace`
 * (ssspy_fastmnmf_loss_workspace_bytes) and are added up in a fixed order: no fp64 atomics, the
 * same bits on every run.   replaces: ssspy/bss/mnmf.py:1240-1258. */
size_t ssspy_fastmnmf_loss_workspace_bytes(int B, int N, int M, int F, int T);
int ssspy_fastmnmf_loss_data(const void *X, const void *Q, const double *D, const double *basis,
                             const double *activation, double *out, int B, int N, int M, int F,
                             int T, int K, void *workspace, size_t workspace_bytes, void *stream);

/* Multichannel Wiener filter output Y (B,N,F,T) for reference channel `reference_id`:
 * per (bin, frame) an M x M Hermitian eigen-decomposition (Jacobi) with floored eigenvalues.
 * replaces: ssspy/bss/mnmf.py:1174-1217 (separate) incl. to_psd (special/psd.py:11-71). */
int ssspy_fastmnmf_separate(const void *X, const void *Q, const double *D, const double *basis,
                            const double *activation, void *Y, int B, int N, int M, int F, int T,
                            int K, int reference_id, int floor_kind, double floor_eps,
                            void *workspace, size_t workspace_bytes, int *info, void *stream);

/* The same filter split at the eigenvalue floor of to_psd, for a flooring callable the kernels do
 * not know (round 5): stage 1 leaves the eigenvalues of R_ij in ascending order, lam (B,F,T,M) -- what
 * numpy.linalg.eigh hands the reference's flooring_fn (special/psd.py:54-62) -- and the eigenvectors
 * P (B,F,T,M,M); the caller applies the callable to lam on the host; stage 2 (same workspace,
 * untouched in between: it holds Q^-1) rebuilds R^-1 from them and writes Y.  Any N, M <= 8.
 * replaces: ssspy/bss/mnmf.py:1174-1217 with an arbitrary flooring_fn. */
int ssspy_fastmnmf_separate_eig(const void *X, const void *Q, const double *D, const double *basis,
                                const double *activation, void *Y, int B, int N, int M, int F,
                                int T, int K, int reference_id, int stage, double *lam, void *P,
                                void *workspace, size_t workspace_bytes, int *info, void *stream);

/* ------------------------------------------------------------------ GaussMNMF (full-rank SCM)
 * State: basis (B,N,F,K) f64, activation (B,N,K,T) f64, spatial (B,N,F,M,M) c128 Hermitian PSD
 * (the reference's `spatial` (N,F,M,M) with a batch axis).  n_sources N in [1, 16] (above 8 the
 * per-point kernels run their 16-source instantiations; SSSPY_ERR_UNSUPPORTED above 16).  n_basis K:
 * the full-storage per-point kernels keep the bin's N spatial matrices and N basis rows in LDS and
 * the spatial sums a row per frame of their 64-frame chunk, so every entry point returns
 * SSSPY_ERR_UNSUPPORTED, before it touches anything, unless
 *   N M^2 16 + N K 8 + 64 (2 M^2 + s) 8 <= 160 KB   (s = 16 above 8 sources at 2 and 3 channels, else 8)
 * -- K <= 2424 at 8 sources and 2 channels, 1344 at 8 and 8, 608 at 16 and 8 (ssspy_gmnmf_route
 * answers for a shape).  Above 48 KB the kernels' dynamic-LDS attribute is raised, at any source
 * count.  n_channels M in [2, 8]: one lane per
 * (bin, frame) point or per spatial matrix; from 4 channels on the point lives in one packed
 * Hermitian matrix inverted in place (herm_packed.hpp) and the full-storage kernels only redo the
 * blocks whose points leave the fast route of to_psd (flags in the workspace).
 * R_ij = to_psd(sum_n lambda_nij H_ni); the instantaneous covariance to_psd(x x^H) of
 * MNMFBase._init_instant_covariance (ssspy/bss/mnmf.py:167-188) is applied in closed form. */
enum {
  SSSPY_GMNMF_BASIS = 1,
  SSSPY_GMNMF_ACTIVATION = 2,
  SSSPY_GMNMF_SPATIAL = 4,
  SSSPY_GMNMF_NORMALIZE = 8,
  SSSPY_GMNMF_ALL = 15,
  SSSPY_GMNMF_LATENT = 16 /* partitioning only; runs last, as in update_once() */
};

size_t ssspy_gmnmf_workspace_bytes(int B, int N, int M, int F, int T, int K);

/* Which kernel forms the GaussMNMF entry points take for a shape (host only, launches nothing; ABI
 * version 6): for tests and tools that must know which launcher branch a case exercises.  A
 * projection of the launch plan the entry points obey (csrc/gmnmf_plan.hpp).  `partitioning`: the
 * caller passes latent variables.  Returns 0, or -1 for arguments the entry points reject (the LDS
 * bound above included, and n_basis > SSSPY_MAX_PARTITION_BASIS with partitioning: the LATENT step).
 * plan (may be NULL): SSSPY_GMNMF_PLAN_INTS ints at the SSSPY_GMNMF_PLAN_* indices (a byte count that
 * does not fit an int reads -1):
 *   PACKED          4..8 channels: traces, loss, separate and the spatial sums run their packed *_p
 *                   kernels first; the full-storage kernels redo the 128-frame blocks whose flag
 *                   word was raised (separate: the points marked NaN in source 0).  0: 2 and 3
 *                   channels, full-storage kernels alone
 *   TRACE_SOURCES   sources k_gmnmf_traces_p is compiled for: 4 (N <= 4), 8, or 0 (not PACKED)
 *   WIDE            9..16 sources: the GM_NWIDE forms (two groups of 8, lambda_n formed again)
 *   SPATIAL_FORM    SSSPY_GMNMF_SPATIAL_LITERAL (2, 3 channels), _PACKED (4..6:
 *                   k_gmnmf_spatial_update_p), _ROWS8 (7, 8: k_gmnmf_spatial_update_rows); the two
 *                   packed forms leave flagged blocks of 64 matrices to the literal kernel
 *   BASIS_FORM      k_gmnmf_basis: SSSPY_GMNMF_BASIS_REGISTERS (T <= 512: the bin's rows of A / Bt in
 *                   registers), _LDS_TILE (T <= 4096), _MEMORY (above: the activation from memory)
 *   BASIS_KC        basis indices it stages in LDS at a time, floor(4096 / T) (0: _MEMORY)
 *   BASIS_BPW       bins per wave, 1..16 (a workgroup takes 4 BASIS_BPW bins)
 *   ACT_CHUNKS, ACT_BINS_PER_CHUNK   bin chunks of the activation sums (slabs folded in chunk
 *                   order) and ceil(F / chunks) bins of each; trailing chunks may hold fewer, or none
 *   ACT_KSLABS      launches of 8 basis indices, ceil(K / 8)
 *   BIN_LDS_BYTES   dynamic LDS of the full-storage traces / loss / separate kernels
 *   LATENT_LDS_BYTES  of the latent update, N K 8 (0 without partitioning)
 *   FLAGS_OFFSET    byte offset of the flag words in the workspace of ssspy_gmnmf_update
 *   POINT_BLOCKS    flag words of the per-point kernels, ceil(T / 128) F B, [b][i][frame block]
 *   MATRIX_BLOCKS   flag words of the spatial update (the same words), ceil(B N F / 64)
 *   LOSS_FLAGS_OFFSET  byte offset of the POINT_BLOCKS flag words in the workspace of ssspy_gmnmf_loss */
enum {
  SSSPY_GMNMF_SPATIAL_LITERAL = 0,
  SSSPY_GMNMF_SPATIAL_PACKED = 1,
  SSSPY_GMNMF_SPATIAL_ROWS8 = 2,
};
enum {
  SSSPY_GMNMF_BASIS_REGISTERS = 0,
  SSSPY_GMNMF_BASIS_LDS_TILE = 1,
  SSSPY_GMNMF_BASIS_MEMORY = 2,
};
enum {
  SSSPY_GMNMF_PLAN_PACKED = 0,
  SSSPY_GMNMF_PLAN_TRACE_SOURCES = 1,
  SSSPY_GMNMF_PLAN_WIDE = 2,
  SSSPY_GMNMF_PLAN_SPATIAL_FORM = 3,
  SSSPY_GMNMF_PLAN_BASIS_FORM = 4,
  SSSPY_GMNMF_PLAN_BASIS_KC = 5,
  SSSPY_GMNMF_PLAN_BASIS_BPW = 6,
  SSSPY_GMNMF_PLAN_ACT_CHUNKS = 7,
  SSSPY_GMNMF_PLAN_ACT_BINS_PER_CHUNK = 8,
  SSSPY_GMNMF_PLAN_ACT_KSLABS = 9,
  SSSPY_GMNMF_PLAN_BIN_LDS_BYTES = 10,
  SSSPY_GMNMF_PLAN_LATENT_LDS_BYTES = 11,
  SSSPY_GMNMF_PLAN_FLAGS_OFFSET = 12,
  SSSPY_GMNMF_PLAN_POINT_BLOCKS = 13,
  SSSPY_GMNMF_PLAN_MATRIX_BLOCKS = 14,
  SSSPY_GMNMF_PLAN_LOSS_FLAGS_OFFSET = 15,
  SSSPY_GMNMF_PLAN_INTS = 16,
};
int ssspy_gmnmf_route(int B, int N, int M, int F, int T, int K, int partitioning, int *plan);

/* The steps of update_once() selected by `steps`, in the reference's order: basis, activation,
 * spatial (H <- to_psd(P^-1 # H Q H), the matrix geometric mean of linalg/mean.py:6-83 type 2),
 * unit-trace normalisation of H with the scale moved into the basis, latent variables.
 * latent == NULL: basis (B,N,F,K), activation (B,N,K,T).  latent (B,N,K) given (partitioning):
 * basis (B,F,K) and activation (B,K,T) are shared, lambda_nij = sum_k z_nk t_ik v_kj, and the
 * normalisation leaves the basis alone (n_basis up to SSSPY_MAX_PARTITION_BASIS for the LATENT step:
 * above, a call that selects it returns SSSPY_ERR_UNSUPPORTED before any step has run).
 * ssspy_gmnmf_loss / _separate take the per-source pair
 * that ssspy_ilrma_partition_expand writes.
 * replaces: ssspy/bss/mnmf.py:806-834, :836-901, :903-968, :970-1016, :391-414, :1018-1073. */
int ssspy_gmnmf_update(const void *X, double *basis, double *activation, double *latent,
                       void *spatial, int B, int N, int M, int F, int T, int K, int steps,
                       int floor_kind, double floor_eps, void *workspace, size_t workspace_bytes,
                       void *stream);

/* out[b] = sum_i mean_j ( tr(R^-1 XX) + log det R ); `out` (B doubles) is overwritten; the
 * per-block shares go through `workspace` (ssspy_gmnmf_loss_workspace_bytes) and are added up in
 * a fixed order (no fp64 atomics).
 * replaces: ssspy/bss/mnmf.py:765-804. */
size_t ssspy_gmnmf_loss_workspace_bytes(int B, int F, int T);
int ssspy_gmnmf_loss(const void *X, const double *basis, const double *activation,
                     const void *spatial, double *out, int B, int N, int M, int F, int T, int K,
                     int floor_kind, double floor_eps, void *workspace, size_t workspace_bytes,
                     void *stream);

/* multichannel Wiener filter: Y[b,n,i,j] = (lambda_nij H_ni R_ij^-1 x_ij)[reference_id]
 * -> Y (B,N,F,T) c128.  replaces: ssspy/bss/mnmf.py:729-763. */
int ssspy_gmnmf_separate(const void *X, const double *basis, const double *activation,
                         const void *spatial, void *Y, int B, int N, int M, int F, int T, int K,
                         int reference_id, int floor_kind, double floor_eps, void *stream);

/* ------------------------------------------------------------------ Hermitian matrix functions
 * One matrix per lane, M in [2, 16] (9 .. 16: the size at run time, csrc/hermitian_rt.hip); arrays
 * flattened to (n, M, M) c128.
 * Tested magnitude range (these, ssspy_eigh, ssspy_to_psd and ssspy_solve): entries from 2^-240 to
 * 2^240 for the one-matrix entry points and from 2^-120 to 2^120 for those that take two matrices, so
 * that every square and pairwise product the kernels form stays inside [1e-300, 1e300], the range the
 * Jacobi rotation and the Cholesky pivots assume (tests/test_gpu_linalg_elementwise.py).
 * generalised eigh through the Cholesky factor of B, eigenvalues ascending -> lamb (n, M), Z (n, M, M):
 *   type 1: A z = lamb B z; 2: A B z = lamb z; 3: B A z = lamb z.   replaces: ssspy/linalg/eigh.py:8-81, :164-207 */
int ssspy_eigh_general(const void *A, const void *Bm, double *lamb, void *Z, long long n, int M,
                       int type, int *info, void *stream);
/* inverse == 0: X^(1/2); inverse == 1: P diag(1 / floor(sqrt(lam))) P^H.  replaces: linalg/sqrtm.py:8-64 */
int ssspy_sqrtmh(const void *X, void *out, long long n, int M, int inverse, int floor_kind,
                 double floor_eps, void *stream);
/* geometric mean: type 1: A # B; 2: A^-1 # B; 3: A # B^-1.   replaces: ssspy/linalg/mean.py:6-83 */
int ssspy_gmeanmh(const void *A, const void *Bm, void *G, long long n, int M, int type,
                  void *stream);
/* y = argmin of the log-quadratically penalised quadratic (type 2): H (n, L, L) Hermitian, v (n, L),
 * z (n) -> y (n, L), L in [1, 15] (8 .. 15: the dimension at run time, csrc/ipa_rt.hip).
 * newton_ws (one 64-bit word of scratch) / not_converged: as for
 * ssspy_ipa_sweep, the n problems forming one group (the reference's loop stops when all of them
 * have converged); NULL: max_iter Newton steps per problem.
 * replaces: ssspy/linalg/lqpqm.py:13-352 (lqpqm2 with singular_fn = "x < flooring_fn(0)"). */
int ssspy_lqpqm2(const void *H, const void *v, const double *z, void *y, long long n, int L,
                 int max_iter, int floor_kind, double floor_eps, void *newton_ws,
                 int *not_converged, void *stream);
/* The same with the reference's `singular_fn` evaluated by the caller: singular (n ints, device) is
 * singular_fn(||v||) per problem -- None: ||v|| == 0, or any callable (the norms are n numbers the
 * host forms from its own v); problems flagged singular take the "v = 0" branch and stay out of the
 * joint convergence test.  replaces: ssspy/linalg/lqpqm.py:61-78 (singular_fn), :80-110. */
int ssspy_lqpqm2_masked(const void *H, const void *v, const double *z, void *y, long long n, int L,
                        int max_iter, int floor_kind, double floor_eps, void *newton_ws,
                        int *not_converged, const int *singular, void *stream);

/* ------------------------------------------------------------------ IPSDTA (block decomposition)
 * GaussIPSDTA / TIPSDTA with the MM source model and the VCD spatial model (ssspy/bss/ipsdta.py).
 * The F bins are cut into n_blocks blocks; a launch covers one partition of equal block size L
 * (the reference's "low" blocks of size F / n_blocks and its "high" blocks of one more,
 * ipsdta.py:545-556): n_part_blocks blocks from bin first_bin on, numbered from first_block among
 * all n_blocks.  2 <= N <= 8, 1 <= L <= 8, 1 <= K <= 32.
 * X (B, N, F, T), W (B, F, N, N), basis (B, N, K, n_part_blocks, L, L) c128; activation (B, N, K, T),
 * pi (B, N, T) f64 or NULL (weight 1: the Gaussian model).
 * Per (mixture, source, block, frame): y = W x on the block's bins, R = to_psd(sum_k v T) with
 * to_psd's default floor (max-flooring of the eigenvalues at 1e-10; ipsdta.py:643-647), R^-1,
 * u = R^-1 y.  `mode` selects what leaves the pass:
 *   SSSPY_IPSDTA_QUAD  out0 = Re(y^H R^-1 y), out1 = log det R, both (B, N, n_blocks, T) f64
 *                      (ipsdta.py:1174-1181, :1438-1446)
 *   SSSPY_IPSDTA_BASIS out0 = P = mean_t v R^-1, out1 = Q = mean_t v pi u u^H, both shaped as basis
 *                      (ipsdta.py:926-939, :1469-1483)
 *   SSSPY_IPSDTA_ACT   out0 = pi Re(u^H T_k u), out1 = Re tr(R^-1 T_k), both (B, N, K, n_blocks, T)
 *                      f64: the terms of ipsdta.py:1001-1004, :1586-1589 before the sum over blocks
 *   SSSPY_IPSDTA_COV   out0 (B, n_part_blocks, L, L, N, N, N) c128 = mean_t pi R^-1[b][a] x_a x_b^H,
 *                      the weighted covariance of the VCD sweep (ipsdta.py:1096-1102, :1711-1718);
 *                      out1 unused
 * route: NULL, or (B, N, n_blocks, T) int32: 1 where the matrix took the eigenvalue route of to_psd
 * (0: a Cholesky factorisation of R - 1e-10 I proved the floor idle). */
enum { SSSPY_IPSDTA_QUAD = 0, SSSPY_IPSDTA_BASIS = 1, SSSPY_IPSDTA_ACT = 2, SSSPY_IPSDTA_COV = 3 };
int ssspy_ipsdta_frame_pass(const void *X, const void *W, const void *basis, const double *activation,
                            const double *pi, int B, int N, int F, int T, int K, int n_part_blocks,
                            int L, int first_bin, int first_block, int n_blocks, int mode,
                            void *out0, void *out1, int *route, void *stream);

/* From the QUAD outputs: pi = (dof + 2F) / (dof + 2 sum_blocks max(quad, 0)) (B, N, T) (model
 * SSSPY_SOURCE_T; ipsdta.py:1518, :1618, :1758; NULL: not wanted) and the data term of the loss (B)
 * (NULL: not wanted): Gauss mean_t(max(sum quad, 0) per partition + sum log det R)
 * (ipsdta.py:1177-1184), t mean_t(sum_n (dof + 2F) / 2 log(1 + 2 / dof sum_blocks max(quad, 0)) +
 * sum log det R) (ipsdta.py:1840-1866).  The first n_low_blocks blocks are the low partition. */
int ssspy_ipsdta_weight_loss(const double *quad, const double *logdet, int B, int N, int n_blocks,
                             int n_low_blocks, int T, int F, int model, double dof, double *pi,
                             double *loss, void *stream);

/* activation (B, N, K, T) *= sqrt(sum_blocks num / sum_blocks den) from the ACT outputs
 * (ipsdta.py:1027-1033, :1623-1632). */
int ssspy_ipsdta_activation(double *activation, const double *num, const double *den, int B, int N,
                            int K, int n_blocks, int T, void *stream);

/* Trace normalisation: T /= tr, V *= tr with tr the trace of a (source, basis)'s matrices summed
 * over both partitions (ipsdta.py:666-697).  basis_high may be NULL with n_high_blocks == 0. */
int ssspy_ipsdta_normalize(void *basis_low, void *basis_high, double *activation, int B, int N, int K,
                           int n_low_blocks, int L_low, int n_high_blocks, int L_high, int T,
                           void *stream);

/* The VCD sweep of one partition, in place on W (B, F, N, N) (_update_spatial_model.py:516-608):
 * weighted_covariance (B, n_part_blocks, L, L, N, N, N); the singular branch is taken where
 * |xi_hat| < threshold (ipsdta.py:1104-1106: flooring_fn(0)).  info[0] counts singular systems. */
int ssspy_ipsdta_vcd(void *W, const void *weighted_covariance, int B, int F, int N, int n_part_blocks,
                     int L, int first_bin, double threshold, int *info, void *stream);

/* out = (A B) C for n matrices of size L x L (1..8), none aliasing out: the products of the basis
 * steps, T Q T (ipsdta.py:940) and Q^1/2 T P T Q^1/2, T Q^1/2 (.) Q^1/2 T (ipsdta.py:1487-1489). */
int ssspy_matmul3(const void *A, const void *Bm, const void *C, void *out, long long n, int L,
                  void *stream);

/* The PSDTF handed out: out (S, T, n_part_blocks, L, L) c128 = to_psd(sum_k v[s, k, t] T[s, k, c])
 * with the floor (floor_kind, floor_eps) on the eigenvalues; exactly Hermitian.  S counts the leading
 * (mixture, source) pairs; activation (S, K, T) f64; basis (S, K, n_part_blocks, L, L) c128, or with
 * basis_last != 0 the reference's other layout (S, n_part_blocks, L, L, K).  1 <= L <= 16 (above 8:
 * the full-matrix PSDTF of IPSDTABase.reconstruct_psdtf, n_part_blocks == 1), 1 <= K <= 32.
 * A lane per matrix, the sum over k in the order of k.
 * replaces: ssspy/bss/ipsdta.py:260-300 (reconstruct_psdtf), :584-664.
 * (Added at SSSPY_ABI_VERSION 11 without a bump: no existing argument list changed.) */
int ssspy_ipsdta_reconstruct(const void *basis, const double *activation, void *out, long long S,
                             int K, int T, int n_part_blocks, int L, int basis_last, int floor_kind,
                             double floor_eps, void *stream);

/* ------------------------------------------------------------------ permutation alignment
 * The two solvers of ssspy/algorithm/permutation_alignment.py, batched and device-resident
 * (csrc/permutation.hip), with the decisions of the host solvers of this package: the first
 * permutation, in itertools.permutations(range(N)) order, of the largest score.
 * A sequence is addressed by strides in elements: (b, n, f, t) at
 * b * stride_b + n * stride_n + f * stride_f + t.  perm is int32 (B, F, N): aligned component n of
 * bin f is original component perm[b, f, n].  2..8 sources (N! permutations are enumerated per
 * bin).  Every sum runs in a fixed order; two runs give the same bits.
 * (Added at SSSPY_ABI_VERSION 11 without a bump: no existing argument list changed.) */
enum { SSSPY_PERM_SOLVER_CORRELATION = 0, SSSPY_PERM_SOLVER_SCORE = 1 };
enum { SSSPY_PERM_ROUTE_DEVICE = 0, SSSPY_PERM_ROUTE_HOST = 1 };
/* layouts of ssspy_permute_sources */
enum {
  SSSPY_PERM_LAYOUT_BIN_SOURCE = 0, /* (B, F, N, inner): filters, the host order of the solvers */
  SSSPY_PERM_LAYOUT_SOURCE_BIN = 1, /* (B, N, F, inner): spectrograms, posteriors, mixing weights  */
};

/* SSSPY_PERM_ROUTE_DEVICE where the kernels below take N sources and T frames with `solver` and the
 * floor `floor_kind` (SSSPY_FLOOR_*; anything else stands for a callable only the host can run),
 * SSSPY_PERM_ROUTE_HOST otherwise: fewer than 2 or more than 8 sources, an unknown floor, or, for
 * the correlation solver, N * T > 16384 (its criterion stays in LDS).  -1 for a bad argument. */
int ssspy_permutation_route(int N, int T, int solver, int floor_kind);

/* index[m] = the first permutation p maximising sum_i tables[m, p[i], i]; tables (n_tables, N, N) */
int ssspy_best_permutation(const double *tables, int *index, long long n_tables, int N,
                           void *stream);

/* envelope (B, F, N, T) = |y| / floor(sqrt(sum_n |y|^2)) and overlap (B, F) = the sum of all
 * entries of P P^T per bin; sequence f64 (is_complex == 0) or c128. */
int ssspy_permutation_envelope_overlap(const void *sequence, int is_complex, long long stride_b,
                                       long long stride_n, long long stride_f, double *envelope,
                                       double *overlap, int B, int N, int F, int T, int floor_kind,
                                       double floor_eps, void *stream);

/* The sweep of the correlation solver over the bins in `order` (B, F) int32 (the argsort of the
 * overlaps): one workgroup per mixture, the criterion in LDS (N * T <= 16384). */
int ssspy_permutation_correlation_sweep(const double *envelope, const int *order, int *perm, int B,
                                        int N, int F, int T, void *stream);

/* normalized (B, F, N, T): every (bin, component) at zero mean and unit population deviation */
int ssspy_permutation_score_normalize(const double *sequence, long long stride_b, long long stride_n,
                                      long long stride_f, double *normalized, int B, int N, int F,
                                      int T, void *stream);

/* global_iter rounds of the global stage on perm (B, F, N) in place (rows are addressed through it);
 * centroid (B, N, T) is scratch, centroid_std (B, N) receives the deviation of the last centroid
 * (with global_iter == 0 that of the sequences as perm orders them). */
int ssspy_permutation_score_global(const double *normalized, int *perm, double *centroid,
                                   double *centroid_std, int B, int N, int F, int T, int global_iter,
                                   int floor_kind, double floor_eps, void *stream);

/* local_iter walks over the bins in increasing order, one workgroup per mixture, on perm in place */
int ssspy_permutation_score_local(const double *normalized, const double *centroid_std, int *perm,
                                  int B, int N, int F, int T, int local_iter, int floor_kind,
                                  double floor_eps, void *stream);

/* dst = the sources of src gathered by perm, out of place, in 8-byte words: dst contiguous in
 * `layout`, word w of (b, f, n) of src at b * stride_b + f * stride_f + n * stride_n + w. */
int ssspy_permute_sources(const void *src, void *dst, const int *perm, int B, int N, int F,
                          long long inner_words, int layout, long long stride_b, long long stride_f,
                          long long stride_n, void *stream);

/* out (B, N, F, T) = |posterior X[:, reference_id]|: the amplitude targets of CACGMM's alignment */
int ssspy_permutation_amplitude(const double *posterior, const void *X, double *out, int B, int N,
                                int M, int F, int T, int reference_id, void *stream);

/* ------------------------------------------------------------------ special functions, quadratic forms
 * The device forms of ssspy.special.softmax / logsumexp and ssspy.linalg.quadratic for tensors that
 * are on the device already (csrc/special.hip).  A float64 tensor reduced over one axis is
 * addressed as (outer, len, inner), contiguous, the reduced axis in the middle: inner == 1 when it
 * is the last axis, otherwise the axis is walked by its stride.  The maximum of a row is subtracted
 * before exp; a wave owns a row, lane l sums elements l, l + 64, ... in order and the 64 partial sums
 * meet in a fixed butterfly: two runs give the same bits.
 * (Added at SSSPY_ABI_VERSION 11 without a bump: no existing argument list changed.) */

/* out (outer, len, inner) = exp(x - max) / sum exp(x - max).  replaces: ssspy/special/softmax.py:4-36 */
int ssspy_softmax(const double *X, double *out, long long outer, int len, long long inner,
                  void *stream);
/* out (outer, inner) = log sum exp(x - max) + max.  replaces: ssspy/special/logsumexp.py:4-40 */
int ssspy_logsumexp(const double *X, double *out, long long outer, int len, long long inner,
                    void *stream);
/* out[i] = x_i^H A_i x_i.  X (n, N), A (n, N, N), out (n) complex128, 1 <= N <= 16; a lane per form.
 * replaces: ssspy/linalg/quadratic.py:4-25. */
int ssspy_quadratic(const void *X, const void *A, void *out, long long n, int N, void *stream);

/* ------------------------------------------------------------------ OverIVA (csrc/overiva.hip)
 * Overdetermined AuxIVA-IP1 (Scheibler & Ono, WASPAA 2019): N <= M demixing rows W_t; the full filter
 * W (B, F, M, M) = [W_t ; [J, -I]] carries a Gaussian background J (M - N, N) fixed by
 * [J, -I] C W_t^H = 0, J = (E2 C W_t^H)(E1 C W_t^H)^-1.  2 <= M <= 16, 1 <= N <= M, else
 * SSSPY_ERR_UNSUPPORTED.  (Added at SSSPY_ABI_VERSION 11 without a bump: no existing argument list
 * changed.) */

/* r2 (B, N, T) = sum_i |y_nij|^2 with y = W_t x; Y (B, N, F, T) receives y when not NULL.  The N x M
 * rows of bin (b, i) start at Wt + (b F + i) w_stride complex numbers (N M for a packed filter, M M for
 * the first rows of the full one).  Bin chunks are folded in chunk order: no fp64 atomics, the same
 * bits on every run.  `workspace`: ssspy_overiva_frame_power_workspace_bytes(...) bytes (may be 0). */
size_t ssspy_overiva_frame_power_workspace_bytes(int B, int N, int F, int T);
int ssspy_overiva_frame_power(const void *X, const void *Wt, long long w_stride, void *Y, double *r2,
                              int B, int M, int N, int F, int T, void *workspace,
                              size_t workspace_bytes, void *stream);

/* One sweep on W (B, F, M, M) in place.  With logdet / trace (B each; both or neither) the sums over
 * the bins of log|det W| and Re tr(U C U^H), U = [J, -I], of the filter AS IT COMES IN are left there
 * first (`workspace`: ssspy_overiva_step_workspace_bytes(B, F) bytes).  Then, with V (B, F, N, M, M)
 * the weighted covariances of the N sources: for n = 0..N-1 in order row n <- IP1 (the arithmetic of
 * ssspy_update_by_ip1 on the full filter with V_n) and rows N.. <- [J, -I] re-formed from C
 * (B, F, M, M).  With V == NULL no row is updated; rows N.. are re-formed only when logdet is NULL too
 * (the state a call starts from).  A pivot of either solve that is not above 16 eps size times the
 * largest entry of its column before the elimination bumps info[0]. */
size_t ssspy_overiva_step_workspace_bytes(int B, int F);
int ssspy_overiva_step(void *W, const void *V, const void *C, int B, int F, int M, int N,
                       int floor_kind, double floor_eps, int *info, double *logdet, double *trace,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ WPE (csrc/wpe.hip)
 * Dereverberation by weighted prediction error: Nakatani, Yoshioka, Kinoshita, Miyoshi, Juang,
 * "Speech dereverberation based on variance-normalized delayed linear prediction", IEEE TASLP 18(7),
 * 2010.  Per bin, with x_t the M channels of frame t, xs_t in C^L (L = taps M) the stacked history,
 * entry k M + m = x[m, t - delay - k] and zero before the first frame (eq. 24), and G (L, M) the
 * prediction filter: y_t = x_t - G^H xs_t (eq. 26).  X, Y (B, M, F, T), G (B, F, L, M) complex128.
 * One workgroup per (mixture, bin).  1 <= M <= 8, taps >= 1, taps M <= 64, else
 * SSSPY_ERR_UNSUPPORTED; delay >= 1 and floor_kind one of SSSPY_FLOOR_*, else SSSPY_ERR_BADARG.
 * No fp64 atomics: the same bits on every run.  `route`: SSSPY_WPE_ROUTE_AUTO, or
 * SSSPY_WPE_ROUTE_STREAMING to re-read the slab where it would fit in LDS (the tests compare the
 * two).  (Added at SSSPY_ABI_VERSION 11 without a bump: no existing argument list changed.) */
enum {
  SSSPY_WPE_ROUTE_AUTO = 0,
  SSSPY_WPE_ROUTE_RESIDENT = 1,  /* the M x T slab of the bin stays in LDS for the whole launch */
  SSSPY_WPE_ROUTE_STREAMING = 2, /* the slab is re-read from memory in tiles on every walk       */
};

/* SSSPY_WPE_ROUTE_RESIDENT or _STREAMING for a shape (-1: a shape the kernels do not take);
 * lds_bytes (may be NULL) receives the dynamic LDS of a workgroup on that route. */
int ssspy_wpe_route(int B, int M, int F, int T, int taps, int *lds_bytes);

/* n_steps >= 1 iterations on G in place in one launch, each: lambda_t = floor(mean_m |y_mt|^2)
 * (eq. 45), R = sum_t xs_t xs_t^H / lambda_t and P = sum_t xs_t x_t^H / lambda_t (eq. 46, 47),
 * G = R^-1 P by a Cholesky factorisation (eq. 48); then Y of the last G when Y is not NULL.
 * loss_data (may be NULL): (F, slot_stride), slot_stride >= (n_steps + 1) B; iteration s leaves
 * (1 / T) sum_t [M log lambda_t + sum_m |y_mt|^2 / lambda_t] (the negative log-likelihood of eq. 41
 * up to a constant) of the state it STARTS from at [f, s B + b] and the last state goes to entry
 * n_steps; fold the bins with ssspy_fold_scalar_slots.  A pivot that is not positive and finite bumps
 * info[0] once per (mixture, bin) and ends the iterations of that bin: its G stays what the failing
 * iteration started from and its Y is formed from that. */
int ssspy_wpe_steps(const void *X, void *G, void *Y, int B, int M, int F, int T, int taps, int delay,
                    int floor_kind, double floor_eps, int n_steps, double *loss_data,
                    long long slot_stride, int *info, int route, void *stream);

/* One iteration (eq. 45 - 48) and Y of the new G.  What the iteration formed is handed out where the
 * pointer is not NULL: lambda (B, F, T), R (B, F, L, L) as a full Hermitian matrix, P (B, F, L, M)
 * and the upper-triangular Cholesky factor U (B, F, L, L), R = U^H U, zeros below the diagonal. */
int ssspy_wpe_step(const void *X, void *G, void *Y, int B, int M, int F, int T, int taps, int delay,
                   int floor_kind, double floor_eps, int *info, double *lambda, void *R, void *P,
                   void *U, int route, void *stream);

/* Y = X - G^H xs (eq. 26) for a given G; Y and loss_data (as above with n_steps = 0: one entry per
 * mixture and bin) may each be NULL, not both. */
int ssspy_wpe_apply(const void *X, const void *G, void *Y, int B, int M, int F, int T, int taps,
                    int delay, int floor_kind, double floor_eps, double *loss_data,
                    long long slot_stride, int route, void *stream);

/* ------------------------------------------------------------------ mask-based beamformers
 * (csrc/beamform.hip)  Masks as covariance weights (Higuchi et al., ICASSP 2016; Heymann et al.,
 * ICASSP 2016).  Per (mixture, bin), with x_t the M channels of frame t, m_nt >= 0 the mask of source
 * n and u_nt its noise weight -- noise_mask (B, N, F, T), or (B, F, T) shared by the sources when
 * noise_shared, or 1 - m_nt formed by the kernel when noise_mask is NULL (never total minus signal):
 *   S_n = sum_t m_nt x_t x_t^H, a_n = sum_t m_nt, N_n = sum_t u_nt x_t x_t^H, b_n = sum_t u_nt
 *   Phi_s = S_n / max(a_n, 1e-10)
 *   Phi_v = N_n / max(b_n, 1e-10) + diagonal_loading (tr(N_n / max(b_n, 1e-10)) / M) I
 * X (B, M, F, T) and Y (B, N, F, T) complex128, masks float64, W (B, F, N, M) complex128 with row n
 * the filter w_n^H (Y = W X per bin), covariances (B, F, N, M, M) complex128 as full Hermitian
 * matrices, a and b (B, F, N) float64.  One workgroup per (mixture, bin); every sum is formed in frame
 * order by one thread: no fp64 atomics, the same bits on every run and on both routes.
 * 1 <= M <= 8 and 1 <= N <= 16, else SSSPY_ERR_UNSUPPORTED.
 * (Added at SSSPY_ABI_VERSION 11 without a bump, as the WPE entry points were: no existing argument
 * list changed.) */
enum {
  SSSPY_BEAMFORM_MVDR = 0,          /* Souden, Benesty, Affes, IEEE TASLP 18(2), 2010, eq. 18        */
  SSSPY_BEAMFORM_GEV_REFERENCE = 1, /* Warsitz, Haeb-Umbach, IEEE TASLP 15(5), 2007, eq. 12, scaled  */
                                    /* to be distortionless towards the reference channel            */
  SSSPY_BEAMFORM_GEV_BAN = 2,       /* the same with blind analytic normalisation (eq. 30)           */
  SSSPY_BEAMFORM_MWF = 3,           /* speech-distortion-weighted MWF (Souden 2010, eq. 16; Doclo)   */
};
enum {
  SSSPY_BEAMFORM_ROUTE_AUTO = 0,
  SSSPY_BEAMFORM_ROUTE_RESIDENT = 1,  /* the M x T slab of the bin stays in LDS: X is read once     */
  SSSPY_BEAMFORM_ROUTE_STREAMING = 2, /* the slab is re-read in tiles for the apply walk            */
};

/* SSSPY_BEAMFORM_ROUTE_RESIDENT (16 M T <= 48 KiB) or _STREAMING for a shape (-1: a shape the kernel
 * does not take); lds_bytes (may be NULL) receives the dynamic LDS of a workgroup of
 * ssspy_beamform_run on that route. */
int ssspy_beamform_route(int B, int M, int N, int F, int T, int *lds_bytes);

/* The sums alone: S <- S_n, Nv <- N_n, a <- a_n, b <- b_n; with normalize, S <- S_n / max(a_n, 1e-10)
 * and Nv <- N_n / max(b_n, 1e-10) (no loading), the division ssspy_beamform_run makes. */
int ssspy_beamform_covariances(const void *X, const double *mask, const double *noise_mask,
                               int noise_shared, void *S, void *Nv, double *a, double *b, int B,
                               int M, int N, int F, int T, int normalize, void *stream);

/* W from given Phi_s and Phi_v (loading included), `kind` one of SSSPY_BEAMFORM_*:
 *   MVDR  A = Phi_v^-1 Phi_s by a Cholesky factorisation, w = A e_ref / max(Re tr A, 1e-10)
 *         (Souden 2010, eq. 18)
 *   MWF   w = (Phi_s + mu Phi_v)^-1 Phi_s e_ref, mu > 0 (Souden 2010, eq. 16)
 *   GEV   Phi_v = L L^H, C = L^-1 Phi_s L^-H, v the unit eigenvector of its largest eigenvalue
 *         (Hermitian Jacobi), w0 = L^-H v (Warsitz 2007, eq. 12), a = L v = Phi_v w0;
 *         _REFERENCE: w = w0 conj(a_ref); _BAN: w = w0 p ||a|| / sqrt(M), p = conj(a_ref) / |a_ref|
 *         (1 where a_ref = 0) -- eq. 30 with the phase pinned.  Both are invariant under the phase of v.
 * A Phi_s that is zero in every entry gives w = 0.  A Cholesky pivot that is not positive and finite
 * bumps info[0] (may be NULL) once per (mixture, bin, source), and that source gets w = 0. */
int ssspy_beamform_filter(const void *Phi_s, const void *Phi_v, void *W, int B, int M, int N, int F,
                          int kind, int reference_id, double mu, int *info, void *stream);

/* Everything in one launch: the sums, Phi_s and Phi_v, the filters of ssspy_beamform_filter and
 * y_nt = w_n^H x_t.  W, Y and the pair Phi_s, Phi_v may each be NULL (not all): what is NULL is not
 * written.  `route`: SSSPY_BEAMFORM_ROUTE_AUTO, or _STREAMING to re-read the slab where it would fit
 * in LDS (the tests compare the two). */
int ssspy_beamform_run(const void *X, const double *mask, const double *noise_mask, int noise_shared,
                       void *W, void *Y, void *Phi_s, void *Phi_v, int B, int M, int N, int F, int T,
                       int kind, int reference_id, double diagonal_loading, double mu, int *info,
                       int route, void *stream);

/* Y = W X per bin for given filters W (B, F, N, M): the apply walk of ssspy_beamform_run. */
int ssspy_beamform_apply(const void *X, const void *W, void *Y, int B, int M, int N, int F, int T,
                         void *stream);

/* ------------------------------------------------------------------ WPD (csrc/wpd.hip)
 * The convolutional beamformer (weighted power minimisation distortionless response): Nakatani,
 * Kinoshita, IEEE SPL 26(6), 2019; Boeddeker et al., ICASSP 2020 for the form without a steering
 * vector.  Per (mixture, bin, source), with x_t the M channels of frame t and Lb = (taps + 1) M: the
 * stacked vector xb_t in C^Lb has block 0 = x_t and block j = 1..taps = x_{t - delay - (j - 1)}, zero
 * before the first frame; the filter wb in C^Lb gives y_t = wb^H xb_t.  X (B, M, F, T), Y (B, N, F, T)
 * and W (B, F, N, Lb) complex128, W[l] = conj(wb[l]) (Y = W xb per bin); mask (B, N, F, T) float64;
 * steering (B, F, N, M) complex128.  One workgroup per (mixture, bin, source); every sum is formed in
 * frame order by one thread: no fp64 atomics, the same bits on every run and on both routes.
 * 1 <= M <= 8, taps >= 0, (taps + 1) M <= 64 and 1 <= N <= 16, else SSSPY_ERR_UNSUPPORTED; delay >= 1
 * and floor_kind one of SSSPY_FLOOR_*, else SSSPY_ERR_BADARG.  `route`: SSSPY_WPD_ROUTE_AUTO, or
 * SSSPY_WPD_ROUTE_STREAMING to re-read the slab where it would fit in LDS (the tests compare the
 * two).  (Added at SSSPY_ABI_VERSION 11 without a bump, as the WPE and beamformer entry points were:
 * no existing argument list changed.) */
enum {
  SSSPY_WPD_ROUTE_AUTO = 0,
  SSSPY_WPD_ROUTE_RESIDENT = 1,  /* the M x T slab of the bin stays in LDS for the whole launch */
  SSSPY_WPD_ROUTE_STREAMING = 2, /* the slab is re-read from memory in tiles on every walk       */
};

/* SSSPY_WPD_ROUTE_RESIDENT (16 M (T + max(taps - 1, 0)) <= 48 KiB) or _STREAMING for a shape (-1: a
 * shape the kernels do not take); lds_bytes (may be NULL) receives the dynamic LDS of a workgroup on
 * that route. */
int ssspy_wpd_route(int B, int M, int N, int F, int T, int taps, int *lds_bytes);

/* n_steps >= 1 iterations on W in place in one launch, each: lambda_t = floor(|y_t|^2),
 * R = (1 / T) sum_t xb_t xb_t^H / lambda_t + diagonal_loading (tr R / Lb) I, R = U^H U (Cholesky), and
 *   mask form (steering == NULL): Phi_s = sum_t m_t x_t x_t^H / max(sum_t m_t, 1e-10), summed in the
 *     first walk; A = (R^-1)[:, :M] Phi_s; wb = A[:, ref] / Re tr(A[:M, :])
 *   steering form (mask may be NULL): vb = [v; 0], a = R^-1 vb, wb = a conj(v_ref) / (vb^H a)
 * with wb = 0 where the denominator is zero or not finite (an all-zero mask); then Y of the last W
 * when Y is not NULL.  Phi_s (may be NULL; mask form) receives (B, F, N, M, M), full Hermitian.
 * loss_data (may be NULL): (F N, slot_stride), slot_stride >= (n_steps + 1) B; iteration s leaves
 * (1 / T) sum_t [log lambda_t + |y_t|^2 / lambda_t] of the state it STARTS from at
 * [f N + n, s B + b] and the last state goes to entry n_steps; fold the rows with
 * ssspy_fold_scalar_slots.  A pivot that is not positive and finite bumps info[0] once per (mixture,
 * bin, source) and ends the iterations of that triple: its W stays what the failing iteration started
 * from, its Y is formed from that, and the loss term of that kept state fills every entry behind the
 * failing iteration's (s + 1 .. n_steps). */
int ssspy_wpd_steps(const void *X, const double *mask, const void *steering, void *W, void *Phi_s,
                    void *Y, int B, int M, int N, int F, int T, int taps, int delay, int reference_id,
                    double diagonal_loading, int floor_kind, double floor_eps, int n_steps,
                    double *loss_data, long long slot_stride, int *info, int route, void *stream);

/* One iteration and Y of the new W.  What the iteration formed is handed out where the pointer is not
 * NULL: lambda (B, F, N, T), R (B, F, N, Lb, Lb) as a full Hermitian matrix (loading included), Phi_s
 * and the upper-triangular Cholesky factor U (B, F, N, Lb, Lb), R = U^H U, zeros below the diagonal. */
int ssspy_wpd_step(const void *X, const double *mask, const void *steering, void *W, void *Phi_s,
                   void *Y, int B, int M, int N, int F, int T, int taps, int delay, int reference_id,
                   double diagonal_loading, int floor_kind, double floor_eps, int *info,
                   double *lambda, void *R, void *U, int route, void *stream);

/* Y = W xb for given filters; Y and loss_data (as above with n_steps = 0: one entry per mixture, bin
 * and source) may each be NULL, not both. */
int ssspy_wpd_apply(const void *X, const void *W, void *Y, int B, int M, int N, int F, int T, int taps,
                    int delay, int floor_kind, double floor_eps, double *loss_data,
                    long long slot_stride, int route, void *stream);

/* ------------------------------------------------------------------ ConvIVA (csrc/conviva.hip)
 * IVA with joint dereverberation (convolutional AuxIVA): Nakatani et al., Interspeech 2020 (the
 * source-wise factorisation); Ikeshita et al., WASPAA 2019.  As many sources as channels, N = M.  With
 * xb_t, Lb and W (B, F, N, Lb) as for WPD above, L = taps M and phi (B, N, T) float64 the auxiliary
 * weights of the sources (ssspy_iva_weight on the frame powers of the estimate), per (mixture, bin,
 * source): Rb = (1 / T) sum_t phi_t xb_t xb_t^H, C = Rb[:M, :M], P = Rb[M:, :M], R = Rb[M:, M:] +
 * diagonal_loading (Re tr R / L) I (taps > 0), G = R^-1 P through R = U^H U (Cholesky) and the Schur
 * complement Sigma = C - P^H G (Sigma = C with taps = 0).  ssspy_update_by_ip1 on the demixing rows
 * Q = W[..., :M] with Sigma as the weighted covariances is the row update; ssspy_conviva_compose forms
 * the convolutional filters from its result and ssspy_wpd_apply the estimate.  One workgroup per
 * (mixture, bin, source); every sum is formed in frame order by one thread: no fp64 atomics, the same
 * bits on every run and on both routes.  2 <= M <= 8, taps >= 0 and (taps + 1) M <= 64, else
 * SSSPY_ERR_UNSUPPORTED; delay >= 1 else SSSPY_ERR_BADARG.  (Added at SSSPY_ABI_VERSION 11 without a
 * bump, as the WPD entry points were: no existing argument list changed.) */
enum {
  SSSPY_CONVIVA_ROUTE_AUTO = 0,
  SSSPY_CONVIVA_ROUTE_RESIDENT = 1,  /* the M x T slab of the bin stays in LDS for the launch */
  SSSPY_CONVIVA_ROUTE_STREAMING = 2, /* the slab is re-read from memory in tiles              */
};
enum {
  SSSPY_CONVIVA_MIN_CHANNELS = 2,
  SSSPY_CONVIVA_MAX_CHANNELS = 8,
  SSSPY_CONVIVA_MAX_ORDER = 64, /* (taps + 1) * n_channels */
};

/* SSSPY_CONVIVA_ROUTE_RESIDENT (16 M (T + max(taps - 1, 0)) <= 48 KiB) or _STREAMING for a shape (-1:
 * a shape the kernel does not take); lds_bytes (may be NULL) receives the dynamic LDS of a workgroup
 * on that route. */
int ssspy_conviva_route(int B, int M, int F, int T, int taps, int *lds_bytes);

/* Sigma (B, F, M, M, M), full Hermitian with an exactly real diagonal, and G (B, F, M, L, M) (may be
 * NULL with taps = 0) of every (mixture, bin, source).  failed (B, F, M) int32, zeroed by the caller
 * once per run: bit 0 is set by a launch in which the triple met a Cholesky pivot that is not positive
 * and finite and cleared by one in which it did not, bit 1 stays set from the first such launch on;
 * info[0] (may be NULL) is bumped when bit 1 is set: once per triple and run.  Sigma and G of a triple
 * that failed are not written.  Rb_out (B, F, M, Lb, Lb), full Hermitian with the loading, and U_out
 * (B, F, M, L, L), upper triangular with zeros below the diagonal, may each be NULL.  `route`:
 * SSSPY_CONVIVA_ROUTE_AUTO, or _STREAMING to re-read the slab where it would fit in LDS. */
int ssspy_conviva_statistics(const void *X, const double *phi, void *Sigma, void *G, int B, int M,
                             int F, int T, int taps, int delay, double diagonal_loading, int *info,
                             int *failed, void *Rb_out, void *U_out, int route, void *stream);

/* The same statistics with the weights of the ILRMA source model (ILRMA with joint dereverberation,
 * ILRMA-T of Ikeshita et al.), which depend on the bin: phi_nft = (sum_k basis[b, n, f, k]
 * activation[b, n, k, t])^(-2 / domain), basis (B, M, F, n_basis) and activation (B, M, n_basis, T)
 * float64, N = M.  The workgroup of a (mixture, bin, source) forms the weights of every tile of frames
 * itself where ssspy_conviva_statistics copies phi: one thread per frame sums over k in ascending order,
 * then 1 / s with domain = 2 (no pow) and pow(s, -2 / domain) otherwise; the basis row is staged once in
 * LDS (n_basis doubles on top of what ssspy_conviva_route reports), the activation is read coalesced
 * along t.  The weights are not floored (the reference's varphi = 1 / R is not): a sum of zero gives
 * phi = inf, R is not finite and the triple takes the failure path.  Everything behind the weights is
 * the kernel body of ssspy_conviva_statistics, and so are Sigma, G, info, failed, Rb_out, U_out, route
 * and the limits on M and taps; no atomics, the same bits on every run, on both routes, in a batch or
 * alone.  phi_out (B, M, F, T) float64 (tests; may be NULL) receives the weights.  1 <= n_basis <=
 * SSSPY_CONVIVA_MAX_BASIS else SSSPY_ERR_UNSUPPORTED; domain outside (0, 2] or delay < 1:
 * SSSPY_ERR_BADARG.  (Added at SSSPY_ABI_VERSION 11 without a bump: no existing argument list
 * changed.) */
enum { SSSPY_CONVIVA_MAX_BASIS = 32 };
int ssspy_conviva_statistics_nmf(const void *X, const double *basis, const double *activation,
                                 void *Sigma, void *G, int B, int M, int F, int T, int taps,
                                 int delay, int n_basis, double domain, double diagonal_loading,
                                 int *info, int *failed, void *Rb_out, void *U_out, double *phi_out,
                                 int route, void *stream);

/* Power normalisation of that model on the convolutional state: psi_n = floor(sqrt(mean_{f,t}
 * |y_nft|^2)) from Y (B, M, F, T); Y[n] /= psi_n, W[:, n, :] /= psi_n on all (taps + 1) M entries of
 * the row (W (B, F, M, Lb)) and basis[n] /= psi_n^domain.  Y and W take the same psi, so Y stays W xb
 * to one rounding per entry; G and the loss do not change.  workspace: one double per (mixture,
 * source, 16 bin rows), added in order (no atomics).
 * replaces: ssspy/bss/ilrma.py:365-444 (normalize_by_power) on a state the reference does not have. */
size_t ssspy_convilrma_normalize_workspace_bytes(int B, int M, int F);
int ssspy_convilrma_normalize(void *Y, void *W, double *basis, int B, int M, int F, int T, int taps,
                              int n_basis, double domain, int floor_kind, double floor_eps,
                              void *workspace, size_t workspace_bytes, void *stream);

/* W (B, F, M, Lb) from the demixing rows Q (B, F, M, M) and G: wb = [q; -G q] with q the conjugated
 * row, stored conjugated: W[:M] = Q row, W[M + l] = -sum_m conj(G[l][m]) Q[m].  The row of a triple
 * with bit 0 of `failed` (may be NULL) set is not touched. */
int ssspy_conviva_compose(const void *Q, const void *G, void *W, const int *failed, int B, int M,
                          int F, int taps, void *stream);

/* ------------------------------------------------------------------ STFT / ISTFT
 * The transforms the reference's workflow takes from SciPy either side of a separator
 * (tests/package/bss/test_ilrma.py, test_iva.py, test_mnmf.py: scipy.signal.stft(x, window="hann",
 * nperseg=n_fft, noverlap=n_fft - hop) and scipy.signal.istft), with SciPy's defaults:
 * boundary="zeros", padded=True, one-sided, scaling="spectrum".  n_fft: a power of two <= 65536
 * or ANY length in [2, 32768], even or odd, as SciPy's nperseg (Bluestein's chirp-z on two radix-2
 * transforms).  Transforms of up to 8192 points run in LDS; longer ones (a power of two above 8192,
 * any other length above 4096) on workgroup-private slices of the workspace.  `workspace` =
 * ssspy_stft_workspace_bytes(n_fft) bytes on the device: the chirp's spectrum and those slices; 0 /
 * NULL for a power of two <= 8192.
 * x (B, C, n_samples) f64 -> Z (B, C, n_fft/2+1, ssspy_stft_frames(...)) c128; `window` (n_fft) f64
 * on the device, `window_sum` its sum. */
int ssspy_stft_frames(long long n_samples, int n_fft, int hop);
size_t ssspy_stft_workspace_bytes(int n_fft);
int ssspy_stft(const double *x, void *Z, const double *window, double window_sum, int B, int C,
               long long n_samples, int n_fft, int hop, void *workspace, void *stream);

/* Z (B, C, n_fft/2+1, n_frames) -> x (B, C, ssspy_istft_samples(...)); `segments` is scratch of
 * B*C*n_frames*n_fft doubles, `workspace` as for ssspy_stft. */
long long ssspy_istft_samples(int n_frames, int n_fft, int hop);
int ssspy_istft(const void *Z, double *x, const double *window, double window_sum,
                double *segments, int B, int C, int n_frames, int n_fft, int hop, void *workspace,
                void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SSSPY_AMD_H */
