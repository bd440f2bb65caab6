"""ctypes binding of libssspy_amd.so (the C ABI declared in include/ssspy_amd.h).

The product path has no CPU fallback: if the shared library is missing or an entry point
fails, an exception is raised.
"""

import ctypes
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# SSSPY_AMD_LIB: another build of the same library (A / B runs of kernel experiments)
LIB_PATH = os.environ.get("SSSPY_AMD_LIB") or os.path.join(_PKG, "lib", "libssspy_amd.so")

OK, ERR_BADARG, ERR_HIP, ERR_UNSUPPORTED, ERR_INTERNAL = 0, 1, 2, 3, 4
FLOOR_NONE, FLOOR_MAX, FLOOR_ADD = 0, 1, 2
WEIGHT_UNIT, WEIGHT_FRAME, WEIGHT_BIN_FRAME = 0, 1, 2
SOURCE_GAUSS, SOURCE_T, SOURCE_GGD = 0, 1, 2
PARTITION_LATENT, PARTITION_BASIS, PARTITION_ACTIVATION = 1, 2, 4
SOURCE_ME = 0x100  # OR-ed into the model: source_algorithm="ME"
CONTRAST_LAPLACE, CONTRAST_GAUSS, CONTRAST_GAUSS_FIXED = 0, 1, 2
# `mode` of ssspy_whitening_filter, named after what pca() asks for: the first principal component
# (largest eigenvalue) in the last channel (ascend=False) or in the first (ascend=True)
WHITEN, PCA_FIRST_COMPONENT_LAST, PCA_FIRST_COMPONENT_FIRST = 0, 1, 2
# SSSPY_IPSDTA_*: `mode` of ssspy_ipsdta_frame_pass; the limits of the IPSDTA kernels
IPSDTA_QUAD, IPSDTA_BASIS, IPSDTA_ACT, IPSDTA_COV = range(4)
IPSDTA_MAX_SOURCES, IPSDTA_MAX_BLOCK, IPSDTA_MAX_BASIS = 8, 8, 32
# SSSPY_ROUTE_*: what ssspy_ilrma_route returns
(ROUTE_LATENCY, ROUTE_THROUGHPUT, ROUTE_GROUPED, ROUTE_GENERIC, ROUTE_WIDE_BASIS,
 ROUTE_RUNTIME_N) = range(6)
# SSSPY_MNMF_ROUTE_*: what ssspy_fastmnmf_route returns; SSSPY_MNMF_PLAN_*: the names of its plan ints
MNMF_ROUTE_TILED, MNMF_ROUTE_GENERIC, MNMF_ROUTE_RUNTIME = range(3)
MNMF_PLAN_FIELDS = ("fast", "ksmall", "basis_copy", "glds_cov", "glds_spatial", "kq", "handover",
                    "tail_full", "tail_tail", "tail_split", "tail_groups", "htail_full", "htail_tail",
                    "htail_split", "htail_groups", "act_chunks", "ip1_records", "spatial_fold_in_norm",
                    "loss_slots", "logdet_slots")
# SSSPY_GMNMF_PLAN_*: the names of the plan ints of ssspy_gmnmf_route; SSSPY_GMNMF_SPATIAL_* / _BASIS_*
GMNMF_PLAN_FIELDS = ("packed", "trace_sources", "wide", "spatial_form", "basis_form", "basis_kc",
                     "basis_bpw", "act_chunks", "act_bins_per_chunk", "act_kslabs", "bin_lds_bytes",
                     "latent_lds_bytes", "flags_offset", "point_blocks", "matrix_blocks",
                     "loss_flags_offset")
GMNMF_SPATIAL_LITERAL, GMNMF_SPATIAL_PACKED, GMNMF_SPATIAL_ROWS8 = range(3)
GMNMF_BASIS_REGISTERS, GMNMF_BASIS_LDS_TILE, GMNMF_BASIS_MEMORY = range(3)
# SSSPY_FDICA_*: `algorithm` of the FDICA entry points; SSSPY_FDICA_ROUTE_*: what ssspy_fdica_route returns
FDICA_GRAD, FDICA_NATURAL_GRAD, FDICA_AUX_IP1, FDICA_AUX_IP2 = range(4)
FDICA_ROUTE_RESIDENT, FDICA_ROUTE_STREAMING, FDICA_ROUTE_COMPOSED = range(3)
# SSSPY_WPE_ROUTE_*: `route` of the WPE entry points and what ssspy_wpe_route returns; the limits
WPE_ROUTE_AUTO, WPE_ROUTE_RESIDENT, WPE_ROUTE_STREAMING = range(3)
WPE_MAX_CHANNELS, WPE_MAX_ORDER = 8, 64
# SSSPY_BEAMFORM_*: `kind` of the beamformer entry points; SSSPY_BEAMFORM_ROUTE_*: their `route` and
# what ssspy_beamform_route returns; the limits
BEAMFORM_MVDR, BEAMFORM_GEV_REFERENCE, BEAMFORM_GEV_BAN, BEAMFORM_MWF = range(4)
BEAMFORM_ROUTE_AUTO, BEAMFORM_ROUTE_RESIDENT, BEAMFORM_ROUTE_STREAMING = range(3)
BEAMFORM_MAX_CHANNELS, BEAMFORM_MAX_SOURCES = 8, 16
# SSSPY_WPD_ROUTE_*: `route` of the WPD entry points and what ssspy_wpd_route returns; the limits
# ((taps + 1) * n_channels <= WPD_MAX_ORDER)
WPD_ROUTE_AUTO, WPD_ROUTE_RESIDENT, WPD_ROUTE_STREAMING = range(3)
WPD_MAX_CHANNELS, WPD_MAX_ORDER, WPD_MAX_SOURCES = 8, 64, 16
# SSSPY_CONVIVA_ROUTE_*: `route` of ssspy_conviva_statistics and what ssspy_conviva_route returns; the
# limits ((taps + 1) * n_channels <= CONVIVA_MAX_ORDER)
CONVIVA_ROUTE_AUTO, CONVIVA_ROUTE_RESIDENT, CONVIVA_ROUTE_STREAMING = range(3)
CONVIVA_MIN_CHANNELS, CONVIVA_MAX_CHANNELS, CONVIVA_MAX_ORDER = 2, 8, 64
CONVIVA_MAX_BASIS = 32  # n_basis of ssspy_conviva_statistics_nmf
# SSSPY_ICA_*: `kind`, `right` of ssspy_ica_stats and `algorithm` of ssspy_ica_step
ICA_LAPLACE, ICA_LOGISTIC, ICA_LOGCOSH, ICA_IDENTITY, ICA_GIVEN = range(5)
ICA_RIGHT_Y, ICA_RIGHT_X = range(2)
ICA_FOLD_ONLY, ICA_GRAD, ICA_NATURAL_GRAD, ICA_FAST = range(4)
ICA_MIN_SOURCES = 2
# SSSPY_PROX_*: `kind` of ssspy_pdsbss_dual_step
PROX_L1, PROX_L21_SOURCES, PROX_L21_BINS, PROX_L21_FRAMES, PROX_MASK, PROX_GIVEN = range(6)
# SSSPY_HVA_ROUTE_*: `route` of the HVA entry points and what ssspy_hva_route returns
HVA_ROUTE_AUTO, HVA_ROUTE_FFT, HVA_ROUTE_DIRECT = range(3)
MAX_PAIRS = 32
# SSSPY_PERM_*: `solver` of ssspy_permutation_route and what it returns; `layout` of
# ssspy_permute_sources
PERM_SOLVER_CORRELATION, PERM_SOLVER_SCORE = range(2)
PERM_ROUTE_DEVICE, PERM_ROUTE_HOST = range(2)
PERM_LAYOUT_BIN_SOURCE, PERM_LAYOUT_SOURCE_BIN = range(2)
# SSSPY_MAX_SOURCES (per-N kernels: IPA, both MNMF classes, the Hermitian operators; GaussMNMF's
# channels and the ILRMA partition entry points stop there), SSSPY_RT_MAX_SOURCES (run-time-N kernels:
# the shared operators, ILRMA, AuxIVA, FastGaussMNMF's channels and sources, GaussMNMF's sources),
# SSSPY_MAX_BASIS
MAX_SOURCES, RT_MAX_SOURCES, MAX_BASIS = 8, 16, 65536
ABI_VERSION = 11  # SSSPY_ABI_VERSION of the include/ssspy_amd.h these prototypes mirror

_p, _i, _d, _z = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
_q = ctypes.c_longlong

# name -> (restype, argtypes); mirrors include/ssspy_amd.h one to one
PROTOTYPES = {
    "ssspy_amd_version": (ctypes.c_char_p, []),
    "ssspy_abi_version": (_i, []),
    "ssspy_last_error": (ctypes.c_char_p, []),
    "ssspy_separate": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "ssspy_weighted_covariance": (_i, [_p, _p, _i, _p, _i, _i, _i, _i, _i, _p]),
    "ssspy_cross_covariance": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "ssspy_update_by_ip1": (_i, [_p, _p, _i, _i, _i, _i, _d, _p, _p]),
    "ssspy_update_by_ip1_logdet_slots": (_i, [_i, _i, _i]),
    "ssspy_update_by_ip1_logdet": (_i, [_p, _p, _i, _i, _i, _i, _d, _p, _p, _q, _p]),
    "ssspy_ip1_source_solve": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _p]),
    "ssspy_scale_filter_row": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "ssspy_iss1_transform": (_i, [_p, _p, _i, _i, _i, _i, _d, _p]),
    "ssspy_update_by_ip2": (_i, [_p, _p, _i, _p, _i, _i, _i, _i, _i, _d, _p, _p]),
    "ssspy_covariance_congruence": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "ssspy_covariance_congruence_sets": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "ssspy_covariance_congruence_tracked": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _p, _i, _p]),
    "ssspy_compose_filters": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "ssspy_ipa_sweep": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _d, _p, _p, _p, _p]),
    "ssspy_ipa_sweep_newton_words": (_z, [_i, _i]),
    "ssspy_debug_barrier_timeouts": (_i, []),
    "ssspy_iss2_transform": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _d, _p, _p]),
    "ssspy_update_by_ip2_deferred": (_i, [_p, _p, _i, _p, _i, _i, _i, _p, _p, _p]),
    "ssspy_iss2_transform_deferred": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _p, _p]),
    "ssspy_iss1_fused_max_frames": (_i, [_i]),
    "ssspy_iss1_fused_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "ssspy_iss1_fused": (_i, [_p, _p, _i, _p, _i, _i, _i, _i, _i, _d, _p, _z, _p]),
    "ssspy_iss1_fused_tracked": (_i, [_p, _p, _i, _p, _i, _i, _i, _i, _i, _d, _p, _p, _z, _p]),
    "ssspy_projection_back_filter": (_i, [_p, _p, _i, _i, _i, _i, _p, _p]),
    "ssspy_mdp_scale": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "ssspy_ilrma_scale_basis": (_i, [_p, _p, _i, _i, _i, _i, _d, _p]),
    "ssspy_projection_back_scale": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _p]),
    "ssspy_demix_from_covariance": (_i, [_p, _p, _p, _i, _i, _i, _p, _p]),
    "ssspy_sum_logdet": (_i, [_p, _p, _i, _i, _i, _p]),
    "ssspy_logdet": (_i, [_p, _p, _q, _i, _p]),
    "ssspy_solve": (_i, [_p, _p, _p, _q, _i, _i, _p, _p]),
    "ssspy_inv2": (_i, [_p, _p, _q, _p]),
    "ssspy_eigh": (_i, [_p, _p, _p, _q, _i, _p]),
    "ssspy_to_psd": (_i, [_p, _p, _q, _i, _i, _d, _p]),
    "ssspy_herm_rebuild": (_i, [_p, _p, _p, _q, _i, _i, _p]),
    "ssspy_eigh2": (_i, [_p, _p, _p, _p, _q, _i, _p, _p]),
    "ssspy_ilrma_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "ssspy_ilrma_update_basis": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _d, _i, _d, _i, _d, _p, _z,
                                      _p]),
    "ssspy_ilrma_update_activation": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _d, _i, _d, _i, _d, _p,
                                           _z, _p]),
    "ssspy_ilrma_weighted_covariance": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _d, _i, _d, _i,
                                             _d, _p, _z, _p]),
    "ssspy_ilrma_normalize_filter": (_i, [_p, _p, _p, _i, _i, _i, _i, _d, _i, _d, _p, _z, _p]),
    "ssspy_ilrma_normalize_output": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _d, _i, _d, _p, _z, _p]),
    "ssspy_ilrma_normalize_output_tracked": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _d, _i, _d, _p, _z,
                                                  _p, _p]),
    "ssspy_ilrma_iss_weight": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _d, _i, _d, _i, _d, _p]),
    "ssspy_ilrma_iss_weight_power": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _d, _i, _d, _i, _d, _p]),
    "ssspy_ilrma_loss_workspace_bytes": (_z, [_i, _i, _i, _i, _i, _i]),
    "ssspy_ilrma_loss_data": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _d, _i, _d, _p, _z, _p]),
    "ssspy_ilrma_ip1_update": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _d, _i, _d, _i, _i, _d,
                                    _p, _z, _p, _p]),
    "ssspy_ilrma_deferred_loss_supported": (_i, [_i, _i, _i, _i, _d, _i]),
    "ssspy_ilrma_ip1_update_deferred_loss": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _d, _i,
                                                  _d, _i, _i, _d, _p, _z, _p, _p, _p, _p]),
    "ssspy_ilrma_deferred_loss_slots": (_i, [_i, _i, _i, _i, _i, _d, _i]),
    "ssspy_ilrma_deferred_logdet_slots": (_i, [_i, _i, _i, _i, _i, _d, _i]),
    "ssspy_ilrma_ip1_update_loss_slots": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _d, _i,
                                               _d, _i, _i, _d, _p, _z, _p, _p, _q, _p, _p]),
    "ssspy_fold_scalar_slots_workspace_bytes": (_z, [_q, _i]),
    "ssspy_fold_scalar_slots": (_i, [_p, _q, _i, _p, _p, _z, _p]),
    "ssspy_ilrma_route": (_i, [_i, _i, _i, _i, _i, _d, _i, ctypes.POINTER(ctypes.c_int),
                                ctypes.POINTER(ctypes.c_int)]),
    "ssspy_ilrma_partition_expand": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "ssspy_ilrma_partition_update": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _d, _i, _d,
                                          _i, _i, _d, _p, _z, _p]),
    "ssspy_ilrma_partition_normalize": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _d, _i, _d, _p,
                                             _z, _p]),
    "ssspy_iva_frame_power_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "ssspy_iva_frame_power": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _z, _p]),
    "ssspy_separate_frame_power": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _z, _p]),
    "ssspy_iva_weight": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _d, _p]),
    "ssspy_iva_loss_data": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "ssspy_overiva_frame_power_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "ssspy_overiva_frame_power": (_i, [_p, _p, _q, _p, _p, _i, _i, _i, _i, _i, _p, _z, _p]),
    "ssspy_overiva_step_workspace_bytes": (_z, [_i, _i]),
    "ssspy_overiva_step": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _d, _p, _p, _p, _p, _z, _p]),
    "ssspy_iva_score_weight": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _d, _p]),
    "ssspy_iva_grad_step_logdet_slots": (_i, [_i, _i, _i]),
    "ssspy_iva_grad_step": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _d, _p, _p, _q, _p]),
    "ssspy_fdica_weight": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _d, _p, _q, _p]),
    "ssspy_fdica_route": (_i, [_i, _i, _i, _i, _i]),
    "ssspy_fdica_steps": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _d, _i, _d, _i, _p, _p, _q, _p, _p]),
    "ssspy_wpe_route": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int)]),
    "ssspy_wpe_steps": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _d, _i, _p, _q, _p, _i, _p]),
    "ssspy_wpe_step": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _d, _p, _p, _p, _p, _p, _i, _p]),
    "ssspy_wpe_apply": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _d, _p, _q, _i, _p]),
    "ssspy_beamform_route": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int)]),
    "ssspy_beamform_covariances": (_i, [_p, _p, _p, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "ssspy_beamform_filter": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _d, _p, _p]),
    "ssspy_beamform_run": (_i, [_p, _p, _p, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _d, _d, _p,
                                _i, _p]),
    "ssspy_beamform_apply": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "ssspy_wpd_route": (_i, [_i, _i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int)]),
    "ssspy_wpd_steps": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _d, _i, _d, _i, _p,
                             _q, _p, _i, _p]),
    "ssspy_wpd_step": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _d, _i, _d, _p, _p,
                            _p, _p, _i, _p]),
    "ssspy_wpd_apply": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _d, _p, _q, _i, _p]),
    "ssspy_conviva_route": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int)]),
    "ssspy_conviva_statistics": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _d, _p, _p, _p, _p, _i,
                                      _p]),
    "ssspy_conviva_statistics_nmf": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _d, _d, _p,
                                          _p, _p, _p, _p, _i, _p]),
    "ssspy_convilrma_normalize_workspace_bytes": (_z, [_i, _i, _i]),
    "ssspy_convilrma_normalize": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _d, _i, _d, _p, _z, _p]),
    "ssspy_conviva_compose": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "ssspy_ica_chunk_samples": (_i, [_i, _q]),
    "ssspy_ica_workspace_bytes": (_z, [_i, _i, _q]),
    "ssspy_ica_stats": (_i, [_p, _p, _p, _p, _p, _z, _i, _i, _q, _i, _i, _p]),
    "ssspy_ica_step": (_i, [_p, _z, _p, _i, _i, _q, _i, _i, _d, _p, _p, _p, _p, _p]),
    "ssspy_ica_separate": (_i, [_p, _p, _p, _i, _i, _q, _p]),
    "ssspy_prox_neg_logdet": (_i, [_p, _p, _q, _i, _d, _p]),
    "ssspy_pdsbss_contract": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "ssspy_pdsbss_filter_step": (_i, [_p, _p, _p, _i, _i, _i, _d, _d, _d, _p]),
    "ssspy_pdsbss_bin_norms_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "ssspy_pdsbss_bin_norms": (_i, [_p, _p, _p, _q, _p, _i, _i, _i, _i, _p, _z, _p]),
    "ssspy_pdsbss_dual_step": (_i, [_p, _p, _p, _q, _i, _d, _d, _p, _p, _i, _i, _i, _i, _p]),
    "ssspy_pdsbss_form_z": (_i, [_p, _p, _p, _q, _p, _i, _i, _i, _i, _p]),
    "ssspy_admmbss_gram_inverse": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "ssspy_admmbss_contract": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "ssspy_admmbss_filter_step": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _d, _d, _p]),
    "ssspy_admmbss_bin_norms_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "ssspy_admmbss_bin_norms": (_i, [_p, _p, _p, _p, _q, _d, _p, _i, _i, _i, _i, _p, _z, _p]),
    "ssspy_admmbss_aux_step": (_i, [_p, _p, _p, _p, _q, _i, _d, _d, _p, _p, _i, _i, _i, _i, _p]),
    "ssspy_admmbss_form_z": (_i, [_p, _p, _p, _p, _q, _d, _p, _i, _i, _i, _i, _p]),
    "ssspy_hva_route": (_i, [_i, _i]),
    "ssspy_hva_cos_table": (_i, [_p, _i, _p]),
    "ssspy_hva_cepstrum": (_i, [_p, _p, _p, _q, _p, _p, _i, _i, _i, _i, _i, _d, _i, _i, _p]),
    "ssspy_hva_dual_step": (_i, [_p, _p, _p, _q, _p, _d, _d, _i, _i, _i, _i, _p]),
    "ssspy_hva_admm_cepstrum": (_i, [_p, _p, _p, _p, _q, _p, _p, _i, _i, _i, _i, _d, _i, _d, _i, _i,
                                     _p]),
    "ssspy_hva_aux_step": (_i, [_p, _p, _p, _p, _q, _p, _d, _d, _i, _i, _i, _i, _p]),
    "ssspy_fast_iva_weights": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _d, _p]),
    "ssspy_fast_iva_stats": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "ssspy_fast_iva_step": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _p]),
    "ssspy_faster_iva_step": (_i, [_p, _p, _i, _i, _i, _p, _p]),
    "ssspy_orthonormalize_rows": (_i, [_p, _i, _i, _i, _p, _p]),
    "ssspy_whitening_filter": (_i, [_p, _p, _i, _i, _i, _i, _p, _p]),
    "ssspy_ipsdta_frame_pass": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i,
                                     _p, _p, _p, _p]),
    "ssspy_ipsdta_weight_loss": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _d, _p, _p, _p]),
    "ssspy_ipsdta_activation": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "ssspy_ipsdta_normalize": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "ssspy_ipsdta_vcd": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _d, _p, _p]),
    "ssspy_matmul3": (_i, [_p, _p, _p, _p, _q, _i, _p]),
    "ssspy_ipsdta_reconstruct": (_i, [_p, _p, _p, _q, _i, _i, _i, _i, _i, _i, _d, _p]),
    "ssspy_softmax": (_i, [_p, _p, _q, _i, _q, _p]),
    "ssspy_logsumexp": (_i, [_p, _p, _q, _i, _q, _p]),
    "ssspy_quadratic": (_i, [_p, _p, _p, _q, _i, _p]),
    "ssspy_cacgmm_unit_input": (_i, [_p, _p, _i, _i, _i, _i, _i, _d, _p]),
    "ssspy_cacgmm_prepare": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _p]),
    "ssspy_cacgmm_frame_pass": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _d, _p, _p, _p, _p, _p,
                                     _p]),
    "ssspy_cacgmm_parameter_step": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _d, _i, _p]),
    "ssspy_cacgmm_normalize": (_i, [_p, _i, _i, _i, _i, _p]),
    "ssspy_cacgmm_fold_loss": (_i, [_p, _p, _q, _i, _p]),
    "ssspy_cacgmm_separate": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "ssspy_permutation_route": (_i, [_i, _i, _i, _i]),
    "ssspy_best_permutation": (_i, [_p, _p, _q, _i, _p]),
    "ssspy_permutation_envelope_overlap": (_i, [_p, _i, _q, _q, _q, _p, _p, _i, _i, _i, _i, _i, _d,
                                                _p]),
    "ssspy_permutation_correlation_sweep": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "ssspy_permutation_score_normalize": (_i, [_p, _q, _q, _q, _p, _i, _i, _i, _i, _p]),
    "ssspy_permutation_score_global": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _d, _p]),
    "ssspy_permutation_score_local": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _d, _p]),
    "ssspy_permute_sources": (_i, [_p, _p, _p, _i, _i, _i, _q, _i, _q, _q, _q, _p]),
    "ssspy_permutation_amplitude": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "ssspy_gmnmf_workspace_bytes": (_z, [_i, _i, _i, _i, _i, _i]),
    "ssspy_gmnmf_route": (_i, [_i, _i, _i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int)]),
    "ssspy_gmnmf_update": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _d, _p, _z, _p]),
    "ssspy_gmnmf_loss_workspace_bytes": (_z, [_i, _i, _i]),
    "ssspy_gmnmf_loss": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _d, _p, _z, _p]),
    "ssspy_gmnmf_separate": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _d, _p]),
    "ssspy_eigh_general": (_i, [_p, _p, _p, _p, _q, _i, _i, _p, _p]),
    "ssspy_sqrtmh": (_i, [_p, _p, _q, _i, _i, _i, _d, _p]),
    "ssspy_gmeanmh": (_i, [_p, _p, _p, _q, _i, _i, _p]),
    "ssspy_lqpqm2": (_i, [_p, _p, _p, _p, _q, _i, _i, _i, _d, _p, _p, _p]),
    "ssspy_lqpqm2_masked": (_i, [_p, _p, _p, _p, _q, _i, _i, _i, _d, _p, _p, _p, _p]),
    "ssspy_stft_frames": (_i, [_q, _i, _i]),
    "ssspy_stft_workspace_bytes": (_z, [_i]),
    "ssspy_stft": (_i, [_p, _p, _p, _d, _i, _i, _q, _i, _i, _p, _p]),
    "ssspy_istft_samples": (_q, [_i, _i, _i]),
    "ssspy_istft": (_i, [_p, _p, _p, _d, _p, _i, _i, _i, _i, _i, _p, _p]),
    "ssspy_fastmnmf_workspace_bytes": (_z, [_i, _i, _i, _i, _i, _i]),
    "ssspy_fastmnmf_update": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _d, _p,
                                   _z, _p, _p]),
    "ssspy_fastmnmf_handover_doubles": (_z, [_i, _i, _i, _i, _i, _i]),
    "ssspy_fastmnmf_update_handover": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _d,
                                            _p, _z, _p, _p, _p, _p]),
    "ssspy_fastmnmf_deferred_logdet_slots": (_i, [_i, _i, _i, _i, _i, _i]),
    "ssspy_fastmnmf_update_handover_logdet": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i,
                                                   _i, _d, _p, _z, _p, _p, _p, _p, _q, _p]),
    "ssspy_fastmnmf_loss_handover_slots": (_i, [_i, _i, _i, _i, _i, _i]),
    "ssspy_fastmnmf_route": (_i, [_i, _i, _i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int)]),
    "ssspy_fastmnmf_loss_data_handover_slots": (_i, [_p, _p, _p, _p, _p, _q, _i, _i, _i, _i, _i, _i,
                                                     _p]),
    "ssspy_fastmnmf_loss_data_handover": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _z,
                                               _p]),
    "ssspy_fastmnmf_loss_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "ssspy_fastmnmf_diagonalizer_covariance": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p,
                                                    _z, _p]),
    "ssspy_fastmnmf_loss_data": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _z, _p]),
    "ssspy_fastmnmf_weights": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "ssspy_fastmnmf_separate": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _d, _p,
                                     _z, _p, _p]),
    "ssspy_fastmnmf_separate_eig": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p,
                                         _p, _p, _z, _p, _p]),
}
GMNMF_BASIS, GMNMF_ACTIVATION, GMNMF_SPATIAL, GMNMF_NORMALIZE, GMNMF_ALL = 1, 2, 4, 8, 15
GMNMF_LATENT = 16
MNMF_BASIS, MNMF_ACTIVATION, MNMF_DIAGONALIZER, MNMF_SPATIAL, MNMF_NORMALIZE, MNMF_ALL = 1, 2, 4, 8, 16, 31

_lib = None


class HipLibraryError(RuntimeError):
    """libssspy_amd.so is missing, fails to load, or an entry point returned an error."""


def load():
    """Load the shared library (once) and attach the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            "{} not found: build it with `python -m ssspy_amd._build` "
            "(there is no CPU fallback for the device path)".format(LIB_PATH)
        )
    try:
        lib = ctypes.CDLL(LIB_PATH, mode=os.RTLD_NOW)  # unresolved symbols fail here, not at first call
    except OSError as e:  # e.g. libamdhip64 missing
        raise HipLibraryError("cannot load {}: {}".format(LIB_PATH, e)) from e
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.ssspy_abi_version() != ABI_VERSION:
        raise HipLibraryError(
            "{} implements ABI version {}, this binding was written against {}: rebuild it with "
            "`python -m ssspy_amd._build`".format(LIB_PATH, lib.ssspy_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what=""):
    """Translate a C-ABI status into the Python exception the reference would raise."""
    if rc == OK:
        return
    msg = load().ssspy_last_error().decode()
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError("{}: {}".format(what, msg))
    if rc == ERR_BADARG:
        raise ValueError("{}: {}".format(what, msg))
    raise HipLibraryError("{}: {} (status {})".format(what, msg, rc))


def raise_if_singular(count, what):
    """Device kernels count singular per-bin systems; the reference raises LinAlgError."""
    if count:
        raise np.linalg.LinAlgError("Singular matrix ({} bin(s) in {})".format(int(count), what))


def raise_if_barrier_timeouts():
    """The fused IPA sweeps count the times a workgroup gave up waiting for its mixture's others
    (ssspy_debug_barrier_timeouts); its vote was then partial."""
    timeouts = load().ssspy_debug_barrier_timeouts()
    if timeouts:
        raise HipLibraryError(
            "an IPA sweep gave up waiting for its mixture's workgroups {} time(s): the "
            "results of this process are not to be trusted".format(timeouts))
