"""ctypes binding of libatlasqtl_hip.so (the C ABI of include/atlasqtl_hip.h).

The library is the product: there is no Python or CPU fallback.  If the shared
object is missing, or no HIP device is visible when a compute entry is called,
the error is raised loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AQ_LIB", os.path.join(_HERE, "libatlasqtl_hip.so"))

AQ_OK = 0
AQ_VB_DONE = 0
AQ_VB_NEED_ALLREDUCE_MAIN = 1
AQ_VB_NEED_ALLREDUCE_ELBO = 2

dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)


class AqVbProblem(C.Structure):
    _fields_ = [
        ("n", C.c_int32), ("p", C.c_int32), ("q", C.c_int32), ("q_total", C.c_int32),
        ("X", dp), ("Y", dp),
        ("A2_inv", C.c_double), ("m0", C.c_double), ("nu", C.c_double), ("rho", C.c_double), ("t02", C.c_double),
        ("eta", dp), ("kappa", dp), ("n0", dp),
        ("gam_vb", dp), ("mu_beta_vb", dp), ("sig02_inv_vb", C.c_double), ("sig2_beta_vb", dp),
        ("sig2_theta_vb", dp), ("tau_vb", dp), ("theta_vb", dp), ("zeta_vb", dp),
        ("has_anneal", C.c_int32), ("anneal", C.c_double * 3), ("tol", C.c_double), ("maxit", C.c_int32),
        ("thinned_elbo_eval", C.c_int32), ("debug", C.c_int32),
        ("device", C.c_int32), ("world_size", C.c_int32),
        ("ext_reduce_main", C.c_void_p), ("ext_reduce_elbo", C.c_void_p), ("init_on_device", C.c_int32),
        ("init_generate", C.c_int32), ("trait_offset", C.c_int32), ("init_seed", C.c_uint64),
        ("init_gam_mean", C.c_double), ("init_gam_sd", C.c_double),
        ("xy_on_device", C.c_int32), ("scheme", C.c_int32), ("df", C.c_int32),
    ]


class AqPrepInput(C.Structure):
    _fields_ = [("n", C.c_int32), ("p", C.c_int32), ("q", C.c_int32), ("X", dp), ("X_i8", C.POINTER(C.c_int8)), ("Y", dp),
                ("device", C.c_int32)]


class AqPrepBedInput(C.Structure):
    _fields_ = [("n_file", C.c_int32), ("n", C.c_int32), ("p", C.c_int32), ("q", C.c_int32), ("bed", C.POINTER(C.c_uint8)),
                ("sample_idx", ip), ("Y", dp), ("count_a2", C.c_int32), ("missing", C.c_int32), ("device", C.c_int32)]


class AqPrepCov(C.Structure):
    _fields_ = [("d", C.c_int32), ("Z", dp)]


class AqPrepLd(C.Structure):
    _fields_ = [("window", C.c_int32), ("r2", C.c_double), ("group", ip), ("pos", C.POINTER(C.c_int64)), ("window_bp", C.c_int64)]


class AqGrmPlan(C.Structure):
    _fields_ = [("tile", C.c_int32), ("tiles_per_edge", C.c_int32), ("n_tiles", C.c_int32), ("splits", C.c_int32),
                ("chunk", C.c_int32), ("chunks_per_split", C.c_int32), ("scratch_bytes", C.c_int64), ("k_bytes", C.c_int64)]


class AqPcsPlan(C.Structure):
    _fields_ = [("lp", C.c_int32), ("panel", C.c_int32), ("n_panels", C.c_int32), ("sample_chunk", C.c_int32), ("n_pad", C.c_int32),
                ("tile", C.c_int32), ("n_tiles", C.c_int32), ("splits", C.c_int32), ("chunk", C.c_int32),
                ("chunks_per_split", C.c_int32), ("t_bytes", C.c_int64), ("scratch_bytes", C.c_int64), ("io_bytes", C.c_int64)]


class AqPrepYtrans(C.Structure):
    _fields_ = [("method", C.c_int32), ("offset", C.c_double)]


class AqYtransPlan(C.Structure):
    _fields_ = [("path", C.c_int32), ("n_pad", C.c_int32), ("lds_bytes", C.c_int32), ("traits_per_batch", C.c_int32),
                ("scratch_bytes", C.c_int64)]


class AqMscreenPlan(C.Structure):
    _fields_ = [("tile", C.c_int32), ("sample_chunk", C.c_int32), ("tiles_p", C.c_int32), ("tiles_q", C.c_int32), ("masked", C.c_int32),
                ("lds_bytes", C.c_int32), ("n_tiles", C.c_int64), ("scratch_bytes", C.c_int64)]


class AqMspermPlan(C.Structure):
    _fields_ = [("tile", C.c_int32), ("pb", C.c_int32), ("batch", C.c_int32), ("launches", C.c_int32), ("tiles_p", C.c_int32),
                ("tiles_q", C.c_int32), ("masked", C.c_int32), ("lds_bytes", C.c_int32), ("yp_bytes", C.c_int64),
                ("scratch_bytes", C.c_int64)]


class AqCisPlan(C.Structure):
    _fields_ = [("tile", C.c_int32), ("sample_chunk", C.c_int32), ("trait_tiles", C.c_int32), ("q_active", C.c_int32),
                ("masked", C.c_int32), ("lds_bytes", C.c_int32), ("perm_lds_bytes", C.c_int32), ("pb", C.c_int32), ("batch", C.c_int32),
                ("launches", C.c_int32), ("n_items", C.c_int64), ("window_pairs", C.c_int64), ("staged_pairs", C.c_int64),
                ("yp_bytes", C.c_int64), ("scratch_bytes", C.c_int64)]


class AqCiscondPlan(C.Structure):
    _fields_ = [("cis", AqCisPlan), ("kc", C.c_int32), ("max_k", C.c_int32), ("lds_bytes", C.c_int32), ("streams", C.c_int32),
                ("qo_bytes", C.c_int64), ("yo_bytes", C.c_int64)]


class AqCisintPlan(C.Structure):
    _fields_ = [("cis", AqCisPlan), ("streams", C.c_int32), ("n_basis", C.c_int32), ("lds_bytes", C.c_int32), ("mult_pad", C.c_int32),
                ("yo_bytes", C.c_int64), ("pred_bytes", C.c_int64), ("basis_bytes", C.c_int64)]


class AqFinemapParams(C.Structure):
    _fields_ = [("L", C.c_int32), ("max_iter", C.c_int32), ("tol", C.c_double), ("scaled_prior_variance", C.c_double),
                ("coverage", C.c_double), ("alpha_min", C.c_double)]


class AqFinemapPlan(C.Structure):
    _fields_ = [("cis", AqCisPlan), ("L", C.c_int32), ("batch_tiles", C.c_int32), ("n_batches", C.c_int32), ("forced", C.c_int32),
                ("state_budget", C.c_int64), ("state_bytes", C.c_int64), ("band_bytes", C.c_int64), ("fit_bytes", C.c_int64)]


class AqPredictPlan(C.Structure):
    _fields_ = [("sample_tiles", C.c_int32), ("trait_tiles", C.c_int32), ("sample_blocks", C.c_int32), ("trait_groups", C.c_int32),
                ("splits", C.c_int32), ("chunk", C.c_int32), ("chunks_per_split", C.c_int32), ("n_pad", C.c_int32),
                ("panel_bytes", C.c_int64), ("scratch_bytes", C.c_int64)]


AQ_N_MAX = 82944          # most samples of one handle, and most rows of one aq_vb_predict call (csrc/aq_plan_const.h)


class AqVbMultiOut(C.Structure):
    _fields_ = [
        ("beta_vb", dp), ("gam_vb", dp), ("mu_beta_vb", dp), ("theta_vb", dp), ("zeta_vb", dp), ("lam2_inv_vb", dp),
        ("sig2_theta_vb", dp), ("tau_vb", dp), ("sig2_beta_vb", dp), ("elbo_it", ip), ("elbo_lb", dp), ("elbo_cap", C.c_int32),
        ("n_elbo", C.c_int32), ("it", C.c_int32), ("converged", C.c_int32), ("lb_opt", C.c_double), ("diff_lb", C.c_double),
        ("sig02_inv_vb", C.c_double), ("sig2_inv_vb", C.c_double), ("seconds", C.c_double), ("core_ms", C.c_double),
    ]


class AqMoments(C.Structure):
    _fields_ = [("count", C.c_int64), ("n_nan", C.c_int64), ("min", C.c_double), ("max", C.c_double), ("sum", C.c_double)]


AQ_RSEL_BITS = 8          # digit width of the radix select (include/atlasqtl_hip.h)
AQ_RSEL_MAX_PREFIX = 16


class AqVbStatus(C.Structure):
    _fields_ = [
        ("it", C.c_int32), ("converged", C.c_int32), ("lb_opt", C.c_double), ("diff_lb", C.c_double),
        ("c", C.c_double), ("annealing", C.c_int32), ("n_elbo", C.c_int32), ("core_ms", C.c_double),
        ("core_launches", C.c_int32), ("sig02_inv_vb", C.c_double), ("sig2_inv_vb", C.c_double),
        ("lentz_iters", C.c_int32), ("core_kernel", C.c_int32), ("split_parts", C.c_int32),
        ("tiles_per_group", C.c_int32), ("chain_segments", C.c_int32),
        # the launched instance of the core kernel (appended fields): NT, NT2, NT3, flags (1 MASK, 2 WIDE, 4 chained), padded n
        ("tiles_matrix", C.c_int32), ("tiles_matrix2", C.c_int32), ("tiles_recurrence", C.c_int32),
        ("instance_flags", C.c_int32), ("n_pad", C.c_int32),
    ]


class AqKernelInstance(C.Structure):
    """aq_kernel_instance: the template parameters of a compiled core-kernel instance (aq_instance_query)."""
    _fields_ = [(k, C.c_int32) for k in ("core_kernel", "nt", "nt2", "seg", "tt", "mask", "nt3", "wide", "ne", "wpt")]


# every symbol include/atlasqtl_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "aq_last_error": (C.c_char_p, []),
    "aq_version": (C.c_char_p, []),
    "aq_device_count": (C.c_int, []),
    "aq_core_dual_loop": (C.c_int, [dp, dp, dp, dp, dp, C.c_double, dp, dp, dp, dp, dp, dp, ip, C.c_int32, ip,
                                    C.c_int32, C.c_double, C.c_int32, C.c_int32]),
    "aq_core_dual_mis_loop": (C.c_int, [dp, C.POINTER(dp), dp, dp, dp, dp, C.c_double, dp, dp, dp, dp, dp, dp, ip,
                                        C.c_int32, ip, C.c_int32, C.c_double, C.c_int32, C.c_int32]),
    "aq_vb_reduce_len": (C.c_int64, [C.c_int32]),
    "aq_vb_create": (C.c_int, [C.POINTER(AqVbProblem), C.POINTER(C.c_void_p)]),
    "aq_vb_destroy": (None, [C.c_void_p]),
    "aq_vb_advance": (C.c_int, [C.c_void_p]),
    "aq_vb_reduce_ptr": (C.c_void_p, [C.c_void_p, C.c_int32]),
    "aq_vb_set_sweep_budget": (C.c_int, [C.c_void_p, C.c_int32]),
    "aq_vb_run": (C.c_int, [C.c_void_p]),
    "aq_vb_run_sweeps": (C.c_int, [C.c_void_p, C.c_int32]),
    "aq_vb_get_status": (C.c_int, [C.c_void_p, C.POINTER(AqVbStatus)]),
    "aq_vb_get_overrides": (C.c_int32, [C.c_void_p, C.c_char_p, C.c_int32]),
    "aq_plan_query": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_char_p,
                                C.POINTER(AqVbStatus)]),
    "aq_instance_query": (C.c_int, [C.POINTER(AqVbStatus), C.c_int32, C.c_int32, C.POINTER(AqKernelInstance)]),
    "aq_vb_get_elbo_trace": (C.c_int32, [C.c_void_p, ip, dp, C.c_int32]),
    "aq_vb_get_result": (C.c_int, [C.c_void_p, dp, dp, dp, dp, dp, dp, dp, dp, dp]),
    "aq_vb_run_multi": (C.c_int, [C.POINTER(AqVbProblem), C.c_int32, ip, C.c_int32, C.POINTER(AqVbMultiOut)]),
    "aq_vb_partition": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, ip, ip]),
    "aq_vb_get_residual": (C.c_int, [C.c_void_p, dp]),
    "aq_prepare_data": (C.c_int, [C.POINTER(AqPrepInput), C.POINTER(C.c_void_p)]),
    "aq_prep_info": (C.c_int, [C.c_void_p, ip, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), ip, dp, dp]),
    "aq_prep_x_device": (C.c_void_p, [C.c_void_p]),
    "aq_prep_y_device": (C.c_void_p, [C.c_void_p]),
    "aq_prep_get": (C.c_int, [C.c_void_p, dp, dp]),
    "aq_prep_destroy": (None, [C.c_void_p]),
    "aq_assign_bfdr": (C.c_int, [dp, dp, C.c_int64, C.c_int32]),
    "aq_hotspot_sizes": (C.c_int, [dp, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int64), C.c_int32]),
    "aq_vb_hotspot_sizes": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "aq_vb_bfdr_begin": (C.c_int, [C.c_void_p]),
    "aq_vb_bfdr_query": (C.c_int, [C.c_void_p, C.c_double, dp]),
    "aq_vb_bfdr_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    "aq_vb_bfdr_end": (None, [C.c_void_p]),
    "aq_vb_select_pairs": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, C.c_int64, ip, ip, dp, dp, dp, C.POINTER(C.c_int64)]),
    "aq_select_pairs": (C.c_int, [dp, dp, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int64, ip, ip, dp, dp, dp,
                                  C.POINTER(C.c_int64), C.c_int32]),
    "aq_vb_bfdr_pairs": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, ip, ip, dp, dp]),
    "aq_vb_radix_hist": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint64), C.c_int32, C.POINTER(C.c_int64)]),
    "aq_vb_moments": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(AqMoments)]),
    "aq_vb_order_stats": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), dp, C.POINTER(AqMoments)]),
    "aq_order_stats": (C.c_int, [dp, C.c_int64, C.c_int32, C.POINTER(C.c_int64), dp, C.POINTER(AqMoments), C.c_int32]),
    "aq_vb_state_bytes": (C.c_int64, [C.c_void_p]),
    "aq_vb_get_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "aq_vb_set_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "aq_special_eval": (C.c_int, [C.c_int32, dp, dp, dp, C.c_int64]),
    "aq_special_eval_device": (C.c_int, [C.c_int32, dp, dp, dp, C.c_int64, C.c_int32]),
    "aq_q_approx_vec": (C.c_int, [dp, dp, C.c_int64, ip]),
    "aq_vb_debug_raise_errflag": (C.c_int, [C.c_void_p]),
    "aq_debug_live_device_bytes": (C.c_int64, []),
    "aq_prep_debug_set_column": (C.c_int, [C.c_void_p, C.c_int32, dp]),
    "aq_vb_debug_get_setup": (C.c_int64, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]),
    "aq_prepare_data_bed": (C.c_int, [C.POINTER(AqPrepBedInput), C.POINTER(C.c_void_p)]),
    "aq_prep_genotype_counts": (C.c_int, [C.c_void_p, ip]),
    "aq_prepare_data_cov": (C.c_int, [C.POINTER(AqPrepInput), C.POINTER(AqPrepCov), C.POINTER(C.c_void_p)]),
    "aq_prepare_data_bed_cov": (C.c_int, [C.POINTER(AqPrepBedInput), C.POINTER(AqPrepCov), C.POINTER(C.c_void_p)]),
    "aq_prep_cov_info": (C.c_int, [C.c_void_p, ip, C.POINTER(C.c_uint8), dp]),
    "aq_cov_basis": (C.c_int, [dp, C.c_int32, C.c_int32, dp, ip]),
    "aq_prep_ld_prune": (C.c_int, [C.c_void_p, C.POINTER(AqPrepLd)]),
    "aq_prep_ld_info": (C.c_int, [C.c_void_p, ip, C.POINTER(C.c_uint8), ip, dp]),
    "aq_prep_ld_band": (C.c_int, [C.c_void_p, C.c_int32, dp]),
    "aq_prep_grm": (C.c_int, [C.c_void_p, dp, dp]),
    "aq_grm_plan_query": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(AqGrmPlan)]),
    "aq_prep_grm_time": (C.c_int, [C.c_void_p, C.c_int32, dp, C.POINTER(AqGrmPlan)]),
    "aq_prep_grm_apply": (C.c_int, [C.c_void_p, dp, C.c_int32, dp, dp]),
    "aq_pcs_plan_query": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(AqPcsPlan)]),
    "aq_prep_grm_apply_time": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, dp, C.POINTER(AqPcsPlan)]),
    "aq_prepare_data_opt": (C.c_int, [C.POINTER(AqPrepInput), C.POINTER(AqPrepBedInput), C.POINTER(AqPrepCov), C.POINTER(AqPrepYtrans),
                                      C.POINTER(C.c_void_p)]),
    "aq_prep_ytrans_info": (C.c_int, [C.c_void_p, ip, dp, ip, ip]),
    "aq_rank_int": (C.c_int, [dp, C.c_int32, C.c_int32, C.c_double, dp, ip, ip, C.c_int32]),
    "aq_ytrans_plan_query": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.POINTER(AqYtransPlan)]),
    "aq_mscreen_plan_query": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(AqMscreenPlan)]),
    "aq_prep_marginal": (C.c_int, [C.c_void_p, dp, C.c_int64, ip, ip, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), ip, dp,
                                   C.POINTER(C.c_int64), dp]),
    "aq_prep_marginal_time": (C.c_int, [C.c_void_p, C.c_int32, dp, C.POINTER(AqMscreenPlan)]),
    "aq_msperm_plan_query": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(AqMspermPlan)]),
    "aq_prep_marginal_perm": (C.c_int, [C.c_void_p, dp, C.c_int32, ip, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int64)]),
    "aq_prep_marginal_perm_time": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, dp, C.POINTER(AqMspermPlan)]),
    "aq_cis_plan_query": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, ip, ip, C.c_int32, C.POINTER(AqCisPlan)]),
    "aq_prep_cis": (C.c_int, [C.c_void_p, ip, ip, dp, C.c_int64, ip, ip, dp, C.POINTER(C.c_int64), ip, dp, C.POINTER(C.c_int64),
                              C.POINTER(AqCisPlan)]),
    "aq_prep_cis_perm": (C.c_int, [C.c_void_p, ip, ip, C.c_int32, ip, dp]),
    "aq_prep_cis_time": (C.c_int, [C.c_void_p, ip, ip, C.c_int32, C.c_int32, dp, dp, C.POINTER(AqCisPlan)]),
    "aq_ciscond_plan_query": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, ip, ip, ip, C.POINTER(AqCiscondPlan)]),
    "aq_prep_cis_cond": (C.c_int, [C.c_void_p, ip, ip, ip, ip, dp, C.c_int64, ip, ip, dp, C.POINTER(C.c_int64), ip, dp,
                                   C.POINTER(C.c_int64), ip, C.POINTER(AqCiscondPlan)]),
    "aq_prep_cis_cond_time": (C.c_int, [C.c_void_p, ip, ip, ip, ip, C.c_int32, dp, dp, C.POINTER(AqCiscondPlan)]),
    "aq_cisint_plan_query": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, ip, ip, C.c_int32, C.POINTER(AqCisintPlan)]),
    "aq_prep_cis_int": (C.c_int, [C.c_void_p, ip, ip, dp, C.c_int32, dp, dp, C.c_int64, ip, ip, dp, C.POINTER(C.c_int64), ip, dp,
                                  C.POINTER(C.c_int64), dp, C.POINTER(AqCisintPlan)]),
    "aq_prep_cis_int_time": (C.c_int, [C.c_void_p, ip, ip, dp, C.c_int32, dp, C.c_int32, dp, dp, C.POINTER(AqCisintPlan)]),
    "aq_finemap_plan_query": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, ip, ip, C.c_int32, C.POINTER(AqFinemapPlan)]),
    "aq_prep_cis_finemap": (C.c_int, [C.c_void_p, ip, ip, ip, C.POINTER(AqFinemapParams), C.c_int64, ip, ip, ip, dp, dp, dp,
                                      C.POINTER(C.c_int64), dp, dp, dp, dp, ip, ip, C.POINTER(C.c_int64), dp, dp,
                                      C.POINTER(AqFinemapPlan)]),
    "aq_prep_set_purity": (C.c_int, [C.c_void_p, ip, ip, C.c_int32, dp, dp]),
    "aq_prep_cis_finemap_time": (C.c_int, [C.c_void_p, ip, ip, C.c_int32, C.c_int32, dp, dp, dp, dp, C.POINTER(AqFinemapPlan)]),
    "aq_predict_plan_query": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(AqPredictPlan)]),
    "aq_vb_predict": (C.c_int, [C.c_void_p, dp, C.POINTER(C.c_int8), C.c_int32, dp, dp, dp]),
    "aq_vb_fitted": (C.c_int, [C.c_void_p, C.c_void_p, dp]),
    "aq_predict": (C.c_int, [dp, C.c_int32, C.c_int32, dp, C.POINTER(C.c_int8), C.c_int32, dp, dp, dp, C.c_int32]),
    "aq_vb_predict_time": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, dp, C.POINTER(AqPredictPlan)]),
}

_lib = None


class AtlasqtlHipError(RuntimeError):
    pass


def lib():
    """Load libatlasqtl_hip.so; raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AtlasqtlHipError(f"{LIB_PATH} not found: build it first (python -c 'import __graft_entry__ as g; "
                                   "g.build()' or make -C atlasqtl_amd/csrc). There is no CPU fallback.")
        # PyTorch (used for device tensors and the collectives of ranks.py) ships its own copy of the HIP runtime.  If it is loaded AFTER this
        # library has initialised the system copy, torch.cuda no longer finds a device ("No HIP GPUs are available"); loaded first,
        # both live together.  So: torch first, when it is installed.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != AQ_OK:
        msg = lib().aq_last_error().decode("utf-8", "replace")
        raise AtlasqtlHipError(f"{what}: [{rc}] {msg}" if what else f"[{rc}] {msg}")


def as_dp(a):
    return a.ctypes.data_as(dp)


def as_ip(a):
    return a.ctypes.data_as(ip)
