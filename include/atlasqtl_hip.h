/*
 * atlasqtl_hip.h -- C ABI of libatlasqtl_hip.so, the MI355X (gfx950) implementation of
 * atlasqtl's variational-inference hot path.  Plain C: pointers + sizes, int status
 * returns (0 = ok), thread-local message via aq_last_error().  No torch / R types.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repository hruffieux/atlasqtl @ v0.1.5).  INTEGRATION.md shows the R-side
 * binding (a .Call shim) a maintainer would add.
 *
 * All matrices are R layout: column-major fp64; indices are 0-based int32.
 */
#ifndef ATLASQTL_HIP_H_
#define ATLASQTL_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQ_OK 0
#define AQ_ERR_ARG 1        /* bad argument (NULL, size, range) -- where the reference would stop()        */
#define AQ_ERR_DEVICE 2     /* no gfx950 device / HIP runtime error                                        */
#define AQ_ERR_UNSUPPORTED 3
#define AQ_ERR_NUMERIC 4    /* "ELBO not increasing monotonically" (R/atlasqtl_global_local_core.R:359-360) */

/* Message of the last failing call on this thread ("" if none). */
const char *aq_last_error(void);
/* Library version string. */
const char *aq_version(void);
/* Number of visible HIP devices (0 on a CPU-only host; never fails). */
int aq_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Operator-level entries: drop-in for the two native functions of the reference.
 *
 * aq_core_dual_loop replaces
 *     SEXP _atlasqtl_coreDualLoop(SEXP x 15)                    src/RcppExports.cpp:17-38
 *     void coreDualLoop(...)                                    src/coreLoop.cpp:38-86
 * Same positional arguments (plus explicit sizes); cp_Y_X is q x p.  gam_vb, m1_beta,
 * cp_betaX_X and mu_beta_vb (each p x q) are updated IN PLACE in the caller's host buffers,
 * exactly as the reference mutates the R objects it is handed (src/RcppExports.cpp:22,27-29).
 * Host pointers in, host pointers out; the arithmetic runs on the GPU in the reference's
 * own Gram-space form and visiting order.  Indices are range-checked (AQ_ERR_ARG) where the
 * reference has undefined behaviour.
 * ---------------------------------------------------------------------------------------- */
int aq_core_dual_loop(const double *cp_X, const double *cp_Y_X, double *gam_vb,
                      const double *log_Phi_theta_plus_zeta, const double *log_1_min_Phi_theta_plus_zeta,
                      double log_sig2_inv_vb, const double *log_tau_vb, double *m1_beta, double *cp_betaX_X,
                      double *mu_beta_vb, const double *sig2_beta_vb /* q */, const double *tau_vb,
                      const int32_t *shuffled_ind, int32_t n_ind, const int32_t *sample_q, int32_t n_q, double c,
                      int32_t p, int32_t q);

/* aq_core_dual_mis_loop replaces
 *     SEXP _atlasqtl_coreDualMisLoop(SEXP x 16)                 src/RcppExports.cpp:41-62
 *     void coreDualMisLoop(...)                                 src/coreLoop.cpp:91-138
 * cp_X_rm: array of q pointers to p x p matrices (the reference's R list); sig2_beta_vb is p x q. */
int aq_core_dual_mis_loop(const double *cp_X, const double *const *cp_X_rm, const double *cp_Y_X, double *gam_vb,
                          const double *log_Phi_theta_plus_zeta, const double *log_1_min_Phi_theta_plus_zeta,
                          double log_sig2_inv_vb, const double *log_tau_vb, double *m1_beta, double *cp_betaX_X,
                          double *mu_beta_vb, const double *sig2_beta_vb /* p x q */, const double *tau_vb,
                          const int32_t *shuffled_ind, int32_t n_ind, const int32_t *sample_q, int32_t n_q,
                          double c, int32_t p, int32_t q);

/* ------------------------------------------------------------------------------------------
 * Whole-run entries: the device-resident replacement of
 *     atlasqtl_global_local_core_(Y, X, shr_fac_inv, anneal, df, tol, maxit, verbose,
 *                                 list_hyper, list_init, ...)   R/atlasqtl_global_local_core.R:8-433
 * (its `while` loop :125-386 incl. elbo_global_local_ :440-495).  X must be the standardised
 * matrix and Y the centred matrix that prepare_data_ (R/prepare_atlasqtl.R:57-83) produces.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_vb *aq_vb_handle;

typedef struct aq_vb_problem {
  int32_t n, p;
  int32_t q;            /* traits held by THIS process (columns of Y given here)                     */
  int32_t q_total;      /* traits of the whole problem (= q on one GPU); shr_fac_inv = q_total        */
  const double *X;      /* n x p, standardised, no NaN                                                */
  const double *Y;      /* n x q, centred; NaN = missing (R/atlasqtl_global_local_core.R:19-22)       */
  /* list_hyper fields (R/set_hyper_init.R:133-134) */
  double A2_inv, m0, nu, rho, t02;
  const double *eta;    /* q */
  const double *kappa;  /* q */
  const double *n0;     /* q */
  /* list_init fields (R/set_hyper_init.R:344-346) */
  const double *gam_vb;        /* p x q */
  const double *mu_beta_vb;    /* p x q */
  double sig02_inv_vb;
  const double *sig2_beta_vb;  /* q */
  const double *sig2_theta_vb; /* p */
  const double *tau_vb;        /* q */
  const double *theta_vb;      /* p */
  const double *zeta_vb;       /* q */
  /* control (R/atlasqtl.R:179-184) */
  int32_t has_anneal;          /* 0 = anneal NULL */
  double anneal[3];            /* type (1 geometric, 2 harmonic, 3 linear), initial temperature, ladder size */
  double tol;
  int32_t maxit;
  int32_t thinned_elbo_eval;
  int32_t debug;               /* 1: non-monotone ELBO -> AQ_ERR_NUMERIC, as the reference's stop()  */
  /* placement */
  int32_t device;              /* HIP device ordinal */
  int32_t world_size;          /* number of cooperating processes (q-sharding); 1 = single GPU       */
  double *ext_reduce_main;     /* optional DEVICE buffer of aq_vb_reduce_len() doubles owned by the
                                  caller (e.g. a torch tensor) used as the all-reduce payload; NULL =
                                  the library allocates it                                            */
  double *ext_reduce_elbo;     /* optional DEVICE buffer of 8 doubles, same purpose                   */
  int32_t init_on_device;      /* 1: gam_vb and mu_beta_vb are DEVICE pointers (p x q column-major) on
                                  `device`; avoids staging 2 x 8pq bytes through the host              */
  /* SURVEY 8f N1 -- the p x q initial values of auto_set_init_ (R/set_hyper_init.R:385-387) drawn ON the
   * device: gam_vb = pnorm(N(init_gam_mean, sd = init_gam_sd)), mu_beta_vb = N(0, 1), from Philox4x32-10 keyed by
   * init_seed with counter (SNP index, trait_offset + local trait index): the draws of a trait do not depend
   * on how the traits are sharded.  gam_vb and mu_beta_vb may then be NULL.                                  */
  int32_t init_generate;
  int32_t trait_offset;        /* global index of this process's first trait (0 on one GPU)              */
  uint64_t init_seed;
  double init_gam_mean, init_gam_sd;
  int32_t xy_on_device;        /* bit 0: X is a DEVICE pointer on `device` (e.g. aq_prep_x_device of aq_prepare_data), taken as
                                  standardised and NaN-free without a host pass; bit 1: Y is a DEVICE pointer (aq_prep_y_device) */
  /* SURVEY 8f N4 -- the other drivers over the same sweep:
   *   scheme 0  atlasqtl_global_local_core_ (horseshoe, R/atlasqtl_global_local_core.R); df = 0 or 1: half-Cauchy local scales;
   *             df = 3 (R/atlasqtl_global_local_core.R:258, R/elbo.R:95-105) and df = 5, 7 (compute_integral_hs_, R/utils.R:425-568;
   *             :260-272, R/elbo.R:107-124) without annealing; other df: AQ_ERR_UNSUPPORTED
   *   scheme 1  atlasqtl_global_core_ (one global scale, R/atlasqtl_global_core.R:117-320); sig2_theta_vb of list_init and
   *             A2_inv are not used there                                                                               */
  int32_t scheme;
  int32_t df;
} aq_vb_problem;

/* Length (in doubles) of the main all-reduce payload for a problem with p predictors:
 * [ rowSums(Z) (p padded to 16) , sum(gam) , sum_k tau_k colSums(m2)_k , sum(zeta) , 5 spare ]. */
int64_t aq_vb_reduce_len(int32_t p);

/* Creates the device state of one VB run.  n may be at most 82 944 (AQ_N_MAX): beyond 10 240 samples the sweep runs as the
 * wide sample split of the look-ahead kernel (9 ... 48 workgroups per trait group); larger n, or a problem whose operand panels
 * or per-trait Gram blocks (Y with missing values) do not fit in device memory, is AQ_ERR_UNSUPPORTED with the reason. */
int aq_vb_create(const aq_vb_problem *prob, aq_vb_handle *out);
void aq_vb_destroy(aq_vb_handle h);

/* State machine for the q-sharded multi-process run.  aq_vb_advance runs device work until a
 * collective is needed or the run is over and returns one of the codes below (<0: error, see
 * aq_last_error).  On AQ_VB_NEED_ALLREDUCE_MAIN / _ELBO the caller must SUM-all-reduce the
 * corresponding device buffer (aq_vb_reduce_ptr) across processes on the same stream order
 * (the library issues all work on the legacy default stream) and call aq_vb_advance again.
 * With world_size == 1 the codes may simply be ignored (aq_vb_run does that). */
#define AQ_VB_DONE 0
#define AQ_VB_NEED_ALLREDUCE_MAIN 1
#define AQ_VB_NEED_ALLREDUCE_ELBO 2
int aq_vb_advance(aq_vb_handle h);
/* which: 0 = main payload (aq_vb_reduce_len doubles), 1 = ELBO payload (8 doubles). */
double *aq_vb_reduce_ptr(aq_vb_handle h, int32_t which);

/* Limit the number of further sweeps aq_vb_advance may start (-1 = no limit); when the budget is
 * used up aq_vb_advance returns AQ_VB_DONE although the run is not over, and a later budget resumes it.
 * bench.py uses it to time exactly K sweeps on N processes. */
int aq_vb_set_sweep_budget(aq_vb_handle h, int32_t sweeps);

/* Single-process convenience: loops aq_vb_advance until AQ_VB_DONE (world_size must be 1). */
int aq_vb_run(aq_vb_handle h);
/* Runs at most max_sweeps further sweeps (stops earlier on convergence / maxit); world_size 1.
 * Used by bench.py to time exactly K sweeps. */
int aq_vb_run_sweeps(aq_vb_handle h, int32_t max_sweeps);

/* ------------------------------------------------------------------------------------------
 * The whole run on several GPUs of one node from ONE host process (`aq_vb_run(handle, ..., n_gpus)`), for
 * hosts without torch.distributed -- the reference's host is R, which calls the core once, single-threaded
 * (R/atlasqtl.R:274-278).  `prob` describes the WHOLE problem (q == q_total, host pointers; init_generate = 1 is allowed and
 * reproduces the single-GPU draws); the library cuts the trait axis into whole 16-trait tiles (aq_vb_partition), runs one host
 * thread and one handle per GPU and SUM-all-reduces the two small payloads of the aq_vb_advance protocol itself:
 *   transport 0  RCCL over xGMI (librccl.so is loaded at run time; distinct devices),
 *   transport 1  staged through host memory in fixed rank order (no RCCL; devices may repeat -- a one-GPU box can rehearse it).
 * devices: n_gpus HIP ordinals, or NULL for 0 .. n_gpus-1.  Results are gathered into the caller's host buffers of aq_vb_multi_out
 * (p x q column-major / q- and p-vectors; any pointer may be NULL).  Errors of any rank (e.g. AQ_ERR_NUMERIC) stop all ranks.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_vb_multi_out {
  double *beta_vb, *gam_vb, *mu_beta_vb;              /* p x q */
  double *theta_vb, *zeta_vb, *lam2_inv_vb, *sig2_theta_vb, *tau_vb, *sig2_beta_vb;
  int32_t *elbo_it;                                   /* ELBO trace: up to elbo_cap (iteration, value) pairs */
  double *elbo_lb;
  int32_t elbo_cap;
  /* written by the call */
  int32_t n_elbo, it, converged;
  double lb_opt, diff_lb, sig02_inv_vb, sig2_inv_vb;
  double seconds;                                     /* wall-clock of the run incl. set-up of the handles */
  double core_ms;                                     /* device time of the core sweep kernel, max over the GPUs */
} aq_vb_multi_out;
int aq_vb_run_multi(const aq_vb_problem *prob, int32_t n_gpus, const int32_t *devices, int32_t transport, aq_vb_multi_out *out);
/* The trait range [*k0, *k1) of part `part` of `n_parts` for q traits: whole 16-trait tiles, tile counts differing by at most
 * one (the last part also takes the ragged end).  No GPU needed. */
int aq_vb_partition(int32_t q, int32_t n_parts, int32_t part, int32_t *k0, int32_t *k1);

typedef struct aq_vb_status {
  int32_t it;            /* sweeps done                                   */
  int32_t converged;
  double lb_opt;         /* last evaluated ELBO (-inf if none yet)        */
  double diff_lb;        /* |lb_opt - lb_old|                             */
  double c;              /* inverse temperature of the NEXT sweep         */
  int32_t annealing;
  int32_t n_elbo;        /* number of ELBO evaluations so far             */
  double core_ms;        /* accumulated device time of the core sweep kernel (HIP events) */
  int32_t core_launches;
  double sig02_inv_vb, sig2_inv_vb;
  int32_t lentz_iters;   /* shared Lentz iteration count of the last non-annealed sweep */
  int32_t core_kernel;   /* which core sweep kernel this handle runs: 0 look-ahead MFMA (complete Y, or Y with NA when the
                            traits' own Gram blocks fit in HBM), 2 generic wave-per-trait (VALU), 3 round-1 masked MFMA */
  int32_t split_parts;   /* launch plan of the core kernel: workgroups sharing one trait group along the samples (1 = none), */
  int32_t tiles_per_group;   /* 16-trait tiles per workgroup (1 or 2),                                                  */
  int32_t chain_segments;    /* chained SNP segments per trait group (0 = none)                                         */
  /* Which template instance of the core kernel the handle launches (appended; the fields above keep their offsets).  For the
   * look-ahead kernel (core_kernel 0) the residual-tile geometry NT / NT2 / NT3; the masked two-barrier kernel (3) reports its
   * own NT (residual tiles per wave) in tiles_matrix and 0 in the other two; the generic kernel (2) reports 0 in all three. */
  int32_t tiles_matrix;      /* NT: residual tiles of matrix waves 0-2                                                   */
  int32_t tiles_matrix2;     /* NT2: residual tiles of matrix waves 4-6 (NT or NT - 1)                                   */
  int32_t tiles_recurrence;  /* NT3: residual tiles on the recurrence wave, as the launched instance has them             */
  int32_t instance_flags;    /* look-ahead kernel: bit 0 MASK (Y with NA), bit 1 WIDE (9 ... 48 sample parts), bit 2 chained (SEG) */
  int32_t n_pad;             /* samples after padding: 16 x the residual tiles of all parts                              */
} aq_vb_status;
int aq_vb_get_status(aq_vb_handle h, aq_vb_status *st);

/* The AQ_* environment variables (launch-plan overrides for tests and experiments: AQ_TT, AQ_CHAIN, AQ_LA_C, AQ_NT3, AQ_KERNEL, ...)
 * that were SET when the handle was created, as "NAME=value NAME=value"; empty when the plan is the library's own.  Returns the
 * length of the full string (buf may be NULL).  A host that inherits its environment (an R session) can check it here. */
int32_t aq_vb_get_overrides(aq_vb_handle h, char *buf, int32_t cap);

/* The launch plan aq_vb_create would make, without a device: the same planner, fed with the problem sizes, the most missing
 * samples of one trait (0 = complete Y), the largest over traits of min(missing, observed), the device's CU count and total
 * memory (negative = unknown), and the hooks as "NAME=value NAME=value" (the format of aq_vb_get_overrides; NULL or "" = none).
 * The process environment is never read: the result is a function of the arguments alone.  Fills the plan fields of *out
 * (core_kernel, split_parts, tiles_per_group, chain_segments, tiles_matrix, tiles_matrix2, tiles_recurrence, instance_flags,
 * n_pad) and zeroes the rest; a problem aq_vb_create would refuse gets the same code and message, except that an unknown
 * memory size where the wide sample split needs it is AQ_ERR_ARG here.  No GPU needed. */
int aq_plan_query(int32_t n, int32_t p, int32_t q, int32_t max_missing, int32_t max_short_list, int32_t ncu, int64_t total_bytes,
                  const char *overrides, aq_vb_status *out);

/* Which compiled template instance of a core kernel a launch request reaches, without a launch and without a device: the
 * launchers' own dispatch, run dry.  The request is read from the instance fields of *request as aq_vb_get_status and
 * aq_plan_query fill them: core_kernel; for the look-ahead kernel (0) tiles_matrix, tiles_matrix2, tiles_recurrence,
 * tiles_per_group and instance_flags; for the masked kernel (3) tiles_matrix; for the generic kernel (2), whose status names
 * no instance, the arguments ne (samples per lane) and wpt (waves per trait).  On AQ_OK *out holds the template parameters of
 * the kernel that would be launched -- its own, not a copy of the request -- and zeroes for the other kernels' fields;
 * AQ_ERR_UNSUPPORTED, with the launcher's own message, when no instance is compiled for the request.  No GPU needed. */
typedef struct aq_kernel_instance {
  int32_t core_kernel;                    /* 0 look-ahead, 2 generic, 3 masked                                            */
  int32_t nt, nt2, seg, tt, mask, nt3, wide;   /* look-ahead kernel: NT, NT2, SEG, TT, MASK, the resolved NT3, WIDE; masked kernel: nt */
  int32_t ne, wpt;                        /* generic kernel: NE, WPT                                                       */
} aq_kernel_instance;
int aq_instance_query(const aq_vb_status *request, int32_t ne, int32_t wpt, aq_kernel_instance *out);

/* ELBO trace: up to cap (iteration, value) pairs in evaluation order; returns the count. */
int32_t aq_vb_get_elbo_trace(aq_vb_handle h, int32_t *it_out, double *lb_out, int32_t cap);

/* Copy results to host buffers (any pointer may be NULL to skip).  Shapes as the reference's
 * return list (R/atlasqtl_global_local_core.R:406-428): p x q column-major matrices, p / q vectors. */
int aq_vb_get_result(aq_vb_handle h, double *beta_vb, double *gam_vb, double *mu_beta_vb, double *theta_vb,
                     double *zeta_vb, double *lam2_inv_vb, double *sig2_theta_vb, double *tau_vb,
                     double *sig2_beta_vb);

/* The residual the sweep carries in n-space, mis_pat .* (Y - X beta_vb), n x q column-major, copied to the host: what
 * cp_Y_X - cp_betaX_X encodes in the reference (src/coreLoop.cpp:71,81; R/atlasqtl_global_local_core.R:42,115).  It is
 * updated incrementally for the whole run, so its distance from Y - X beta_vb recomputed from aq_vb_get_result is the
 * accumulated rounding drift (tests/test_gpu_bigp.py). */
int aq_vb_get_residual(aq_vb_handle h, double *R_out);

/* ------------------------------------------------------------------------------------------
 * Input construction on the device: the O(n p) part of
 *     prepare_data_(Y, X, ...)                                      R/prepare_atlasqtl.R:8-87
 * i.e. X <- scale(X) (:57), rm_constant_ (R/utils.R:276-302), rm_collinear_ = duplicated(mat, MARGIN = 2) (:304-343),
 * Y <- scale(Y, center = TRUE, scale = FALSE) (:83) and the two missingness guards (:39-45, same messages).
 * X is given as fp64 (n x p column-major) or as int8 dosages X_i8 (0 / 1 / 2 ..., 1 byte per genotype; used when X is NULL),
 * so that the fp64 genotype matrix need never exist on the host.  The standardised compact matrix (n x p_kept) and the
 * centred Y stay on the device; pass aq_prep_x_device / aq_prep_y_device to aq_vb_create with xy_on_device = 1 (the handle
 * must outlive that call only).
 *   aq_prep_info   p_kept; bool_cst[p] (constant columns); bool_coll[p] (later copies of an identical column, in the
 *                  ORIGINAL numbering); dup_of[p] (original index of the kept column a removed copy equals, else -1);
 *                  the column means and n-1 standard deviations used.  Any pointer may be NULL.
 *   aq_prep_get    copies the standardised X (n x p_kept) and / or the centred Y (n x q) to the host.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_prep *aq_prep_handle;
typedef struct aq_prep_input {
  int32_t n, p, q;
  const double *X;      /* n x p fp64, or NULL */
  const int8_t *X_i8;   /* n x p int8 dosages, read when X is NULL */
  const double *Y;      /* n x q, NaN = missing */
  int32_t device;
} aq_prep_input;
int aq_prepare_data(const aq_prep_input *in, aq_prep_handle *out);
int aq_prep_info(aq_prep_handle h, int32_t *p_kept, uint8_t *bool_cst, uint8_t *bool_coll, int32_t *dup_of, double *x_mean,
                 double *x_sd);
const double *aq_prep_x_device(aq_prep_handle h);
const double *aq_prep_y_device(aq_prep_handle h);
int aq_prep_get(aq_prep_handle h, double *X_out, double *Y_out);
void aq_prep_destroy(aq_prep_handle h);

/* ------------------------------------------------------------------------------------------
 * Post-processing of the posterior inclusion probabilities on the device.
 *   aq_assign_bfdr       assign_bFDR, R/summarise_output.R:207-223: Bayesian FDR estimate of every entry of
 *                        mat_ppi (len = p*q, any layout: the function works on as.vector(mat_ppi)); ties keep their
 *                        original order as with R's order(decreasing = TRUE).  Host pointers.  Any length that fits the
 *                        device (64-bit positions from 2^32 entries on).
 *   aq_hotspot_sizes     rowSums(gam_vb > thres) / rowSums(assign_bFDR(gam_vb) < thres) and their total
 *                        (summary.atlasqtl / plot.atlasqtl, R/summarise_output.R:98-105,177-182); mat_ppi p x q
 *                        column-major on the host.
 *   aq_vb_hotspot_sizes  the same from the gam_vb resident in a handle, without copying it to the host.
 * ---------------------------------------------------------------------------------------- */
int aq_assign_bfdr(const double *mat_ppi, double *mat_fdr, int64_t len, int32_t device);
int aq_hotspot_sizes(const double *mat_ppi, int32_t p, int32_t q, double thres, int32_t fdr_adjust,
                     int64_t *rs_thres, int64_t *nb_pairwise, int32_t device);
int aq_vb_hotspot_sizes(aq_vb_handle h, double thres, int32_t fdr_adjust, int64_t *rs_thres, int64_t *nb_pairwise);
/* The same FDR thresholding when the traits are spread over several processes: assign_bFDR ranks ALL p q PPIs, so a
 * shard cannot do it alone.  Each process sorts its shard once (aq_vb_bfdr_begin) and answers, for a PPI value c,
 *   out5 = { #{ppi >= c}, sum(1 - ppi : ppi >= c), #{ppi > c}, sum(1 - ppi : ppi > c), largest ppi < c (or -1) }
 * (aq_vb_bfdr_query).  Summed over the processes these give the running mean of 1 - PPI at the end of c's tie block -- the
 * estimated FDR there, non-decreasing along the order -- so the caller bisects over c with one small all-reduce per
 * step.  aq_vb_bfdr_rows then counts, per predictor, this shard's first `upto` entries of the order plus `take` entries of
 * the tie block starting at sorted position tie_first (ties go in original order, R's order(decreasing = TRUE)).
 * atlasqtl_amd/core.py::VbRun.hotspot_sizes drives it over torch.distributed. */
int aq_vb_bfdr_begin(aq_vb_handle h);
int aq_vb_bfdr_query(aq_vb_handle h, double c, double *out5);
int aq_vb_bfdr_rows(aq_vb_handle h, int64_t upto, int64_t tie_first, int64_t take, int64_t *rs);
void aq_vb_bfdr_end(aq_vb_handle h);

/* ------------------------------------------------------------------------------------------
 * Sparse table of associations: what summary.atlasqtl / plot.atlasqtl read off gam_vb (R/summarise_output.R:99-106),
 *     fdr_adjust = 0   { (j,k) : gam_vb[j,k] > thres }                      (:104)
 *     fdr_adjust = 1   { (j,k) : assign_bFDR(gam_vb)[j,k] < thres }         (:100-101)
 * as rows (snp j, trait k, ppi, beta = gam_vb mu_beta_vb (R/update_vb.R:17), fdr), 0-based, in the order of
 * order(as.vector(gam_vb), decreasing = TRUE): decreasing PPI, ties by increasing column-major position j + p k.  In
 * both modes the set is a prefix of that order, so fdr = cumsum(1 - ppi) / (1:N) along the table equals assign_bFDR at
 * those entries.  The p x q matrices never leave the device; in PPI mode on a handle nothing of size p q is allocated
 * (the trait-tiled state is read in place and only the selected rows are sorted).
 *   aq_vb_select_pairs  from the gam_vb / mu_beta_vb resident in a handle (trait = index local to the handle).  Writes
 *                       the first min(cap, *n_pairs) rows; *n_pairs is always the full count.  cap = 0 with NULL arrays
 *                       counts only.  Any output array may be NULL.  Synchronises and reports an expired in-kernel wait
 *                       (AQ_ERR_DEVICE) as aq_vb_get_result does.
 *   aq_select_pairs     the same on host matrices (p x q column-major); mat_beta may be NULL (beta is then not written).
 *   aq_vb_bfdr_pairs    trait-sharded FDR mode, between aq_vb_bfdr_begin and aq_vb_bfdr_end, with the arguments of
 *                       aq_vb_bfdr_rows: this shard's first `upto` sorted entries plus `take` entries of the tie block
 *                       at tie_first, as rows (snp, local trait, ppi, beta).  The caller merges the shards' rows by
 *                       (-ppi, global position) and takes the running mean (atlasqtl_amd/core.py::VbRun.associations).
 * NaN thres, cap < 0, NULL n_pairs / handle / mat_ppi: AQ_ERR_ARG before any device call.
 * ---------------------------------------------------------------------------------------- */
int aq_vb_select_pairs(aq_vb_handle h, double thres, int32_t fdr_adjust, int64_t cap, int32_t *snp, int32_t *trait,
                       double *ppi, double *beta, double *fdr, int64_t *n_pairs);
int aq_select_pairs(const double *mat_ppi, const double *mat_beta, int32_t p, int32_t q, double thres,
                    int32_t fdr_adjust, int64_t cap, int32_t *snp, int32_t *trait, double *ppi, double *beta,
                    double *fdr, int64_t *n_pairs, int32_t device);
int aq_vb_bfdr_pairs(aq_vb_handle h, int64_t upto, int64_t tie_first, int64_t take, int32_t *snp, int32_t *trait,
                     double *ppi, double *beta);

/* ------------------------------------------------------------------------------------------
 * Order statistics and moments of the p x q posterior values, computed where they lie: the first block of
 * summary.atlasqtl (R/summarise_output.R:89-97), summary(as.vector(gam_vb)) and summary(as.vector(beta_vb)) -- minimum,
 * quartiles, mean, maximum -- without a p x q array leaving the device or being allocated on it.
 *   which = 0   gam_vb of the handle (trait-tiled storage read in place; padding rows and traits are not values)
 *   which = 1   beta_vb = gam_vb * mu_beta_vb (R/update_vb.R:17), one fp64 product per element formed on the fly
 * Order: a double maps to a 64-bit key whose unsigned order is the order of the values (negative: all bits flipped;
 * otherwise: sign bit set; -0.0 sorts just below +0.0).  NaN is not a value: it is counted in n_nan and left out of every
 * histogram, order statistic and moment, as R's summary.default does with NA.
 * The select is a radix select on AQ_RSEL_BITS-wide digits of the key, 64 / AQ_RSEL_BITS passes over the storage; its
 * scratch is the histogram and one record per workgroup, nothing that grows with p q.
 *   aq_vb_radix_hist   one step, the primitive a trait-sharded driver needs (histograms of disjoint shards add): for each
 *                      of n_prefix (1 ... AQ_RSEL_MAX_PREFIX) prefixes, strictly ascending, the histogram of the digit at
 *                      bit `shift` among the values whose key satisfies key >> (shift + AQ_RSEL_BITS) == prefix[i].
 *                      shift + AQ_RSEL_BITS == 64: all values, n_prefix must be 1 and prefix is not read.
 *                      hist: n_prefix x 2^AQ_RSEL_BITS counts, host.  One pass over the storage serves all prefixes.
 *   aq_vb_moments      count, n_nan, min, max, sum over the non-NaN values in one pass.  sum is reproducible: fixed-order
 *                      partial sums, no floating atomics -- two calls on one handle return the same bits.  No value:
 *                      count = 0, min = +Inf, max = -Inf (the neutral elements, so that shards combine by min / max).
 *   aq_vb_order_stats  the whole select: out[i] = the ranks[i]-th smallest value (0-based; ranks ascending, equal ones
 *                      allowed; 1 <= n_ranks <= AQ_RSEL_MAX_PREFIX; each rank < count); mom may be NULL.
 *   aq_order_stats     the same on a host array of len doubles (copied to the device as aq_assign_bfdr does).
 * All four synchronise; the handle entries report an expired in-kernel wait (AQ_ERR_DEVICE) as aq_vb_get_result does.
 * NULL handle / array / output, which not 0 / 1, n_ranks or n_prefix out of range, ranks negative or not ascending,
 * prefixes not ascending, len < 1, shift not a multiple of AQ_RSEL_BITS in [0, 64): AQ_ERR_ARG, with the entry's name in
 * aq_last_error(), before any device call; a rank >= count is AQ_ERR_ARG once the count is known.
 * ---------------------------------------------------------------------------------------- */
#define AQ_RSEL_BITS 8          /* digit width; divides 64.  8 passes, 256 bins x 8 B x 16 prefixes = 32 KB of LDS */
#define AQ_RSEL_MAX_PREFIX 16
typedef struct aq_moments {
  int64_t count, n_nan;
  double min, max, sum;
} aq_moments;
int aq_vb_radix_hist(aq_vb_handle h, int32_t which, int32_t n_prefix, const uint64_t *prefix, int32_t shift, int64_t *hist);
int aq_vb_moments(aq_vb_handle h, int32_t which, aq_moments *out);
int aq_vb_order_stats(aq_vb_handle h, int32_t which, int32_t n_ranks, const int64_t *ranks, double *out, aq_moments *mom);
int aq_order_stats(const double *x, int64_t len, int32_t n_ranks, const int64_t *ranks, double *out, aq_moments *mom,
                   int32_t device);

/* ------------------------------------------------------------------------------------------
 * Checkpoint / resume.  The reference's checkpoint_ (R/utils.R:571-611, called at
 * R/atlasqtl_global_local_core.R:379) only writes outputs every 100 iterations and cannot resume; these
 * entries capture and restore the COMPLETE loop state between two sweeps (valid after aq_vb_run /
 * aq_vb_run_sweeps returned, or between aq_vb_advance calls that returned AQ_VB_DONE), so that a
 * restored handle continues bit-identically.  The handle receiving the state must have been created
 * for the same X, Y, hyper-parameters and device geometry (any list_init): shapes are checked.
 * ---------------------------------------------------------------------------------------- */
int64_t aq_vb_state_bytes(aq_vb_handle h);
int aq_vb_get_state(aq_vb_handle h, void *buf, int64_t cap);
int aq_vb_set_state(aq_vb_handle h, const void *buf, int64_t len);

/* ------------------------------------------------------------------------------------------
 * Test hooks for the fp64 special functions the path uses (host evaluation of the same
 * header the kernels compile): which = 0 log_ndtr, 1 digamma, 2 expint_E1 (x<=1),
 * 3 gamma_inc_upper(a=x2, x), 4 sigmoid_neg, 5 / 6 log Phi / log(1-Phi) and 7 / 8 the inverse Mills
 * ratios phi/Phi, -phi/(1-Phi) (R/utils.R:172-191) from aq_probit_terms, 9 erfcx(x), x >= 0,
 * 10 / 11 / 12 log(1-Phi) - log Phi and the two Mills ratios from the pre-pass form aq_probit_A_imr.
 * 13 the short-dependency-chain sigmoid of the SNP recursion (aq_sigmoid_neg_fast).
 * 14 - 17 compute_integral_hs_ (x = L, x2 = Q(L)); 18 / 19 / 20 log(1-Phi) - log Phi and the two Mills ratios from the piecewise
 * polynomial tables the sweep kernel evaluates (aq_probit_tab.h; tail series beyond |x| = 12); 21 / 22 / 23
 * update_annealed_lam2_inv_vb_(x = L_vb, x2 = c, df = 3 / 5 / 7) (R/update_vb.R:76-81, Kummer's 1F1).
 * 24 / 25 log Phi / log(1 - Phi) from the tables, as the ELBO pass (R/elbo.R:10-34) evaluates them (aq_log_ndtr_pair_tab).
 * Evaluates elementwise into out.  aq_special_eval_device runs the same switch in a kernel on `device`
 * (host pointers in and out): the device build of these functions (ocml, v_rcp_f64) is what the sweep executes.
 * ---------------------------------------------------------------------------------------- */
int aq_special_eval(int32_t which, const double *x, const double *x2, double *out, int64_t len);
int aq_special_eval_device(int32_t which, const double *x, const double *x2, double *out, int64_t len, int32_t device);
/* Test hook: raises the device-side flag that a bounded in-kernel wait sets when it expires (a chained SNP segment
 * waiting for its predecessor, a sample part waiting for its partners); every later aq_vb_run / aq_vb_get_status /
 * aq_vb_get_state / aq_vb_get_result on the handle must then fail with AQ_ERR_DEVICE. */
int aq_vb_debug_raise_errflag(aq_vb_handle h);
/* Test hook: the bytes of device memory that the library's own allocations hold in this process at the moment (handles,
 * prepared data, buffers of entries in flight).  0 in a fresh process; back at its earlier value once everything that was
 * created since has been destroyed. */
int64_t aq_debug_live_device_bytes(void);
/* Test hook: column col of a prepare handle's standardised compact X replaced by values[n].  The preparation removes constant
 * columns, so a column of zeros -- which the cis fine-mapping must give no prior weight -- reaches a handle only this way. */
int aq_prep_debug_set_column(aq_prep_handle h, int32_t col, const double *values);
/* Test hook: one of the buffers aq_vb_create builds once per handle, as it lies in device memory (the layouts are described in
 * atlasqtl_amd/csrc/aq_core_sweep.h and aq_vb.h).  Returns the buffer's length in bytes and copies it to buf when cap_bytes
 * suffices (buf may be NULL with cap_bytes = 0: the length alone); 0 for a buffer this handle does not hold -- GK without the
 * MASK instances, XR once a MASK handle has released it, the operand panels and Gram blocks under the generic kernel; and
 * -AQ_ERR_ARG / -AQ_ERR_DEVICE with aq_last_error() set (NULL handle, which out of range, cap_bytes < 0, NULL buf with
 * cap_bytes > 0; a failed copy).  Copies only: launches nothing, allocates nothing, keeps nothing alive.
 * AQ_SETUP_GEOMETRY: AQ_SETUP_GEOMETRY_LEN int32 -- nb, ntile, n_pad, p_pad, q_pad, NR, Mmax, dmode, then 0 / 1 each for
 * use_la, la_mask, la_wide, use_mis, use_tw (the planner's fields, atlasqtl_amd/csrc/aq_plan.h).  XA, XU: double2; midx,
 * mcnt4, mobs: int32; everything else: double. */
enum {
  AQ_SETUP_GEOMETRY = 0, AQ_SETUP_XA, AQ_SETUP_XU, AQ_SETUP_XR, AQ_SETUP_G, AQ_SETUP_GX, AQ_SETUP_GK, AQ_SETUP_MIDX,
  AQ_SETUP_MCNT4, AQ_SETUP_MOBS, AQ_SETUP_MIS, AQ_SETUP_R, AQ_SETUP_GAM, AQ_SETUP_MU, AQ_SETUP_COUNT
};
#define AQ_SETUP_GEOMETRY_LEN 13
int64_t aq_vb_debug_get_setup(aq_vb_handle h, int32_t which, void *buf, int64_t cap_bytes);
/* exp(x) E1(x) for a vector with the reference's shared Lentz stopping rule (R/utils.R:380-423);
 * host evaluation; writes the shared iteration count to *iters. */
int aq_q_approx_vec(const double *x, double *out, int64_t len, int32_t *iters);

/* ------------------------------------------------------------------------------------------
 * aq_prepare_data from the variant blocks of a PLINK 1 .bed file (variant-major), 2 bits per genotype: the packed bytes
 * are uploaded as they are and unpacked on the device into the column-major dosage buffer that the int8 path of
 * aq_prepare_data reads, so only n p / 4 bytes cross PCIe.  Sample s of a variant is (block[s >> 2] >> (2 (s & 3))) & 3;
 * 0 = homozygous A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2; the padding bits of a block's last byte are never
 * read as genotypes.  With no missing genotype among the n rows used the result is bit-identical to aq_prepare_data on the
 * same dosages as int8.  missing = 1: a missing genotype takes (n_het + 2 n_hom_counted) / n_obs of its variant, ONE fp64
 * division of the exact counts, and the result is bit-identical to aq_prepare_data on that fp64 matrix; a variant without an
 * observed genotype becomes all 0.0 and is reported constant.  missing = 0: a missing genotype is AQ_ERR_ARG (the
 * reference's message for a matrix X with NA, then how many and where).  Y as in aq_prepare_data.  The argument checks
 * (NULL, n < 2, p < 1, q < 1, n > n_file, sample_idx NULL with n != n_file, an index out of range, count_a2 / missing not
 * 0 or 1) come before any device call.  The handle is an aq_prep_handle like any other (aq_prep_info, aq_prep_get, ...).
 *   aq_prep_genotype_counts   the counts the decode pass took per variant over the n rows used.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_prep_bed_input {
  int32_t n_file;             /* samples in the file; stride = (n_file + 3) / 4 bytes per variant            */
  int32_t n, p, q;            /* rows of X and Y, variants given, traits                                      */
  const uint8_t *bed;         /* p x stride bytes: the variant blocks only, without the 3-byte header (host)  */
  const int32_t *sample_idx;  /* n entries in [0, n_file): row i of X is file sample sample_idx[i];
                                 NULL: n == n_file, identity                                                   */
  const double *Y;            /* n x q column-major, NaN = missing                                            */
  int32_t count_a2;           /* 0: dosage of A1, 1: dosage of A2                                             */
  int32_t missing;            /* 0: a missing genotype is an error, 1: the column mean of the observed ones   */
  int32_t device;
} aq_prep_bed_input;
int aq_prepare_data_bed(const aq_prep_bed_input *in, aq_prep_handle *out);
int aq_prep_genotype_counts(aq_prep_handle h, int32_t *counts);   /* 4 x p column-major: hom A1, het, hom A2, missing,
                                                                     over the n rows used; AQ_ERR_ARG for a handle that
                                                                     aq_prepare_data made                              */

/* ------------------------------------------------------------------------------------------
 * Covariates: aq_prepare_data / aq_prepare_data_bed on the residuals of X and Y after regression on W = [1, Z], Z an
 * n x d matrix of covariates (age, sex, genotype PCs, PEER or batch factors ...), finite, 1 <= d <= 96, d + 1 < n.  The fit
 * is the fit of the unchanged code to the residualised data; the reference has no such argument (its users residualise in R).
 * Q is an orthonormal basis of W's columns taken in order (Q[:, 0] = 1 / sqrt(n)).
 *   X   x_j <- x_j - Q (Q' x_j) over all n rows, applied twice.  With s0 = sum_i (x_ij - mean_j)^2 and s1 = sum_i xr_ij^2, a
 *       non-constant column with s1 <= 1e-10 s0 is ABSORBED by the covariates: it is written as all 0.0 and the pipeline then
 *       reports it constant (bool_cst).  (The error of xr is about eps |x|, so at 1 - R^2 = 1e-10 the standardised column is
 *       still good to about 1e-11; below that it is rounding noise which scale() would blow up to unit variance.)  The fp64
 *       pipeline of aq_prepare_data then runs on the residuals unchanged; identical columns give bit-identical residuals.
 *   Y   for trait k with observed rows O_k: y_k[O_k] <- y_k[O_k] - W[O_k] b_k, b_k the least-squares solution on those rows
 *       (Cholesky of Q[O_k]' Q[O_k], one step of refinement); NaN stays NaN.  This replaces the centring.  |O_k| <= d + 1 or a
 *       Cholesky pivot <= 1e-10: AQ_ERR_ARG, "covariates are collinear on the samples observed for column k of Y" (k 1-based),
 *       after the two missingness guards.
 * For a trait with missing rows the residual genotypes are orthogonal to the covariates over all n rows, not over O_k (as in
 * every tool that residualises the genotypes once), and the model is not told about the d + 1 degrees of freedom removed.
 *   aq_prepare_data_cov, aq_prepare_data_bed_cov   cov == NULL or cov->d == 0: exactly aq_prepare_data / aq_prepare_data_bed.
 *       On the bed path the decoded int8 dosages (missing = 1 with missing calls: the imputed fp64 matrix) are residualised.
 *   aq_prep_cov_info   d (0: the handle was made without covariates, nothing else is written); absorbed[p]; r2[p] = 1 - s1 / s0
 *       per column given (NaN for a constant column).  Any pointer may be NULL.
 *   aq_cov_basis       host only: Q (n x (d + 1) column-major) by modified Gram-Schmidt applied twice.  Covariate l (0-based)
 *       is collinear when what is left of it after the intercept and the covariates before it has a squared norm <= 1e-10
 *       times its own (a constant covariate is collinear with the intercept): AQ_ERR_ARG, *bad_col = l, the message names
 *       column l + 1.  Otherwise *bad_col = -1.  bad_col may be NULL.
 * NULL, d > 96, d + 1 >= n, a non-finite entry of Z and a collinear covariate are AQ_ERR_ARG before any device call.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_prep_cov {
  int32_t d;
  const double *Z;   /* n x d column-major, host */
} aq_prep_cov;
int aq_prepare_data_cov(const aq_prep_input *in, const aq_prep_cov *cov, aq_prep_handle *out);
int aq_prepare_data_bed_cov(const aq_prep_bed_input *in, const aq_prep_cov *cov, aq_prep_handle *out);
int aq_prep_cov_info(aq_prep_handle h, int32_t *d, uint8_t *absorbed, double *r2);
int aq_cov_basis(const double *Z, int32_t n, int32_t d, double *Q, int32_t *bad_col);

/* ------------------------------------------------------------------------------------------
 * LD pruning: thins the compact standardised matrix of a handle that any of the four aq_prepare_data* entries returned, so
 * that no two kept predictors within `window` columns of each other correlate above a threshold.  The model splits a signal's
 * posterior inclusion probability over every variant of an LD block; the reference's authors prune before they fit.  It runs
 * on the columns the fit sees (after constant and duplicate removal, with covariates on the residuals) and where they lie.
 * Xs is n x p1, every column with mean 0 and sum of squares n - 1; i, j below are compact indices.
 *   r(i, j) = (Xs_i . Xs_j) / (n - 1).
 *   A pair i < j is ELIGIBLE when j - i <= window, group[i] == group[j] (NULL: one group) and, if window_bp > 0,
 *   |pos_j - pos_i| <= window_bp.
 *   Columns are visited in increasing j.  Column j is REMOVED iff some KEPT column i < j forms an eligible pair with it and
 *   r(i, j)^2 > r2 (strictly).  Its tag is the smallest such i.  The first column is always kept.  With r^2(A, B) > r2,
 *   r^2(B, C) > r2 and r^2(A, C) <= r2 the result is A and C kept, B removed: first one wins, as rm_collinear_ does.
 * The banded Gram matrix is formed on the f64 matrix pipe (2 n p1 window flop) and thresholded in registers: one bit per
 * (column, band entry) is stored, never the p1 x window values.  One wave scans the bit rows; the kept columns are gathered
 * into a new n x p_kept matrix, a copy of their bits, and the old one is released.
 *   aq_prep_ld_prune   in place, once per handle.  Afterwards aq_prep_x_device, aq_prep_get and the p_kept of aq_prep_info
 *                      describe the pruned matrix; bool_cst, bool_coll and dup_of are unchanged.
 *   aq_prep_ld_info    in the ORIGINAL column numbering (p entries each, any pointer may be NULL): bool_ld[j] = 1 removed for
 *                      LD; ld_of[j] the original index of its tag, else -1; ld_r2[j] = r(tag, j)^2, NaN where the column was
 *                      not removed for LD.
 *   aq_prep_ld_band    the band of the handle's current matrix, for inspection and tests: r_band[b p_kept + j] =
 *                      r(j - 1 - b, j) for 0 <= b < window, NaN where j - 1 - b < 0.  Every entry is within (n + 2) 2^-53 of
 *                      the exact quotient.  This entry does write the p_kept x window doubles.
 * A NULL handle, struct or output, window outside [1, 4096], r2 outside (0, 1] or NaN, window_bp > 0 without pos, a second
 * aq_prep_ld_prune on one handle and aq_prep_ld_info on an unpruned handle are AQ_ERR_ARG, with the entry's name in
 * aq_last_error(), before any device call.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_prep_ld {
  int32_t window;         /* 1 ... 4096 columns                                             */
  double r2;              /* threshold on r^2, in (0, 1]; 1 removes nothing beyond rounding */
  const int32_t *group;   /* p entries, original column numbering, or NULL: one group       */
  const int64_t *pos;     /* p entries, original column numbering, or NULL                  */
  int64_t window_bp;      /* <= 0: no distance limit; > 0 needs pos                         */
} aq_prep_ld;
int aq_prep_ld_prune(aq_prep_handle h, const aq_prep_ld *ld);
int aq_prep_ld_info(aq_prep_handle h, int32_t *p_kept, uint8_t *bool_ld, int32_t *ld_of, double *ld_r2);
int aq_prep_ld_band(aq_prep_handle h, int32_t window, double *r_band);

/* ------------------------------------------------------------------------------------------
 * Genetic relationship matrix (GRM) of a handle that any of the four aq_prepare_data* entries returned: the n x n matrix
 *   K[a, b] = (sum_j Xs[a, j] Xs[b, j]) / p1
 * over all p1 columns of the handle's CURRENT matrix Xs (what aq_prep_x_device shows: after constant and duplicate removal,
 * with covariates the residuals, after aq_prep_ld_prune the kept columns), every column with mean 0 and sum of squares
 * n - 1.  Its leading eigenvectors are the genotype principal components that a QTL analysis passes as covariates; they are
 * taken on the host (atlasqtl_amd.genotype_pcs).  Every column is centred, so K 1 = 0 up to rounding and trace K = n - 1.
 * The product is formed on the f64 matrix pipe (n^2 p1 useful flop): one triangle of output tiles, the predictors split over
 * several workgroups per tile whose partial tiles a second kernel adds in a fixed order -- no floating-point atomics, so two
 * calls on one handle return the same bits -- and both halves of K are written from the same registers, so K equals its
 * transpose exactly.  Every entry is within (p1 + 2) 2^-53 (sum_j |Xs[a, j] Xs[b, j]|) / p1 of the exact value.
 *   aq_prep_grm         K_out: n x n column-major, host.  trace_out (may be NULL): the diagonal of K_out added in index order.
 *                       The handle is not changed.
 *   aq_grm_plan_query   the launch plan without a device, a pure function of its arguments: tile edge, tiles of one triangle
 *                       (tile t = ti (ti + 1) / 2 + tj, ti >= tj), splits, predictors per chunk and chunks per split; the
 *                       grid is n_tiles x splits workgroups.  splits = 1 when the tiles alone give two workgroups per CU;
 *                       k_bytes + scratch_bytes <= free_bytes.  The environment variable AQ_GRM_SPLITS (1 ... 64; tests)
 *                       forces the splits of aq_prep_grm; the query does not read it.
 *   aq_prep_grm_time    measurement: the two kernels `reps` times between two events after one warm-up, without the copy to
 *                       the host; ms_per_call and, if not NULL, the plan used.
 * n > 10240 is AQ_ERR_UNSUPPORTED (K is 0.84 GB there and its eigen-decomposition runs on the host); a NULL handle or output
 * is AQ_ERR_ARG; both come before any device call.  A plan that does not fit the free memory is AQ_ERR_DEVICE.  Every error
 * names the entry that was called (aq_prep_grm, aq_grm_plan_query, aq_prep_grm_time) in aq_last_error().
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_grm_plan {
  int32_t tile;               /* edge of an output tile: 64 or 128 samples                   */
  int32_t tiles_per_edge;     /* ceil(n / tile)                                              */
  int32_t n_tiles;            /* tiles of one triangle: tiles_per_edge (tiles_per_edge + 1) / 2 */
  int32_t splits;             /* workgroups per tile, each with its own predictors           */
  int32_t chunk;              /* predictors staged per step                                  */
  int32_t chunks_per_split;   /* split s owns chunks [s chunks_per_split, (s + 1) chunks_per_split) */
  int64_t scratch_bytes;      /* the partial tiles: splits n_tiles tile^2 doubles            */
  int64_t k_bytes;            /* K on the device: n^2 doubles                                */
} aq_grm_plan;
int aq_prep_grm(aq_prep_handle h, double *K_out, double *trace_out);
int aq_grm_plan_query(int32_t n, int32_t p1, int32_t ncu, int64_t free_bytes, aq_grm_plan *out);
int aq_prep_grm_time(aq_prep_handle h, int32_t reps, double *ms_per_call, aq_grm_plan *plan_out);

/* ------------------------------------------------------------------------------------------
 * The relationship operator applied to a block of vectors, without the n x n matrix: for a handle as above and Q (n x L),
 *   Z = Xs (Xs' Q) / p1 = K Q
 * over the same current matrix Xs that aq_prep_grm uses.  It is the step of subspace iteration for the leading eigenvectors
 * of K (the genotype principal components), and it grows as n p1 L, not as n^2: every n a handle holds is taken (up to
 * 82 944, AQ_N_MAX); the 10 240 of aq_prep_grm does not apply.
 * Two tall-skinny products on the f64 matrix pipe (4 n p1 lp flop, two reads of Xs; lp = L padded to 16): T = Xs' Q
 * (p1 x lp, kept in device memory), one workgroup per panel of predictors, the reduction over the samples; then Xs T over
 * tiles of samples, the predictors split over several workgroups per tile whose partial tiles a third kernel adds in a fixed
 * order and divides by p1 -- no floating-point atomics, so two calls on one handle return the same bits.  Rows >= n and
 * columns >= L of the padded block contribute exact zeros; Q = 0 gives Z = 0 exactly.  Every entry is within
 * (n + p1 + 4) 2^-53 (|Xs| (|Xs'| |Q|)) / p1 of the exact value.
 *   aq_prep_grm_apply       Q, Z_out: n x L column-major, host, 1 <= L <= 128 (AQ_PCS_MAX_L).  trace_out (may be NULL): the
 *                           trace of K, (sum of Xs^2) / p1, every column's sum of squares added in a fixed order and the
 *                           columns in index order.  The handle is not changed.
 *   aq_pcs_plan_query       the launch plan without a device, a pure function of its arguments: the padded width, the panels
 *                           of the first product (grid n_panels), the sample tiles and predictor splits of the second (grid
 *                           n_tiles x splits; split s owns the chunks [s chunks_per_split, (s + 1) chunks_per_split)) and the
 *                           device memory: t_bytes + io_bytes + scratch_bytes <= free_bytes.  splits = 1 when the tiles alone
 *                           give two workgroups per CU.  The environment variable AQ_PCS_SPLITS (1 ... 64; tests) forces the
 *                           splits of aq_prep_grm_apply; the query does not read it.
 *   aq_prep_grm_apply_time  measurement: the kernels of one application `reps` times between two events after one warm-up,
 *                           without the copies from and to the host; ms_per_call and, if not NULL, the plan used.
 * L outside [1, 128], a NULL handle or a NULL operand is AQ_ERR_ARG, before any device call.  A plan that does not fit the free
 * memory is AQ_ERR_DEVICE.  Every error names the entry that was called (aq_prep_grm_apply, aq_pcs_plan_query,
 * aq_prep_grm_apply_time) in aq_last_error().
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_pcs_plan {
  int32_t lp;                 /* L padded to a multiple of 16: columns of T and of a partial tile */
  int32_t panel;              /* predictors per workgroup of T = Xs' Q                        */
  int32_t n_panels;           /* ceil(p1 / panel): the grid of the first product              */
  int32_t sample_chunk;       /* samples of Q staged per step of the first product           */
  int32_t n_pad;              /* n padded to a multiple of sample_chunk                       */
  int32_t tile;               /* samples per workgroup of Xs T                                */
  int32_t n_tiles;            /* ceil(n / tile)                                               */
  int32_t splits;             /* workgroups per tile, each with its own predictors           */
  int32_t chunk;              /* predictors staged per step of the second product            */
  int32_t chunks_per_split;   /* split s owns chunks [s chunks_per_split, (s + 1) chunks_per_split) */
  int64_t t_bytes;            /* T on the device: panel n_panels lp doubles                  */
  int64_t scratch_bytes;      /* the partial tiles: splits n_tiles tile lp doubles           */
  int64_t io_bytes;           /* Q, Z (n L doubles each) and the padded row-major Q (n_pad lp) */
} aq_pcs_plan;
int aq_prep_grm_apply(aq_prep_handle h, const double *Q, int32_t L, double *Z_out, double *trace_out);
int aq_pcs_plan_query(int32_t n, int32_t p1, int32_t L, int32_t ncu, int64_t free_bytes, aq_pcs_plan *out);
int aq_prep_grm_apply_time(aq_prep_handle h, int32_t L, int32_t reps, double *ms_per_call, aq_pcs_plan *plan_out);

/* ------------------------------------------------------------------------------------------
 * Rank-based inverse normal transform (INT) of the traits, the step every molecular-QTL pipeline applies to expression,
 * protein or metabolite levels before anything else: the model is Gaussian per trait, and a handful of outlying samples in
 * a few skewed traits otherwise show up as spurious hotspots.  The reference has no such argument (its users transform in R).
 * For trait k with observed rows O_k, m = |O_k| (NaN is missing and stays NaN): r_i is the 1-based rank of y_ik among the
 * observed values of the column, ties given their AVERAGE rank; -0.0 and +0.0 are equal and tie; -inf and +inf rank as the
 * extremes.  Then
 *   y_ik <- Phi^-1((r_i - c) / (m + 1 - 2 c)),   0 <= c <= 1/2:  c = 3/8 Blom (the usual choice), 0 van der Waerden, 1/2 rankit.
 * It runs BEFORE everything else that is done to Y: with covariates the transformed column is residualised, without them it
 * is centred, and the two missingness guards keep their messages and their order.  A column with fewer than two distinct
 * observed values is AQ_ERR_ARG, "column k of Y has fewer than two distinct observed values; it cannot be rank-normalised"
 * (k 1-based), after the two guards.
 * One workgroup per trait sorts the column's order-preserving 64-bit keys (NaN above every value) by a bitonic network --
 * in LDS up to 16 384 samples, beyond that (up to 82 944, AQ_N_MAX) in device memory, chunk by chunk through LDS -- and every
 * sample finds the number of keys below and not above its own by two binary searches: the doubled rank 2 r is an exact
 * integer whatever the ties, and the argument of Phi^-1 is ONE fp64 division, (t - 2 c) / (2 m + 2 - 4 c) with t = min(2 r,
 * 2 m + 2 - 2 r), the sign applied afterwards: ranks r and m + 1 - r give exact negatives of each other, the middle rank
 * exactly 0, and the two paths the same bits.  The environment variable AQ_YT_PATH (lds | global; tests) forces a path where
 * the column fits both.
 *   aq_prepare_data_opt    the four aq_prepare_data* entries in one: exactly one of in / bed is non-NULL; cov and yt may be
 *                          NULL.  yt == NULL or yt->method == 0: exactly the entry that the other arguments name.
 *   aq_prep_ytrans_info    method (0: the handle was made without a transform, nothing else is written), offset = c, and per
 *                          trait n_obs[q] = m and n_tied[q] = the observed values that share their value with another one.
 *                          Any pointer may be NULL.
 *   aq_rank_int            the transform alone.  Y, out: n x q column-major, host (out may be Y); n_obs, n_tied: q each, may
 *                          be NULL.  No missingness guard: only the column without two distinct observed values is refused.
 *   aq_ytrans_plan_query   the launch plan without a device: path 0 (LDS) or 1 (device memory), the padded key count, the
 *                          dynamic LDS of a workgroup, the traits per launch and the scratch for their keys, scratch_bytes <=
 *                          free_bytes.  It reads AQ_YT_PATH as the entries do.  A column whose keys do not fit free_bytes and
 *                          n > 82 944 are AQ_ERR_UNSUPPORTED, as in aq_plan_query.
 * An unknown method, c outside [0, 1/2] or NaN, a NULL argument and n > 82 944 are AQ_ERR_ARG before any device call.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_prep_ytrans {
  int32_t method;   /* 0 none, 1 rank-based inverse normal */
  double offset;    /* c */
} aq_prep_ytrans;
typedef struct aq_ytrans_plan {
  int32_t path;               /* 0: keys in LDS; 1: keys in device memory                    */
  int32_t n_pad;              /* keys per column: n padded to a power of two                 */
  int32_t lds_bytes;          /* dynamic LDS of a workgroup: 8 min(n_pad, 16 384) <= 160 KiB */
  int32_t traits_per_batch;   /* workgroups per launch                                       */
  int64_t scratch_bytes;      /* path 1: 8 n_pad traits_per_batch; path 0: 0                 */
} aq_ytrans_plan;
int aq_prepare_data_opt(const aq_prep_input *in, const aq_prep_bed_input *bed, const aq_prep_cov *cov, const aq_prep_ytrans *yt,
                        aq_prep_handle *out);
int aq_prep_ytrans_info(aq_prep_handle h, int32_t *method, double *offset, int32_t *n_obs, int32_t *n_tied);
int aq_rank_int(const double *Y, int32_t n, int32_t q, double offset, double *out, int32_t *n_obs, int32_t *n_tied, int32_t device);
int aq_ytrans_plan_query(int32_t n, int32_t q, int64_t free_bytes, aq_ytrans_plan *out);

/* ------------------------------------------------------------------------------------------
 * Marginal screen of a finished handle: every predictor of the handle's CURRENT matrix Xs (p1 columns) tested against every
 * trait of Yc on its own, the classical univariate scan that a joint fit is compared with.  For predictor s and trait t, over
 * the m_t rows O_t where the trait is observed:
 *   Sxy = sum x y,  Sx = sum x,  Sxx = sum x^2,  Syy_t = sum y^2 (added in index order; Yc is centred over O_t, so sum y = 0)
 *   Vx = Sxx - Sx^2 / m_t,   r = Sxy / sqrt(Vx Syy_t),   df_t = m_t - 2 - n_cov,   t = r sqrt(df_t / (1 - r^2)).
 * A pair is UNDEFINED when Vx <= 1e-10 Sxx (the predictor is constant over O_t), Syy_t = 0 or df_t < 1: its r is NaN, it is
 * never selected, and it is counted in n_undefined.  With covariates and missing values the predictors were residualised
 * over all rows, not over O_t: the same approximation as in the fit.
 * The p1 q work runs on the f64 matrix pipe, one workgroup per tile of predictors x traits contracting over all n samples
 * (2 n p1 q flop for complete Y; with missing values three products from the same operand reads, 6 n p1 q), and the
 * selection happens in registers: nothing of size p1 q is allocated unless r_dense is given.  No floating-point atomics: two
 * calls on one handle give the same set of rows and the same bits in every other output; the order of the rows is unspecified.
 *   aq_prep_marginal       r2_cut: q doubles, trait t selects the pairs with r^2 >= r2_cut[t] (+inf: none).  cap: rows of the
 *                          table snp / trait / r (int32, int32, double; cap = 0 only counts); n_pairs: the number of
 *                          selected pairs, always the full count, of which min(n_pairs, cap) rows are written.  rs: int64[p1],
 *                          selected traits per predictor.  best_snp: int32[q], the predictor of largest r^2 per trait, the
 *                          lowest index on a tie, -1 where the trait has no defined pair; best_r: double[q], its r (NaN
 *                          there).  n_undefined: int64.  r_dense: NULL, or p1 x q column-major on the host.  Any output may
 *                          be NULL.  The handle is not changed.
 *   aq_mscreen_plan_query  the launch plan without a device, a pure function of its arguments: tile edge (complete Y: 128 when
 *                          the 128 x 128 tiles alone give every CU a workgroup, else 64; masked: 64), samples per step, tile
 *                          counts (the grid is n_tiles = tiles_p tiles_q workgroups), static LDS and scratch.  The environment
 *                          variable AQ_MSCREEN_TILE (64 | 128; tests) forces the tile edge of the complete instance in
 *                          aq_prep_marginal; the query does not read it.
 *   aq_prep_marginal_time  measurement: the kernels of one screen `reps` times between two events after one warm-up, counting
 *                          only (cap = 0, r2_cut = 40 / (40 + df_t)), without the copies and without the per-trait pass over
 *                          Yc (Syy_t, m_t: O(n q), it also decides the plan and runs before); ms_per_call and, if not NULL,
 *                          the plan used.
 * A NULL r2_cut, cap < 0, a NULL handle or a NaN cutoff are AQ_ERR_ARG, in this order, before any device call.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_mscreen_plan {
  int32_t tile;               /* edge of a tile: predictors and traits per workgroup, 64 or 128 */
  int32_t sample_chunk;       /* samples staged per step                                     */
  int32_t tiles_p;            /* ceil(p1 / tile)                                             */
  int32_t tiles_q;            /* ceil(q / tile)                                              */
  int32_t masked;             /* 1: the three-stream instance for Yc with missing values     */
  int32_t lds_bytes;          /* static LDS of a workgroup, <= 64 KiB                        */
  int64_t n_tiles;            /* tiles_p tiles_q: the grid                                   */
  int64_t scratch_bytes;      /* each trait's best predictor per row of tiles: 12 tiles_p q  */
} aq_mscreen_plan;
int aq_mscreen_plan_query(int32_t n, int32_t p1, int32_t q, int32_t masked, int32_t ncu, aq_mscreen_plan *out);
int aq_prep_marginal(aq_prep_handle h, const double *r2_cut, int64_t cap, int32_t *snp, int32_t *trait, double *r, int64_t *n_pairs,
                     int64_t *rs, int32_t *best_snp, double *best_r, int64_t *n_undefined, double *r_dense);
int aq_prep_marginal_time(aq_prep_handle h, int32_t reps, double *ms_per_call, aq_mscreen_plan *plan_out);

/* ------------------------------------------------------------------------------------------
 * Permutation nulls of the marginal screen.  Permutation b is an int32 vector perm[b] of length n, a permutation of
 * 0 ... n - 1; the permuted response is Y'[i, t] = Yc[perm[b][i], t]: the rows of Yc move, all traits together and the NaN
 * pattern with the values, and Xs is untouched, so the LD among predictors and the correlation among traits stay and only the
 * link between the two is broken.  For every b the statistic of aq_prep_marginal is evaluated on (Xs, Y') by the same
 * definition: the same undefined rule and the same m_t, Syy_t and df_t, which do not change with the permutation.  Kept per
 * permutation, and nothing else (no object of size p1 q exists and no pair table is written):
 *   max_r2[b][t]  the largest defined r^2 of trait t over all predictors; -1.0 where the trait has no defined pair
 *   hs_max[b]     the largest number of traits with r^2 >= r2_cut[t] that one predictor has (the largest null hotspot)
 *   n_sel[b]      the number of selected pairs;   n_undef[b]  the number of undefined pairs
 * The permutations run in batches: a gather kernel writes the permuted panels Yp[batch][q][n] of a batch (at most 1 GiB), a
 * tile kernel on the f64 matrix pipe stages each panel of Xs once for PB permutations, and a reduce kernel turns the
 * per-predictor counts into hs_max and n_sel.  No floating-point atomics (max_r2 is an integer maximum over bit patterns of
 * non-negative values): two calls with the same arguments return the same bits in every output.  Every output element is
 * accumulated over the samples in the order of aq_prep_marginal, so the identity permutation returns max_r2 = best_r^2 of
 * aq_prep_marginal to the bit, whatever the tile edge and PB.
 *   aq_prep_marginal_perm       r2_cut: q doubles, as in aq_prep_marginal.  perm: [n_perm][n] int32, row-major.  max_r2:
 *                               [n_perm][q] doubles, row-major; hs_max, n_sel, n_undef: int64[n_perm].  Any output may be
 *                               NULL.  The handle is not changed.
 *   aq_msperm_plan_query        the launch plan without a device, a pure function of its arguments: the tile edge of
 *                               aq_mscreen_plan_query; PB (complete Y: 2 at tile 64, 1 at tile 128; masked: 1); batch, the
 *                               largest multiple of PB with batch q n 8 <= 2^30 and batch scratch_per_perm <= 2^30, cut to
 *                               n_perm rounded up to PB and to a grid below 2^31 workgroups; PB = 1 where PB panels exceed
 *                               1 GiB; AQ_ERR_UNSUPPORTED where one panel does.  The environment variables AQ_MSCREEN_TILE,
 *                               AQ_MSPERM_PB (complete Y: 1 | 2 | 4 at tile 64, 1 at tile 128; masked: 1 | 2) and
 *                               AQ_MSPERM_BATCH (a multiple of PB within the bounds above) force the three in
 *                               aq_prep_marginal_perm (tests, small shapes); the query does not read them.
 *   aq_prep_marginal_perm_time  measurement: the gather, tile and reduce kernels of n_perm permutations (generated rows)
 *                               `reps` times between two events after one warm-up, without the copies; the milliseconds of
 *                               ONE permutation and, if not NULL, the plan used.
 * n_perm < 1, a NULL r2_cut or perm, a NULL handle, a NaN cutoff and a row of perm that is not a permutation of 0 ... n - 1
 * (the message names the row) are AQ_ERR_ARG, in this order, before any device call: an index out of range never reaches a
 * kernel.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_msperm_plan {
  int32_t tile;               /* edge of a tile: predictors and traits per workgroup, 64 or 128 */
  int32_t pb;                 /* permutations per workgroup: they share the staged panel of Xs  */
  int32_t batch;              /* permutations per launch, a multiple of pb                      */
  int32_t launches;           /* ceil(n_perm / batch); the last one may be ragged               */
  int32_t tiles_p;            /* ceil(p1 / tile)                                                */
  int32_t tiles_q;            /* ceil(q / tile): the grid is tiles_p tiles_q ceil(nb / pb)      */
  int32_t masked;             /* 1: the three-stream instance for Yc with missing values        */
  int32_t lds_bytes;          /* static LDS of a workgroup, <= 64 KiB                           */
  int64_t yp_bytes;           /* the gathered panels: 8 batch q n <= 2^30                       */
  int64_t scratch_bytes;      /* batch (4 p1 + 16 q + 4 n + 24): counts, maxima, perm rows      */
} aq_msperm_plan;
int aq_msperm_plan_query(int32_t n, int32_t p1, int32_t q, int32_t masked, int32_t ncu, int32_t n_perm, aq_msperm_plan *out);
int aq_prep_marginal_perm(aq_prep_handle h, const double *r2_cut, int32_t n_perm, const int32_t *perm, double *max_r2, int64_t *hs_max,
                          int64_t *n_sel, int64_t *n_undef);
int aq_prep_marginal_perm_time(aq_prep_handle h, int32_t n_perm, int32_t reps, double *ms_per_perm, aq_msperm_plan *plan_out);

/* ------------------------------------------------------------------------------------------
 * Cis scan of a finished handle: every trait (gene) tested only against the predictors of its own window, and the
 * permutation null of its best cis predictor.  The window of trait t is a half-open range of indices into the handle's
 * CURRENT matrix Xs (p1 columns): s_lo[t] <= s < s_hi[t], 0 <= s_lo[t] <= s_hi[t] <= p1; an empty window is allowed.  The
 * statistic, the rule for an undefined pair, m_t, Syy_t and df_t are those of the marginal screen above.  A pair outside its
 * trait's window does not exist: it is neither selected, nor counted as undefined, nor a candidate for the best predictor.
 * Only the band is computed.  The traits are ordered by (s_lo, s_hi, t), those with an empty window last; 64 consecutive
 * traits of the order form a trait tile with the union range [L, H) of their windows; the work items of a tile are the
 * predictor ranges [p0, p0 + 64), p0 = L, L + 64, ... < H, and a plain grid of one workgroup per item takes the place of the
 * grid of all predictor tiles x trait tiles.  The traits' columns are copied into the order once per call, so a tile's traits
 * are contiguous.  Every pair is accumulated over the samples in the order of the marginal screen (steps of 4, one matrix
 * instruction per step) and goes through the same epilogue: r of a pair inside its window is r_dense of aq_prep_marginal on
 * the same handle to the bit, and max_r2 of the identity permutation is best_r^2.  No floating-point atomics: two calls give
 * the same set of rows and the same bits in every other output; the order of the rows is unspecified.
 *   aq_prep_cis        r2_cut: q doubles, trait t selects its in-window pairs with r^2 >= r2_cut[t] (+inf: none).  cap: rows
 *                      of the table snp / trait / r (cap = 0 only counts); n_pairs: always the full count, of which
 *                      min(n_pairs, cap) rows are written.  best_snp: int32[q], the in-window predictor of largest r^2, the
 *                      lowest index on a tie, -1 where the window holds no defined pair; best_r: double[q], its r (NaN
 *                      there).  n_undef: int64[q], undefined pairs inside each trait's window.  plan_out: the plan used.
 *                      Any output may be NULL.  The handle is not changed.
 *   aq_prep_cis_perm   perm: [n_perm][n] int32 as in aq_prep_marginal_perm.  max_r2: [n_perm][q] doubles, row-major, the
 *                      largest defined r^2 of trait t over its window under permutation b; -1.0 where there is none.
 *   aq_cis_plan_query  the plan without a device, a pure function of its arguments; n_perm = 0 plans the scan alone (pb,
 *                      batch, launches, perm_lds_bytes, yp_bytes = 0).  PB: complete Y 2, masked 1 (measured: DESIGN.md
 *                      section 9; the defaults of aq_msperm_plan_query at tile 64); the batch by the rules there, with the panel 8 n
 *                      max(q_active, 1) bytes.  The environment variables AQ_CIS_PB (complete Y: 1 | 2 | 4; masked: 1 | 2)
 *                      and AQ_CIS_BATCH (a multiple of PB within the bounds) force the two in aq_prep_cis_perm and
 *                      aq_prep_cis_time (tests, small shapes); the query does not read them.  More than 2^31 - 1 work items
 *                      or a panel above 1 GiB are AQ_ERR_UNSUPPORTED.
 *   aq_prep_cis_time   measurement: ms_scan, the kernels of one scan (the ordered copy of Y, the column sums, the tile
 *                      kernel, the reduction of the bests), counting only, cutoffs as in aq_prep_marginal_time; ms_per_perm,
 *                      with n_perm >= 1, the gather, tile and reduce kernels of n_perm generated permutations, per
 *                      permutation (n_perm = 0: not measured, 0.0).  Each `reps` times between two events after a warm-up.
 * AQ_ERR_ARG, in this order, before any device call: n_perm < 1 (aq_prep_cis_perm); a NULL s_lo, s_hi, r2_cut or perm;
 * cap < 0; a NULL handle; a bound outside [0, p1] or s_lo > s_hi (the message names the trait); a NaN cutoff; a row of perm
 * that is not a permutation of 0 ... n - 1.  No index out of range reaches a kernel.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_cis_plan {
  int32_t tile;               /* edge of a work item: predictors and traits per workgroup, 64     */
  int32_t sample_chunk;       /* samples staged per step                                         */
  int32_t trait_tiles;        /* ceil(q_active / tile)                                           */
  int32_t q_active;           /* traits with a non-empty window                                  */
  int32_t masked;             /* 1: the three-stream instances for Yc with missing values        */
  int32_t lds_bytes;          /* static LDS of a workgroup of the scan, <= 64 KiB                */
  int32_t perm_lds_bytes;     /* ... of the permutation kernel                                   */
  int32_t pb;                 /* permutations per workgroup: they share the staged panel of Xs   */
  int32_t batch;              /* permutations per launch, a multiple of pb                       */
  int32_t launches;           /* ceil(n_perm / batch); the last one may be ragged                */
  int64_t n_items;            /* W, the work items: the grid of the scan                         */
  int64_t window_pairs;       /* sum of s_hi - s_lo: the pairs that exist                        */
  int64_t staged_pairs;       /* tile tile W >= window_pairs; the ratio is the fill of the band  */
  int64_t yp_bytes;           /* the gathered panels of a launch: 8 batch max(q_active, 1) n     */
  int64_t scratch_bytes;      /* 12 tile W (each item's best per trait) + batch (16 q + 4 n)     */
} aq_cis_plan;
int aq_cis_plan_query(int32_t n, int32_t p1, int32_t q, int32_t masked, int32_t ncu, const int32_t *s_lo, const int32_t *s_hi,
                      int32_t n_perm, aq_cis_plan *out);
int aq_prep_cis(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, const double *r2_cut, int64_t cap, int32_t *snp,
                int32_t *trait, double *r, int64_t *n_pairs, int32_t *best_snp, double *best_r, int64_t *n_undef,
                aq_cis_plan *plan_out);
int aq_prep_cis_perm(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, int32_t n_perm, const int32_t *perm, double *max_r2);
int aq_prep_cis_time(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, int32_t n_perm, int32_t reps, double *ms_scan,
                     double *ms_per_perm, aq_cis_plan *plan_out);

/* ------------------------------------------------------------------------------------------
 * Conditional cis scan of a finished handle: the scan of aq_prep_cis after each trait's own conditioning variants have been
 * regressed out of the trait and of every predictor, which asks whether a second, independent signal sits in a window or only
 * LD proxies of the first (the conditional pass of FastQTL, QTLtools and tensorQTL's map_independent).
 * The statistic.  Complete Y only.  Xs and Yc are the prepared matrices of the handle, centred and, with covariates,
 * residualised; n_cov as in aq_prep_marginal.  Trait t has a conditioning list C_t of 0 <= k_t <= 4 distinct predictor
 * indices in [0, p1), in the order given, independent of the trait's window: cond_idx[cond_ptr[t]] ... cond_idx[cond_ptr[t + 1] - 1].
 *   Basis.  Go through C_t in order.  v = Xs[:, c].  Project out the basis vectors accepted so far, twice: in each of two
 *   passes, for every accepted q in the order of acceptance, v <- v - q (q'v) (Gram-Schmidt with one re-orthogonalisation).
 *   If |v|^2 <= 1e-10 |Xs[:, c]|^2 the column is dropped: a conditioning variant collinear with the earlier ones.  Otherwise
 *   q = v / |v| is accepted.  k_eff[t] is the number accepted.
 *   Residual trait.  y~_t = y_t - sum_j q_tj (q_tj' y_t), S~yy_t = sum y~^2.  With k_eff = 0, y~_t is the copy of y_t.
 *   Per pair with s_lo[t] <= s < s_hi[t]:  a_j = q_tj' x_s;  Vx = (Sxx - Sx^2 / n) - (a_1^2 + ... + a_k^2), the parenthesis
 *   evaluated first, exactly as the plain scan does;  r = (x_s' y~_t) / sqrt(Vx S~yy_t);  df_t = n - 2 - n_cov - k_eff[t].
 *   Undefined pairs.  A pair is undefined when Vx <= 1e-10 Sxx, when S~yy_t <= 1e-10 Syy_t, or when df_t < 1.  Its r is NaN;
 *   it is counted and never selected.  The first condition removes each conditioning variant from its own trait's tests, and
 *   anything collinear with the list.
 * r is the partial correlation of x_s and y_t given the list, so t = r sqrt(df_t / (1 - r^2)) is the t statistic of x_s in the
 * regression of y_t on x_s and the list.  The sums factor into 1 + KC dense products against one staged panel of Xs (the
 * numerators, and one product per basis vector), KC = the smallest of 1, 2, 4 that holds the longest list of a trait with a
 * window; nothing of size p1 q is stored.  A trait with an empty list gets r, best_snp, best_r and n_undef of aq_prep_cis on
 * the same handle to the bit, whatever the other traits' lists are.  No floating-point atomics: two calls give the same set
 * of rows and the same bits in every other output.
 *   aq_prep_cis_cond        r2_cut, cap, snp, trait, r, n_pairs, best_snp, best_r, n_undef: as for aq_prep_cis.  k_eff:
 *                           int32[q], 0 for a trait with an empty window (its basis is not formed).  plan_out: the plan used.
 *                           Any output may be NULL.  The handle is not changed.
 *   aq_ciscond_plan_query   the plan without a device, a pure function of its arguments (the lists enter by their lengths).
 *                           A list longer than 4, or basis panels and residual traits above 4 GiB together, are
 *                           AQ_ERR_UNSUPPORTED, as is what aq_cis_plan_query refuses.
 *   aq_prep_cis_cond_time   measurement, after aq_prep_cis_time: ms_basis, the basis kernel alone; ms_scan, the other kernels
 *                           of one scan (the column sums, the tile kernel, the reduction of the bests), counting only, with
 *                           the cutoff t^2 = 40 at df_t.  Each `reps` times between two events after a warm-up.
 * AQ_ERR_ARG, in this order, before any device call: a NULL r2_cut (ms_basis, ms_scan); cap < 0 (reps < 1); a NULL s_lo, s_hi,
 * cond_ptr or cond_idx; a NULL handle; cond_ptr[0] != 0 or decreasing offsets; a list longer than 4; an index outside
 * [0, p1); an index repeated within a trait; the window errors of aq_prep_cis; a NaN cutoff.  A handle whose Y has missing
 * values is AQ_ERR_UNSUPPORTED, and the message says so.  No index out of range reaches a kernel.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_ciscond_plan {
  aq_cis_plan cis;            /* the plan of the windows: complete Y, no permutations             */
  int32_t kc;                 /* the tile kernel's instance: 0 (the plain scan's), 1, 2 or 4      */
  int32_t max_k;              /* the longest list of a trait with a window                        */
  int32_t lds_bytes;          /* static LDS of a workgroup of that instance, <= 64 KiB            */
  int32_t streams;            /* 1 + kc matrix-instruction streams per staged panel of Xs         */
  int64_t qo_bytes;           /* the basis panels: 8 kc max(q_active, 1) n                        */
  int64_t yo_bytes;           /* the residual traits: 8 max(q_active, 1) n                        */
} aq_ciscond_plan;
int aq_ciscond_plan_query(int32_t n, int32_t p1, int32_t q, int32_t ncu, const int32_t *s_lo, const int32_t *s_hi,
                          const int32_t *cond_ptr, aq_ciscond_plan *out);
int aq_prep_cis_cond(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, const int32_t *cond_ptr, const int32_t *cond_idx,
                     const double *r2_cut, int64_t cap, int32_t *snp, int32_t *trait, double *r, int64_t *n_pairs, int32_t *best_snp,
                     double *best_r, int64_t *n_undef, int32_t *k_eff, aq_ciscond_plan *plan_out);
int aq_prep_cis_cond_time(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, const int32_t *cond_ptr, const int32_t *cond_idx,
                          int32_t reps, double *ms_basis, double *ms_scan, aq_ciscond_plan *plan_out);

/* ------------------------------------------------------------------------------------------
 * Interaction cis scan of a finished handle: for every in-window pair, whether the effect of the predictor on the trait
 * depends on a sample-level variable e (cell-type fraction, sex, age, treatment): the genotype x environment pass of an eQTL
 * pipeline, tensorQTL's map_cis(interaction_df=).  The windows, the order of the traits and the work items are those of
 * aq_prep_cis.
 * The statistic.  Complete Y only.  Xs [p1][n] and Yc [q][n] are the handle's prepared matrices.  B is nb orthonormal
 * n-vectors spanning [1, Z, e], Z the covariates the handle was prepared with, nb = n_cov + 2: basis[k n + i] is entry i of
 * b_k.  m is the per-sample multiplier: e centred, n doubles (mult).
 *   Per trait t:      y' = y_t - sum_k b_k (b_k'y_t), in the order of B;  S'yy_t = sum y'^2;  S0yy_t is the Syy_t of the
 *                     plain scan.
 *   Per predictor s,  with g = Xs[:, s] and w = g o m, every product rounded once:
 *                     a_k = b_k'g;  c_k = b_k'w;  Sxx = g'g;  Sww = w'w;
 *                     Vg = Sxx - sum a_k^2;  Cgw = g'w - sum a_k c_k;  Vw = Sww - sum c_k^2 - Cgw^2 / Vg.
 *   Per in-window pair (s_lo[t] <= s < s_hi[t]):  Sgy = g'y' and Swy = w'y', the two matrix-instruction streams, both fed
 *                     from one staged panel of Xs, w formed in registers;
 *                     num = Swy - (Cgw / Vg) Sgy;  S'' = S'yy - Sgy^2 / Vg;  r = num / sqrt(Vw S'').
 *   df = n - nb - 2 and t = r sqrt(df / (1 - r^2)).
 * r is the partial correlation of the interaction term g o e with the trait given the intercept, Z, e and g, so this t is the
 * OLS t of the coefficient of g o e in y ~ 1 + Z + e + g + g o e.
 *   Undefined pairs.  A pair is undefined when Vg <= 1e-10 Sxx, Vw <= 1e-10 Sww, S'' <= 1e-10 S0yy_t, or df < 1.  Its r is
 *   NaN; it is counted in n_undef and never selected.  Two realistic cases: a variant that is zero outside one level of a
 *   binary e, where g o m is collinear with [g, e]; a variant that equals e.
 * No floating-point atomics: two calls give the same set of rows and the same bits in every other output.
 *   aq_prep_cis_int        r2_cut, cap, snp, trait, r, n_pairs, best_snp, best_r, n_undef: as for aq_prep_cis.  int_tol:
 *                          double[p1], Vw / Sww, the share of the interaction term that [1, Z, e, g] leave; NaN where the
 *                          predictor itself is undefined (one of the first two rules).  plan_out: the plan used.  Any output
 *                          may be NULL.  The handle is not changed.
 *   aq_cisint_plan_query   the plan without a device, a pure function of its arguments.  What aq_cis_plan_query refuses,
 *                          and residual traits above 4 GiB, are refused here.
 *   aq_prep_cis_int_time   measurement, after aq_prep_cis_cond_time: ms_stats, the per-predictor kernel and the trait
 *                          residuals; ms_scan, the rest of one scan (the tile kernel, the reduction of the bests), counting
 *                          only, with the cutoff t^2 = 40 at df.  Each `reps` times between two events after a warm-up.
 * AQ_ERR_ARG, in this order, before any device call: a NULL s_lo, s_hi, basis, mult or r2_cut (ms_stats, ms_scan) or a NULL
 * handle; cap < 0 (reps < 1); n_basis < 1 (n_basis > 256 is AQ_ERR_UNSUPPORTED at this place, and the message says that at
 * most 256 basis vectors are supported); a non-finite entry of basis or of mult; max |B'B - I| > 1e-8; mult outside
 * span(B), |m - B B'm|^2 > 1e-10 |m|^2; mult all zero; the window errors of aq_prep_cis; a NaN cutoff.  A handle whose Y has
 * missing values is AQ_ERR_UNSUPPORTED, and the message says so.  No index out of range reaches a kernel.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_cisint_plan {
  aq_cis_plan cis;            /* the plan of the windows: complete Y, no permutations             */
  int32_t streams;            /* 2 matrix-instruction streams per staged panel of Xs              */
  int32_t n_basis;            /* nb                                                               */
  int32_t lds_bytes;          /* static LDS of a workgroup of the tile kernel, <= 64 KiB          */
  int32_t mult_pad;           /* doubles of the zero-padded multiplier: n up to whole chunks      */
  int64_t yo_bytes;           /* the residual traits: 8 max(q_active, 1) n                        */
  int64_t pred_bytes;         /* per predictor Vg, Cgw / Vg, Vw, int_tol and the flag: 36 p1      */
  int64_t basis_bytes;        /* the basis and the padded multiplier: 8 (nb n + mult_pad)         */
} aq_cisint_plan;
int aq_cisint_plan_query(int32_t n, int32_t p1, int32_t q, int32_t ncu, const int32_t *s_lo, const int32_t *s_hi, int32_t n_basis,
                         aq_cisint_plan *out);
int aq_prep_cis_int(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, const double *basis, int32_t n_basis, const double *mult,
                    const double *r2_cut, int64_t cap, int32_t *snp, int32_t *trait, double *r, int64_t *n_pairs, int32_t *best_snp,
                    double *best_r, int64_t *n_undef, double *int_tol, aq_cisint_plan *plan_out);
int aq_prep_cis_int_time(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, const double *basis, int32_t n_basis,
                         const double *mult, int32_t reps, double *ms_stats, double *ms_scan, aq_cisint_plan *plan_out);

/* ------------------------------------------------------------------------------------------
 * Cis fine-mapping of a finished handle: per trait the credible sets of the variants that carry its independent signals, by
 * SuSiE (the sum of L single effects, fitted by IBSS; tensorQTL's susie.map), over the predictors of the trait's own window.
 * The windows, the order of the traits and the work items are those of aq_prep_cis.
 * The model.  Complete Y only.  The fit is on the handle's own matrices, Xs [p1][n] and Yc [q][n], without further centring
 * or scaling: susieR's susie(standardize = FALSE, intercept = FALSE).  Per trait with window [lo, hi) and effects l < L:
 * d_s = x_s'x_s; a predictor with d_s <= 1e-10 n has prior weight 0 and is counted in n_undef, the other P have the weight
 * pi = 1 / P.
 *   Start.          alpha = pi, mu = 0, fit_l = 0, sigma2 = y'y / (n - 1), V_l = scaled_prior_variance y'y / (n - 1), ELBO = -inf.
 *   An iteration.   Rf = y - sum_l fit_l, subtracted in the order l = 0 ... L - 1.  Then for l = 0 ... L - 1:
 *                   r_l = Rf + fit_l;  z_s = x_s'r_l;
 *                   lbf_s = 1/2 log(sigma2 / (sigma2 + V_l d_s)) + 1/2 z_s^2 V_l / (sigma2 (sigma2 + V_l d_s)), 0 if V_l = 0;
 *                   alpha_s = pi exp(lbf_s) / sum pi exp(lbf), the largest lbf taken out first;  lbf_model = log sum pi exp(lbf);
 *                   v_s = 1 / (d_s / sigma2 + 1 / V_l);  mu_s = v_s z_s / sigma2;  mu2_s = v_s + mu_s^2;
 *                   V_l <- sum alpha_s mu2_s, used from the next iteration on, and V_l <- 0 if lbf_model at that new V_l is <= 0;
 *                   fit_l <- sum_s x_s alpha_s mu_s;  Rf <- r_l - fit_l;
 *                   KL_l = -lbf_model + (2 sum z_s alpha_s mu_s - sum d_s alpha_s mu2_s) / (2 sigma2).
 *   After them.     ERSS = |Rf|^2 + sum_l (sum_s d_s alpha_ls mu2_ls - |fit_l|^2);
 *                   ELBO = -(n / 2) log(2 pi sigma2) - ERSS / (2 sigma2) - sum_l KL_l with the sigma2 the iteration used.
 *                   The trait has converged if tol > 0 and ELBO - ELBO_prev < tol; otherwise sigma2 <- ERSS / n.  At most
 *                   max_iter iterations; tol = 0 never converges.  A converged trait's state is not written again.
 * x'r_l over the window is the cis tile loop with the residuals in the place of the traits, X (alpha mu) its banded
 * transpose, both on the f64 matrix pipe for the 64 traits of a trait tile at once; consecutive trait tiles run in lockstep
 * in batches whose alpha and mu stay within a budget (aq_finemap_plan).  Traits are independent: the batches change no bit,
 * and neither does `active`, which leaves the tiles as they are.  Every sum runs in a fixed order and no floating-point atomic
 * is used: two calls give the same set of rows and the same bits in every other output.
 *   aq_prep_cis_finemap       active: int32[q] or NULL (all); a trait with active[t] = 0 is not fitted and NO output of it is
 *                             written.  cap: rows of the table (0 only counts); n_rows: always the full count.  A row is
 *                             (snp, trait, effect l, alpha, mu, mu2) of the iteration in which the trait stopped, for every
 *                             effect whose final V_l > 0 and every in-window predictor with alpha >= thr_t =
 *                             min(alpha_min, 0.1 (1 - coverage) / P): the mass an effect loses is below 0.1 (1 - coverage).
 *                             sigma2: double[q]; V, lbf: double[q][L] (the final V_l; lbf_model of the last iteration);
 *                             elbo_trace: double[max_iter][q], NaN where the trait did not run; n_iter, converged: int32[q];
 *                             n_undef: int64[q].  alpha_dense, mu_dense: double[q][L][p1], 0.0 outside the window (tests and
 *                             small problems: they go through the host).  A trait with an empty window, or without a
 *                             predictor of prior weight, gets no rows, n_iter = 0 and NaN in sigma2, V, lbf.  Any output
 *                             may be NULL.  The handle is not changed.
 *   aq_finemap_plan_query     the plan without a device: a function of its arguments and of the environment variable
 *                             AQ_FM_BATCH_TILES (>= 1; tests, small shapes), which forces the trait tiles per batch in the
 *                             entries and which the query reads as they do.  L outside [1, 16] is AQ_ERR_ARG.
 *   aq_prep_set_purity        set b = the columns set_idx[set_ptr[b]] ... set_idx[set_ptr[b + 1] - 1], 1 ... 100 of them:
 *                             min_abs_r[b] and mean_abs_r[b], the smallest and the mean |Pearson correlation| over its pairs
 *                             of columns of Xs; 1 and 1 for a set of one; a pair with a constant column counts as 0.
 *   aq_prep_cis_finemap_time  measurement: the four kernels of one iteration at the default parameters, each `reps` times
 *                             between two events after a warm-up: ms_xtr, ms_ser, ms_fit (L launches each) and ms_iter_end,
 *                             summed over the batches.
 * AQ_ERR_ARG, in this order, before any device call: a NULL s_lo or s_hi; NULL params; L outside [1, 16]; max_iter < 1; tol
 * negative or not finite; scaled_prior_variance not positive; coverage outside (0, 1); alpha_min outside [0, 1]; cap < 0; a
 * NULL handle; the window errors of aq_prep_cis.  A handle whose Y has missing values is AQ_ERR_UNSUPPORTED, and the message
 * says so.  No index out of range reaches a kernel.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_finemap_params {
  int32_t L;                  /* single effects, 1 ... 16                                          */
  int32_t max_iter;           /* most IBSS iterations                                             */
  double tol;                 /* converged when the ELBO gains less; 0: never                     */
  double scaled_prior_variance; /* V_l at the start, as a share of y'y / (n - 1)                  */
  double coverage;            /* of the credible sets the rows are meant for: enters thr_t        */
  double alpha_min;           /* rows with alpha below min(alpha_min, 0.1 (1 - coverage) / P) are dropped */
} aq_finemap_params;
typedef struct aq_finemap_plan {
  aq_cis_plan cis;            /* the plan of the windows: complete Y, no permutations             */
  int32_t L;                  /* single effects                                                   */
  int32_t batch_tiles;        /* trait tiles that run in lockstep: batch b = tiles [b batch_tiles, ...) */
  int32_t n_batches;          /* ceil(trait_tiles / batch_tiles)                                  */
  int32_t forced;             /* 1: batch_tiles is AQ_FM_BATCH_TILES                              */
  int64_t state_budget;       /* the bound on alpha and mu of a batch, 4 GiB                      */
  int64_t state_bytes;        /* alpha and mu of the largest batch: 2 L 64 64 8 per work item     */
  int64_t band_bytes;         /* its band buffer x'r: 64 64 8 per work item                       */
  int64_t fit_bytes;          /* its residuals and fits: 8 (L + 2) n per trait                    */
} aq_finemap_plan;
int aq_finemap_plan_query(int32_t n, int32_t p1, int32_t q, int32_t ncu, const int32_t *s_lo, const int32_t *s_hi, int32_t L,
                          aq_finemap_plan *out);
int aq_prep_cis_finemap(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, const int32_t *active,
                        const aq_finemap_params *params, int64_t cap, int32_t *row_snp, int32_t *row_trait, int32_t *row_effect,
                        double *row_alpha, double *row_mu, double *row_mu2, int64_t *n_rows, double *sigma2, double *V, double *lbf,
                        double *elbo_trace, int32_t *n_iter, int32_t *converged, int64_t *n_undef, double *alpha_dense, double *mu_dense,
                        aq_finemap_plan *plan_out);
int aq_prep_set_purity(aq_prep_handle h, const int32_t *set_ptr, const int32_t *set_idx, int32_t n_sets, double *min_abs_r,
                       double *mean_abs_r);
int aq_prep_cis_finemap_time(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, int32_t L, int32_t reps, double *ms_xtr,
                             double *ms_ser, double *ms_fit, double *ms_iter_end, aq_finemap_plan *plan_out);

/* ------------------------------------------------------------------------------------------
 * Prediction: the fitted model applied to genotypes,
 *   Yhat = Xt B,   B = beta_vb = gam_vb * mu_beta_vb (p x q, R/update_vb.R:17),   Xt = (X_new - center) / scale per column,
 * n_new x q: the genetic component of the traits on the scale of the prepared Y, in-sample (the X_beta_vb that the reference's
 * man page lists and its code never returns: the update is commented out at src/coreLoop.cpp:100, R/update_vb.R:52) or for
 * new samples.  B is read where it lies: the trait-tiled gam_vb and mu_beta_vb of the handle are multiplied in registers into
 * the B operand of the f64 matrix instruction, a row at or beyond p or a trait at or beyond q is replaced by 0.0 there
 * (whatever the padding of the storage holds), and nothing of size p q is allocated -- so a run whose p x q matrices never
 * leave the device (sparse output) can be predicted from.  A pre-pass writes Xt from the uploaded fp64 or int8 columns as
 * (x - center) (1 / scale), two roundings and the one of 1 / scale, into panels of 16 samples, [n_pad / 16][p_pad][16], with
 * exact zeros in the rows >= n_new and the predictors >= p.  Workgroup (b, g, s) of the grid (sample_blocks, trait_groups,
 * splits) owns sample_tiles tiles of 16 samples (a quarter per wave, every wave holding sample_tiles / 4 x trait_tiles
 * accumulators so that a loaded block of B serves all its sample tiles), trait_tiles tiles of 16 traits and the predictors of
 * split s, chunks_per_split chunks of `chunk` each, and writes its partial tiles to scratch, [splits][ceil(q / 16)][n_pad][16];
 * a second kernel adds the partials of an entry in the order s = 0, 1, ... and writes the column-major result.  No
 * floating-point atomics: two calls return the same bits, and so do two row batches of one matrix whose plans have the same
 * splits.  Every offset is 64-bit.  Every entry is within (p + 8) 2^-53 sum_s |Xt_is B_st| of the exact value.
 *   aq_vb_predict          X_new (n_new x p column-major fp64, host) or, when it is NULL, X_new_i8 (int8 dosages), with the
 *                          handle's p columns; center, scale: p each, or both NULL: the input is standardised already.
 *                          1 <= n_new <= 82 944 (AQ_N_MAX) per call.  Yhat_out: n_new x q column-major, host, q the handle's
 *                          traits.  NaN in X_new is not looked for: it spreads to its row of Yhat.  Synchronises and reports
 *                          an expired in-kernel wait as aq_vb_get_result does.
 *   aq_vb_fitted           the same kernels on a standardised matrix that lies on the handle's device, n x p column-major
 *                          with the handle's n rows: aq_prep_x_device of the prepare handle the fit was made from.
 *   aq_predict             the matrix-level twin for a dense result, as aq_select_pairs is to aq_vb_select_pairs: beta_vb
 *                          (p x q column-major, host) is uploaded into the tiled layout and the same kernels run.
 *   aq_predict_plan_query  the launch plan without a device: a function of its arguments and of the environment variable
 *                          AQ_PREDICT_SPLITS (1 ... 64; tests), which forces the splits of the entries above whatever p and
 *                          the CU count say and which the query reads as they do (as aq_ytrans_plan_query reads AQ_YT_PATH);
 *                          a value outside [1, 64] is AQ_ERR_ARG in all of them.  The entries plan for the device's CU count,
 *                          or for AQ_NCU when it is set (the hook of aq_vb_create's planner; tests reach two trait tiles per
 *                          workgroup at small shapes with it); the query takes the count as its argument.  More than
 *                          1 048 560 traits per call (65 535 trait tiles, the y dimension of the grids) is AQ_ERR_UNSUPPORTED.
 *   aq_vb_predict_time     measurement: the pre-pass (from int8 zeros, center 0, scale 1) and the two kernels `reps` times
 *                          between two events after one warm-up, without the copies from and to the host; ms_per_call and,
 *                          if not NULL, the plan used.
 * A NULL handle, matrix or output, center without scale or the reverse, n_new outside [1, 82 944], p or q < 1 and a scale that
 * is not finite and positive are AQ_ERR_ARG, with the entry's name in aq_last_error(), before any device call.
 * ---------------------------------------------------------------------------------------- */
typedef struct aq_predict_plan {
  int32_t sample_tiles;       /* 16-sample tiles per workgroup: 4, 8 or 16 (1, 2 or 4 per wave)  */
  int32_t trait_tiles;        /* 16-trait tiles per workgroup: 1 or 2                        */
  int32_t sample_blocks;      /* ceil(ceil(n_new / 16) / sample_tiles)                       */
  int32_t trait_groups;       /* ceil(ceil(q / 16) / trait_tiles)                            */
  int32_t splits;             /* workgroups per (block, group), each with its own predictors */
  int32_t chunk;              /* predictors per step: 16                                     */
  int32_t chunks_per_split;   /* split s owns chunks [s chunks_per_split, (s + 1) chunks_per_split) */
  int32_t n_pad;              /* 16 sample_tiles sample_blocks                               */
  int64_t panel_bytes;        /* Xt in panel order: n_pad p_pad doubles, p_pad = p padded to 16 */
  int64_t scratch_bytes;      /* the partial tiles: splits ceil(q / 16) n_pad 16 doubles     */
} aq_predict_plan;
int aq_predict_plan_query(int32_t n_new, int32_t p, int32_t q, int32_t ncu, aq_predict_plan *out);
int aq_vb_predict(aq_vb_handle h, const double *X_new, const int8_t *X_new_i8, int32_t n_new, const double *center,
                  const double *scale, double *Yhat_out);
int aq_vb_fitted(aq_vb_handle h, const double *Xs_device, double *Yhat_out);
int aq_predict(const double *beta_vb, int32_t p, int32_t q, const double *X_new, const int8_t *X_new_i8, int32_t n_new,
               const double *center, const double *scale, double *Yhat_out, int32_t device);
int aq_vb_predict_time(aq_vb_handle h, int32_t n_new, int32_t reps, double *ms_per_call, aq_predict_plan *plan_out);

#ifdef __cplusplus
}
#endif
#endif /* ATLASQTL_HIP_H_ */
