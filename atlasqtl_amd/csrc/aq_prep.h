// aq_prep.h -- the prepare side's analogue of aq_vb.h: the handle of aq_prepare_data*, the prototype of every host function
// that one aq_prep*.hip unit calls in another, and the timing loop that the *_time entries share.  Every unit that defines
// or calls one of them includes this header, so a definition that differs from its declaration is a compile error.
#pragma once
#include <stdint.h>
#include <vector>

#include "aq_internal.h"   // aq_fail, AQ_HIP, AQ_TRY, aq_need_device, AqDev

struct aq_prep {
  int n = 0, p = 0, q = 0, p_kept = 0, device = 0;
  AqDev<double> Xs;   // n x p_kept, standardised, compact
  AqDev<double> Yc;   // n x q, centred (NaN = missing)
  std::vector<uint8_t> bool_cst, bool_coll;   // p each (bool_coll in the ORIGINAL column numbering)
  std::vector<int32_t> dup_of;                // original index of the kept column a removed duplicate equals, else -1
  std::vector<double> mean, sd;               // p each
  std::vector<int32_t> gcounts;               // 4 x p (hom A1, het, hom A2, missing): aq_prepare_data_bed only
  int n_cov = 0;                              // covariates regressed out of X and Y (0: none)
  std::vector<uint8_t> cov_absorbed;          // p: the covariates explain the column (written as 0.0, reported constant)
  std::vector<double> cov_r2;                 // p: share of the column's variance that the covariates explain
  bool ld_done = false;                       // aq_prep_ld_prune has run: Xs holds the kept columns only
  std::vector<uint8_t> ld_removed;            // p: removed by aq_prep_ld_prune (original numbering, like the two below)
  std::vector<int32_t> ld_of;                 // p: original index of the kept column that tags a removed one, else -1
  std::vector<double> ld_r2;                  // p: r^2 of a removed column with its tag, else NaN
  int yt_method = 0;                          // transform of Y before everything else (0: none, 1: rank-based inverse normal)
  double yt_offset = 0.0;                     // its c
  std::vector<int32_t> yt_nobs, yt_ntied;     // q each: observed values of the trait, and those that share their value
};

// aq_prep_bed.hip (PLINK input)
// the checks of a .bed input after the NULL and shape checks, all on the host
int aq_bed_check_args(const aq_prep_bed_input *in);
// the source step of a .bed input: decode and count; the int8 dosages in *dG when no genotype is missing, else (missing =
// "mean") imputed as fp64 in *dX, else the error.  Fills h->gcounts.
int aq_bed_source(aq_prep *h, const aq_prep_bed_input *in, AqDev<int8_t> *dG, AqDev<double> *dX);

// aq_prep_cov.hip (covariates)
// the checks of a covariate argument and its basis, all on the host: Q is n x (d + 1) afterwards
int aq_cov_host_basis(const aq_prep_cov *cov, int n, const char *who, std::vector<double> *Q);
// x_j <- x_j - Q (Q' x_j) for every column of the device matrix: of the int8 dG into dX, or (dG NULL) of dX in place
int aq_cov_residualise_x(aq_prep *h, const int8_t *dG, double *dX, const double *dQt, int D);
// the residuals of every column of dY on [1, Z] over its observed rows into h->Yc; dnobs, dflag (zero on entry): q ints each.
// Asynchronous.
int aq_cov_residualise_y(aq_prep *h, const double *dY, const double *dQt, int D, int *dnobs, int *dflag);

// aq_prep_ytrans.hip (rank transform)
// the transform argument, before any device call (method 0 asks for nothing and is not looked at further)
int aq_ytrans_check_args(const aq_prep_ytrans *yt, int n, const char *who);
// dY (n x q column-major, device) -> dOut (may be dY); dnobs, dntied, ddeg: q ints each on the device.  Asynchronous after
// the plan: the caller's next copy from the device waits for the kernels.  The current device is the arrays' one.
int aq_ytrans_device(const double *dY, double *dOut, int n, int q, double c, int *dnobs, int *dntied, int *ddeg, const char *who,
                     aq_ytrans_plan *plan_out);
// the first column that cannot be rank-normalised, if any
int aq_ytrans_check_degenerate(const int *deg, int q);

// the *_time entries (aq_prep_grm.hip, aq_prep_marginal.hip): `launch` once as a warm-up, then `reps` times between two events:
// the milliseconds of one call
template <typename F>
int aq_time_launches(int reps, double *ms_per_call, F launch) {
  AQ_TRY(launch());
  AQ_HIP(hipDeviceSynchronize());
  struct Events {                              // both destroyed on every way out
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() {
      for (hipEvent_t ev : e)
        if (ev) hipEventDestroy(ev);
    }
  } ev;
  AQ_HIP(hipEventCreate(&ev.e[0]));
  AQ_HIP(hipEventCreate(&ev.e[1]));
  AQ_HIP(hipEventRecord(ev.e[0], 0));
  for (int r = 0; r < reps; r++) AQ_TRY(launch());
  AQ_HIP(hipEventRecord(ev.e[1], 0));
  AQ_HIP(hipEventSynchronize(ev.e[1]));
  float ms = 0.f;
  AQ_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  *ms_per_call = (double)ms / reps;
  return AQ_OK;
}
