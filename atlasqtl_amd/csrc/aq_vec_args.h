// aq_vec_args.h -- the device-resident scalars and the argument blocks of the vector kernels that surround the core sweep
// (aq_sweep_kernels.h).  Types only, no kernel: every unit that holds or fills one includes this header.
#pragma once

#define AQ_RED_EXTRA 8   // scalars appended to the row-sum all-reduce payload

// Device-resident scalars of the VB state (one struct, updated by 1-thread kernels).
struct AqScalars {
  double sig02_inv;     // horseshoe global precision sig02_inv_vb
  double S_gam;         // sum(gam_vb) over all traits (all-reduced)
  double T2;            // sum_k tau_k * colSums(m2_beta)_k (all-reduced)
  double sum_zeta_old;  // sum(zeta_vb) before this sweep's zeta update (all-reduced)
  double nu_vb, rho_vb, sig2_inv, log_sig2_inv;   // S1-S3, S8
  double rho_xi_inv, xi_inv, nu_s0, rho_s0;       // S13, S15, S18
  double sum_theta;     // sum(theta_vb) after S17
  double sum_sig2_theta;
  double sum_theta_sq;  // global-only core: sum (theta - m0)^2
  double elbo_C;        // e_theta_hs_ / e_theta_ (replicated p-sum)
  double elbo;          // assembled ELBO
  unsigned long long lentz_mask[2];
  int lentz_iters;
  int pad_;
};

// argument block of aq_k_prepass (aq_sweep_kernels.h)
struct AqPrepass {
  const double *theta, *zeta, *gam;
  double *Aarr, *Barr, *rowA, *colApart, *Hpart;
  int p, q, p_pad, q_pad, rows_per_chunk;
  double sqrt_c;
  int c_is_one, do_H;
  int write_AB;   // 0: only the ELBO part (do_H); A, b and the sums of a are produced inside the sweep kernel
};

// argument block of the q-vector kernels, S1-S8
struct AqQvec {
  const double *eta_h, *kappa_h, *n0, *nobs;  // hyper (q_pad), observed-sample counts
  double *zeta, *tau, *sig2b, *log_tau, *eta_vb, *kappa_vb, *coef, *inv2s, *cst;
  double *sums;  // [5][q_pad]: sum gam, sum m2, sum beta^2, sum gam*b, ||R||^2
  const double *colApart;  // [nchunk][q_pad] column sums of the Z intercept a
  int nchunk;
  int q, q_pad, n;
  double nu_h, rho_h;
  int na;   // 1: Y has missing values: kappa uses the X_norm_sq form (R/update_vb.R:150-155), sums[2] = sum_j X_norm_sq (m2 - beta^2),
            //    sums[5] = sum_j gam log sig2_beta_jk (sig2_beta_vb is p x q, R/update_vb.R:45)
};

// argument block of the p-vector kernels, S12-S18
struct AqPvec {
  double *theta, *sig2_theta, *L, *lam2_inv, *Q;
  const double *rsZ;     // all-reduced row sums of Z
  double *part;          // [3][nblk] partial sums: theta, lam*shr*(...), sig2_theta
  int p, p_pad;
  double shr, m0, A2_inv, df;
};
