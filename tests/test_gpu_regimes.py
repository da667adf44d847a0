"""GPU: the sweep kernels on linkage disequilibrium, rare variants, traits of very different scale and per-trait
hyper-parameters, against the CPU oracle.

Every other whole-run parity test builds its inputs with tests/util.make_problem: independent Binomial(2, 0.2) SNPs (largest
off-diagonal r^2 about 0.04), no rare variant, traits of variance about 1, and every q-vector of the hyper-parameters and of the
init constant over the traits.  So the in-block Gram terms G_b[j, i] delta_i, the cross-block correction X_{b+1}' X_b delta and the
per-trait Gram blocks G^(k) of the MASK instances were always small corrections to S, X_norm_sq(j, k) was always about n - 1,
the 16 lanes of a trait tile always held constants within a factor of 2 of each other, and a trait index off by a lane, a tile,
a padding column or a shard offset would have changed nothing.  The cases below start from tests/util.make_regime_problem:
  ld         neighbouring SNPs with r^2 up to 0.99, also across every border of 16-SNP blocks and of chained segments, two active
             SNPs among them (47 and 48);
  rare       every 5th SNP with 1, 2 or 3 carriers (a standardised carrier value near sqrt(n)); with missing values all carriers
             of three of them missing in one trait each, where X_norm_sq(j, k) is about 1 and x_j' R_k is pure cancellation;
  scale      Y[:, k] *= 10^s_k, s_k in [-4, 4], both ends inside one trait tile and inside the ragged last one: tau_vb from 1e-8
             to 1e8;
  per_trait  eta_k, kappa_k, n0_k and the initial tau_vb distinct in every trait (nu, rho, t02 not the automatic ones).
tests/test_regime_coverage_host.py asserts, on the CPU, that the inputs of every case here hold what they claim, that the
planner gives every case the kernel instance it is written for, and that rolling eta, kappa, n0 by one trait moves the oracle's
tau_vb and zeta_vb by more than 1000 times the bars below.

Each case runs 1 and 3 sweeps, the ladder and four ELBO evaluations (thinned_elbo_eval = False) and -- the oracle converges
within 150 sweeps on every input, which the CPU file asserts -- a whole run; proves the launched kernel instance from
aq_vb_status; and holds `it`, theta_vb, zeta_vb, mu_beta_vb, tau_vb, lam2_inv_vb, the ELBO trace and gam_vb -- absolutely, and
on the logit scale where the oracle's value is inside (0, 1) -- to the bars below.  Whole runs also hold the residual the handle
carries against a fresh mis_pat .* (Y - X beta_vb), relative to each trait's rms.

Metrics that follow the trait's scale.  mu_beta_vb[j, k] scales with sd(y_k): its bar is rtol |mu| + 1e-10 sd(y_k) (deviations()
returns |d| / (|mu| + 1e-4 sd(y_k)), held to rtol <= 1e-6).  On the entries whose observed rows hold no carrier (X_norm_sq(j, k)
< 4: about 1, 2 or 3, the number of carriers) x_j' R_k is a sum of n terms that cancels to nothing, and two correct
double-precision implementations differ by 3.5e-7 of |mu| there at n = 300: there |mu| is replaced by max(|mu|, the posterior
sd sqrt(sig2_beta(j, k))), sig2_beta(j, k) = 1 / (c (X_norm_sq(j, k) + sig2_inv_vb) tau_k) from the oracle's outputs -- the scale on
which such an entry means anything.

The bars come from the reference side only.  For every distinct input, sweep count and field
    (a) the oracle as it is against the same oracle with log_ndtr / inv_mills_ratio_ at 40 digits, and
    (b) the oracle's Gram-space driver against its n-space form (oracle.sharded_oracle.run_sharded; it states df = 1, so an
        input with df > 1 is measured on its df = 1 twin -- same data, lists and ladder, the same sweep over the p x q entries;
        the global scheme has no (b))
were measured on the CPU with
    python tests/tools/measure_regime_bars.py
and the bar of a field is 10 x max(a, b) over all cases, capped by the bar the rest of the suite holds that field to (CAP).
A case is in the file only if its own (a) and (b) are at most CAP / 10 in every field (the CPU file asserts it from the table
WORST_OF_INPUT, which the same command prints).  MEASURED holds what that command printed for the annealed inputs,
MEASURED_NOANNEAL for the input without a ladder: {sweeps: {field: (a, b)}}.

What the file found when it was written:
  * X_norm_sq(j, k) of the MASK look-ahead instances is the diagonal of the trait's own Gram block, formed as G_jj minus the sum
    over the trait's missing samples.  Where those samples carry almost all of x_j' x_j -- the carriers-missing entries here:
    n - 1 less almost n - 1 leaves about 1 -- the difference kept an absolute error of a few ulp of n, and after three sweeps
    tau_vb was off by 2.9e-13 and 4.1e-13 at n = 1000 (mask-n1000-*), 2.8e-12 and 4.2e-12 at n = 4000 (mask-wide-c12-*, there also
    zeta_vb 1.1e-13 against 6.0e-14) against a bar of 1.7e-13, where the reference's two forms differ by 5.6e-15; 4e-16 ... 9e-16
    after one sweep (which still runs on the init's per-trait sig2_beta_vb), 1e-14 at n = 300, and 2e-15 ... 2e-14 in the
    complete-Y instances and under AQ_KERNEL = 2, 3, which take X_norm_sq directly.  Four orders inside the suite's 1e-8, so no
    earlier test saw it.  Fixed with it: aq_k_gk_diag_exact redoes the entries that keep less than an eighth of G_jj with both
    sums in double-double (atlasqtl_amd/csrc/aq_setup_kernels.h; once per handle).
  * The bars of a run without a ladder cannot come from annealed runs: its first sweeps run at c = 1 and move the state much
    further (df5 after 3 sweeps: gam_vb 2.3e-11 on the GPU, 2.3e-11 between the oracle's two forms on the df = 1 twin, against
    3.6e-12 from the annealed runs).  Hence MEASURED_NOANNEAL, and (b) on the df = 1 twin for the inputs with df > 1."""
import numpy as np
import pytest

from tests.test_gpu_link_range import compared, logit, logit_grain
from tests.test_gpu_split_instances import MASK, WIDE, SEG, _assert_instance

pytestmark = pytest.mark.gpu

ELBO = "elbo"        # the sweep count of an ELBO case: its ladder + ELBO_EVALS sweeps, every one of the latter with an ELBO
WHOLE = "whole"      # a whole run: maxit = WHOLE_MAXIT, the library's thinned ELBO schedule
ELBO_EVALS = 4
WHOLE_MAXIT = 150
SWEEPS = (1, 3, ELBO, WHOLE)

# the suite's bars (tests/test_gpu_split_instances.py::_check, tests/test_gpu_parity.py::_check_state): upper caps
CAP = dict(theta_vb=1e-6, zeta_vb=1e-6, mu_beta_vb=1e-6, tau_vb=1e-8, lam2_inv_vb=1e-6, gam_vb=1e-9, gam_logit=np.inf, elbo=1e-9)
FLOOR = dict(theta_vb=1e-6, zeta_vb=1e-6, tau_vb=0.0, lam2_inv_vb=1e-6)     # relative deviations: |d| / max(|ref|, floor)
MU_ATOL_OVER_RTOL = 1e-10 / 1e-6       # atol = 1e-10 sd(y_k) next to rtol = 1e-6
NO_CARRIER = 4.0                       # X_norm_sq(j, k) below this: the observed rows of trait k hold no carrier of SNP j (it is then
                                       # about the number of carriers, 1 to 3; with one carrier left it is above n / 4)
RESIDUAL_BAR = 1e-10                   # of tests/test_gpu_bigp.py, relative to each trait's rms

# python tests/tools/measure_regime_bars.py  ->  (a), (b) per sweep count and field, maxima over all inputs
MEASURED = {
    1: dict(theta_vb=(7.2e-14, 1.5e-12), zeta_vb=(4.0e-16, 1.5e-15), tau_vb=(0.0e+00, 6.7e-16), lam2_inv_vb=(7.3e-14, 0.0e+00), mu_beta_vb=(3.5e-13, 1.7e-09), gam_vb=(3.3e-15, 8.7e-14), gam_logit=(3.2e-14, 8.3e-13)),
    3: dict(theta_vb=(4.3e-12, 1.1e-11), zeta_vb=(9.8e-16, 6.0e-15), tau_vb=(1.7e-15, 1.7e-14), lam2_inv_vb=(5.7e-14, 2.2e-15), mu_beta_vb=(3.9e-10, 3.3e-09), gam_vb=(3.6e-14, 3.6e-13), gam_logit=(3.1e-13, 2.7e-12)),
    'elbo': dict(theta_vb=(4.7e-12, 6.0e-10), zeta_vb=(2.0e-13, 7.8e-12), tau_vb=(6.3e-13, 1.7e-12), lam2_inv_vb=(1.3e-13, 3.6e-11), mu_beta_vb=(3.0e-10, 6.8e-09), gam_vb=(2.4e-12, 6.3e-11), gam_logit=(2.4e-10, 1.7e-09), elbo=(2.0e-15, 4.6e-14)),
    'whole': dict(theta_vb=(2.3e-11, 1.2e-09), zeta_vb=(9.7e-14, 1.9e-12), tau_vb=(9.0e-15, 8.6e-13), lam2_inv_vb=(1.2e-11, 4.4e-12), mu_beta_vb=(4.0e-10, 8.2e-09), gam_vb=(3.3e-13, 1.5e-11), gam_logit=(2.7e-12, 3.6e-10), elbo=(9.0e-16, 4.2e-14)),
}

# the same command, for the inputs that run without a ladder (here: df = 5).  Their first sweeps run at c = 1 and move the state
# much further than annealed ones, so they take no bar from annealed runs and give none to them.
MEASURED_NOANNEAL = {
    1: dict(theta_vb=(3.5e-13, 6.9e-13), zeta_vb=(2.8e-16, 1.0e-15), tau_vb=(0.0e+00, 3.7e-16), lam2_inv_vb=(1.5e-14, 0.0e+00), mu_beta_vb=(2.2e-15, 9.8e-11), gam_vb=(3.3e-16, 1.4e-14), gam_logit=(5.8e-15, 2.5e-13), elbo=(0.0e+00, 0.0e+00)),
    3: dict(theta_vb=(1.0e-13, 3.0e-11), zeta_vb=(4.6e-16, 8.1e-14), tau_vb=(2.6e-16, 2.0e-13), lam2_inv_vb=(1.1e-14, 2.2e-15), mu_beta_vb=(4.4e-13, 8.6e-10), gam_vb=(6.8e-15, 2.3e-11), gam_logit=(3.3e-14, 1.9e-10), elbo=(0.0e+00, 9.3e-15)),
    'elbo': dict(theta_vb=(7.0e-14, 3.0e-11), zeta_vb=(2.9e-16, 6.0e-14), tau_vb=(1.0e-15, 1.9e-12), lam2_inv_vb=(7.1e-15, 1.8e-13), mu_beta_vb=(3.6e-13, 9.0e-09), gam_vb=(1.6e-14, 6.4e-12), gam_logit=(1.1e-13, 2.6e-10), elbo=(1.7e-16, 2.1e-14)),
    'whole': dict(theta_vb=(5.2e-14, 1.6e-11), zeta_vb=(2.1e-15, 1.4e-13), tau_vb=(2.0e-15, 3.2e-13), lam2_inv_vb=(4.9e-15, 7.8e-14), mu_beta_vb=(2.5e-12, 1.1e-09), gam_vb=(4.4e-15, 3.1e-12), gam_logit=(9.3e-14, 8.9e-11), elbo=(5.3e-16, 9.3e-15)),
}

# the same command: per input, the largest of (a), (b) over the sweep counts it runs here as a fraction of CAP (gam_logit has no cap)
WORST_OF_INPUT = {
    'n1000-q40-ld+rare+scale-na0.0-auto-anneal-df1-global_local': dict(theta_vb=1.8e-06, zeta_vb=4.7e-08, tau_vb=5.0e-06, lam2_inv_vb=4.4e-06, mu_beta_vb=9.8e-04, gam_vb=4.5e-04, elbo=2.0e-06),
    'n1000-q40-ld+rare+scale-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=4.5e-06, zeta_vb=1.4e-07, tau_vb=2.9e-05, lam2_inv_vb=2.6e-07, mu_beta_vb=2.1e-03, gam_vb=2.2e-03, elbo=3.1e-06),
    'n1000-q40-ld+rare+scale-na0.06-auto-anneal-df1-global_local': dict(theta_vb=1.8e-06, zeta_vb=5.0e-09, tau_vb=8.3e-07, lam2_inv_vb=7.3e-08, mu_beta_vb=1.8e-03, gam_vb=1.0e-04, elbo=2.1e-07),
    'n1000-q40-ld+rare+scale-na0.06-per_trait-anneal-df1-global_local': dict(theta_vb=1.2e-04, zeta_vb=1.3e-06, tau_vb=2.8e-05, lam2_inv_vb=9.5e-06, mu_beta_vb=1.9e-03, gam_vb=6.3e-02, elbo=1.1e-05),
    'n1000-q40-ld-na0.0-auto-anneal-df1-global_local': dict(theta_vb=3.0e-06, zeta_vb=3.2e-08, tau_vb=2.1e-06, lam2_inv_vb=1.6e-06, mu_beta_vb=1.5e-05, gam_vb=5.8e-04, elbo=8.8e-07),
    'n1000-q40-ld-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=5.0e-06, zeta_vb=1.6e-08, tau_vb=2.2e-06, lam2_inv_vb=1.3e-07, mu_beta_vb=1.4e-05, gam_vb=5.4e-04, elbo=3.7e-07),
    'n1000-q40-rare-na0.0-auto-anneal-df1-global_local': dict(theta_vb=1.0e-06, zeta_vb=2.8e-09, tau_vb=1.0e-06, lam2_inv_vb=7.3e-08, mu_beta_vb=3.7e-06, gam_vb=1.0e-05, elbo=3.8e-07),
    'n1000-q40-rare-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=2.0e-07, zeta_vb=3.3e-09, tau_vb=9.9e-07, lam2_inv_vb=1.1e-07, mu_beta_vb=2.7e-06, gam_vb=8.5e-06, elbo=2.5e-07),
    'n1000-q40-scale-na0.0-auto-anneal-df1-global_local': dict(theta_vb=4.1e-07, zeta_vb=2.9e-09, tau_vb=1.4e-06, lam2_inv_vb=1.2e-07, mu_beta_vb=5.3e-04, gam_vb=2.6e-05, elbo=2.6e-07),
    'n1000-q40-scale-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=3.5e-06, zeta_vb=9.1e-08, tau_vb=1.7e-05, lam2_inv_vb=3.6e-07, mu_beta_vb=2.9e-03, gam_vb=1.8e-03, elbo=8.2e-07),
    'n1100-q24-ld+rare+scale-na0.0-auto-anneal-df1-global_local': dict(theta_vb=4.3e-06, zeta_vb=3.4e-09, tau_vb=6.1e-07, lam2_inv_vb=7.0e-08, mu_beta_vb=5.5e-04, gam_vb=3.3e-05, elbo=1.9e-07),
    'n1100-q24-ld+rare+scale-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=4.0e-05, zeta_vb=7.8e-07, tau_vb=1.9e-05, lam2_inv_vb=1.1e-06, mu_beta_vb=8.2e-03, gam_vb=3.7e-02, elbo=3.8e-06),
    'n1100-q24-ld-na0.0-auto-anneal-df1-global_local': dict(theta_vb=3.1e-06, zeta_vb=1.1e-08, tau_vb=5.0e-07, lam2_inv_vb=9.5e-08, mu_beta_vb=2.2e-05, gam_vb=6.2e-05, elbo=3.8e-07),
    'n1100-q24-ld-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=4.6e-06, zeta_vb=5.2e-08, tau_vb=1.3e-06, lam2_inv_vb=1.1e-07, mu_beta_vb=3.9e-05, gam_vb=3.9e-04, elbo=5.7e-07),
    'n1100-q24-rare-na0.0-auto-anneal-df1-global_local': dict(theta_vb=1.1e-06, zeta_vb=2.7e-09, tau_vb=1.1e-06, lam2_inv_vb=7.0e-08, mu_beta_vb=5.1e-06, gam_vb=1.6e-05, elbo=3.8e-07),
    'n1100-q24-rare-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=1.3e-07, zeta_vb=4.7e-09, tau_vb=9.9e-07, lam2_inv_vb=7.5e-08, mu_beta_vb=4.4e-06, gam_vb=1.1e-05, elbo=5.8e-07),
    'n1100-q24-scale-na0.0-auto-anneal-df1-global_local': dict(theta_vb=6.3e-07, zeta_vb=1.9e-09, tau_vb=4.0e-07, lam2_inv_vb=1.1e-07, mu_beta_vb=1.1e-03, gam_vb=7.3e-06, elbo=3.6e-07),
    'n1100-q24-scale-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=1.5e-04, zeta_vb=8.6e-08, tau_vb=3.2e-05, lam2_inv_vb=5.3e-07, mu_beta_vb=1.6e-03, gam_vb=3.2e-03, elbo=4.4e-06),
    'n1100-q40-ld+rare+scale-na0.06-auto-anneal-df1-global_local': dict(theta_vb=1.9e-06, zeta_vb=5.2e-09, tau_vb=6.3e-07, lam2_inv_vb=8.6e-08, mu_beta_vb=4.9e-04, gam_vb=9.7e-04, elbo=1.9e-07),
    'n1100-q40-ld+rare+scale-na0.06-per_trait-anneal-df1-global_local': dict(theta_vb=2.0e-05, zeta_vb=3.8e-07, tau_vb=2.0e-05, lam2_inv_vb=1.0e-05, mu_beta_vb=1.3e-03, gam_vb=6.2e-02, elbo=1.2e-06),
    'n300-q24-ld+rare+scale-na0.0-auto-anneal-df1-global_local': dict(theta_vb=4.7e-06, zeta_vb=2.0e-07, tau_vb=6.3e-05, lam2_inv_vb=3.7e-07, mu_beta_vb=2.1e-03, gam_vb=2.4e-03, elbo=2.0e-06),
    'n300-q24-ld+rare+scale-na0.0-per_trait-anneal-df1-global': dict(theta_vb=1.2e-07, zeta_vb=1.2e-09, tau_vb=2.4e-07, lam2_inv_vb=0.0e+00, mu_beta_vb=2.7e-06, gam_vb=5.3e-05, elbo=5.3e-07),
    'n300-q24-ld+rare+scale-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=6.0e-05, zeta_vb=1.3e-07, tau_vb=8.6e-05, lam2_inv_vb=5.4e-06, mu_beta_vb=1.6e-03, gam_vb=5.2e-03, elbo=4.2e-05),
    'n300-q24-ld+rare+scale-na0.0-per_trait-anneal-df3-global_local': dict(theta_vb=6.0e-05, zeta_vb=1.3e-07, tau_vb=8.6e-05, lam2_inv_vb=1.2e-05, mu_beta_vb=1.6e-03, gam_vb=5.2e-03, elbo=4.2e-05),
    'n300-q24-ld+rare+scale-na0.0-per_trait-noanneal-df5-global_local': dict(theta_vb=3.0e-05, zeta_vb=1.4e-07, tau_vb=1.9e-04, lam2_inv_vb=1.8e-07, mu_beta_vb=9.0e-03, gam_vb=2.3e-02, elbo=2.1e-05),
    'n300-q24-ld-na0.0-auto-anneal-df1-global_local': dict(theta_vb=1.3e-07, zeta_vb=4.2e-09, tau_vb=6.4e-07, lam2_inv_vb=7.0e-08, mu_beta_vb=2.0e-05, gam_vb=4.2e-04, elbo=5.1e-07),
    'n300-q24-ld-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=1.7e-06, zeta_vb=5.5e-08, tau_vb=1.3e-06, lam2_inv_vb=1.1e-07, mu_beta_vb=3.3e-05, gam_vb=4.5e-04, elbo=2.2e-06),
    'n300-q24-rare-na0.0-auto-anneal-df1-global_local': dict(theta_vb=2.5e-07, zeta_vb=2.4e-09, tau_vb=9.0e-07, lam2_inv_vb=7.0e-08, mu_beta_vb=3.9e-06, gam_vb=1.9e-05, elbo=1.7e-07),
    'n300-q24-rare-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=1.5e-06, zeta_vb=3.7e-09, tau_vb=5.7e-07, lam2_inv_vb=7.0e-08, mu_beta_vb=1.8e-06, gam_vb=3.0e-05, elbo=3.4e-07),
    'n300-q24-scale-na0.0-auto-anneal-df1-global_local': dict(theta_vb=1.6e-06, zeta_vb=3.0e-09, tau_vb=7.6e-07, lam2_inv_vb=7.0e-08, mu_beta_vb=2.4e-03, gam_vb=1.6e-05, elbo=2.7e-07),
    'n300-q24-scale-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=1.3e-06, zeta_vb=3.9e-08, tau_vb=1.3e-05, lam2_inv_vb=1.5e-07, mu_beta_vb=1.6e-03, gam_vb=2.7e-04, elbo=2.3e-07),
    'n300-q40-ld+rare+scale-na0.06-auto-anneal-df1-global_local': dict(theta_vb=1.4e-07, zeta_vb=7.1e-09, tau_vb=2.0e-06, lam2_inv_vb=1.0e-07, mu_beta_vb=4.3e-04, gam_vb=5.0e-05, elbo=1.1e-07),
    'n300-q40-ld+rare+scale-na0.06-per_trait-anneal-df1-global_local': dict(theta_vb=4.8e-06, zeta_vb=4.2e-07, tau_vb=6.0e-05, lam2_inv_vb=3.7e-06, mu_beta_vb=3.0e-03, gam_vb=1.4e-02, elbo=1.7e-05),
    'n300-q40-scale-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=7.7e-07, zeta_vb=4.5e-08, tau_vb=1.7e-05, lam2_inv_vb=2.6e-07, mu_beta_vb=1.1e-03, gam_vb=1.5e-03, elbo=1.4e-06),
    'n4000-q24-ld+rare+scale-na0.0-auto-anneal-df1-global_local': dict(theta_vb=9.1e-07, zeta_vb=4.7e-08, tau_vb=1.4e-06, lam2_inv_vb=2.7e-07, mu_beta_vb=6.8e-03, gam_vb=2.9e-04, elbo=6.2e-07),
    'n4000-q24-ld+rare+scale-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=1.2e-03, zeta_vb=1.9e-06, tau_vb=4.0e-05, lam2_inv_vb=2.2e-06, mu_beta_vb=5.7e-03, gam_vb=2.7e-02, elbo=4.4e-06),
    'n4000-q24-ld-na0.0-auto-anneal-df1-global_local': dict(theta_vb=1.2e-05, zeta_vb=1.5e-07, tau_vb=8.5e-07, lam2_inv_vb=6.4e-07, mu_beta_vb=6.7e-05, gam_vb=4.5e-03, elbo=1.3e-06),
    'n4000-q24-ld-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=1.9e-06, zeta_vb=1.7e-07, tau_vb=1.2e-06, lam2_inv_vb=8.3e-08, mu_beta_vb=3.8e-05, gam_vb=2.8e-04, elbo=1.1e-06),
    'n4000-q24-rare-na0.0-auto-anneal-df1-global_local': dict(theta_vb=1.9e-07, zeta_vb=2.5e-09, tau_vb=9.3e-07, lam2_inv_vb=7.0e-08, mu_beta_vb=1.4e-06, gam_vb=8.8e-06, elbo=4.3e-07),
    'n4000-q24-rare-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=5.5e-07, zeta_vb=2.3e-09, tau_vb=1.3e-06, lam2_inv_vb=7.0e-08, mu_beta_vb=1.5e-06, gam_vb=1.8e-05, elbo=2.1e-07),
    'n4000-q24-scale-na0.0-auto-anneal-df1-global_local': dict(theta_vb=6.9e-08, zeta_vb=2.0e-09, tau_vb=1.1e-06, lam2_inv_vb=8.0e-08, mu_beta_vb=5.7e-04, gam_vb=1.4e-05, elbo=1.5e-07),
    'n4000-q24-scale-na0.0-per_trait-anneal-df1-global_local': dict(theta_vb=1.8e-05, zeta_vb=1.0e-07, tau_vb=1.4e-05, lam2_inv_vb=4.8e-07, mu_beta_vb=1.5e-03, gam_vb=3.4e-03, elbo=9.8e-06),
    'n4000-q40-ld+rare+scale-na0.06-auto-anneal-df1-global_local': dict(theta_vb=3.2e-06, zeta_vb=1.6e-07, tau_vb=1.2e-06, lam2_inv_vb=1.0e-06, mu_beta_vb=4.0e-03, gam_vb=4.2e-04, elbo=5.0e-07),
    'n4000-q40-ld+rare+scale-na0.06-per_trait-anneal-df1-global_local': dict(theta_vb=2.4e-04, zeta_vb=7.8e-06, tau_vb=1.7e-04, lam2_inv_vb=3.6e-05, mu_beta_vb=6.5e-03, gam_vb=5.3e-02, elbo=4.6e-05),
}


# Runs whose reference-side deviation exceeds CAP / 10 in some field do not run here (a bar is never widened to admit a run):
# {(input, sweeps): the figure}.  Both are gam_vb between the oracle's Gram-space and n-space forms, on inputs where the posterior
# mass sits between two SNPs with r^2 = 0.99; the same inputs stay in with their other sweep counts, and the same regimes and launch
# forms run these sweep counts at the other n.  The command above lists the runs beyond CAP / 10: exactly these.
EXCLUDED_RUNS = {
    ("n1000-q40-ld+rare+scale-na0.0-per_trait-anneal-df1-global_local", ELBO): "gam_vb 7.0e-10",
    ("n1100-q40-ld+rare+scale-na0.06-per_trait-anneal-df1-global_local", WHOLE): "gam_vb 1.1e-10",
}

# Where (a) and (b) are both exactly 0 -- the ELBO after 1 and 3 sweeps exists only without annealing, in the df = 5 case, which
# has no (b) -- ten times the measurement is no bar.  The ELBO is a sum over n q residual terms and p q entries that the two sides
# add in different orders: sqrt(n q + p q) units in the last place at the largest shape of the file (n = 4000, q = 40) is the floor.
ELBO_GRAIN = float(np.sqrt(4000 * 40 + 130 * 40) * 2.0 ** -52)


def bar(sweeps, field, inputs=None):
    """The bar of a field after `sweeps`: from MEASURED_NOANNEAL for an input without a ladder, else from MEASURED."""
    table = MEASURED_NOANNEAL if inputs is not None and inputs[4] is None else MEASURED
    a, b = table[sweeps][field]
    m = 10.0 * max(a, b)
    if field == "elbo":
        m = max(m, ELBO_GRAIN)
    return min(m, CAP[field])


# ------------------------------------------------------------------------------------------------------------------------------
# The cases: plain data.  inputs = (shape, regime, na_frac, hyper, anneal, df, scheme); env = launch-plan hooks; expect = what
# aq_vb_status must report (None for a case that does not go through one VbRun handle).

P = 130                      # 9 SNP blocks, the last of 2; chained in 3 segments the borders are at columns 48 and 96
ALL = ("ld", "rare", "scale")
LADDER = (1, 2, 10)
NA = 0.06
Q_LA, Q_NA = 24, 40          # two trait tiles, the last of 8; three, the last of 8 (with AQ_TT = 2 the second group's second tile is padding)


def _inp(n=300, q=Q_LA, regime=ALL, na=0.0, hyper="per_trait", anneal=LADDER, df=1, scheme="global_local"):
    return ((n, P, q), tuple(regime), na, hyper, anneal, df, scheme)


def _exp(kernel=0, flags=0, parts=1, tt=1, chain=0, geom=None, natural=False):
    return dict(core_kernel=kernel, instance_flags=flags, split_parts=parts, tiles_per_group=tt, chain_segments=chain, geom=geom,
                natural=natural)


REGIME_SETS = (("ld",), ("rare",), ("scale",), ALL)
HYPERS = ("auto", "per_trait")
# n = 300 -> 19 sample tiles.  AQ_LA_C = 2: 10 per part -> geometry 2 / 2; AQ_LA_C = 3: 7 per part -> 2 / 1.  n = 4000 in 12 parts:
# 21 tiles per part -> NT = 4 (tests/test_gpu_link_range.py).  n = 1100 -> 69 tiles: with so few trait tiles the planner splits them
# in two parts of 6 / 6.  n = 1000 -> 63 tiles in one workgroup: 9 / 9 / 9 with two trait tiles per workgroup (AQ_TT = 2), 10 / 10 / 3
# with one and the split switched off (AQ_TT = 1, AQ_LA_NOSPLIT = 1: the form of a trait shard); with missing values the planner
# keeps n = 1000 in one MASK workgroup, 11 / 10 (tests/test_regime_coverage_host.py holds all of these against the planner).
_SPLIT_FORMS = [(f"c{C}-x{x}", {"AQ_LA_C": str(C), "AQ_LA_XHELPER": str(x)}, C, geom)
                for C, geom in ((2, (2, 2)), (3, (2, 1))) for x in (0, 1)]

CASES = {}
for _r in REGIME_SETS:
    for _h in HYPERS:
        _t = "+".join(_r) + "-" + _h
        # look-ahead kernel, complete Y
        CASES[f"la-host-{_t}"] = (_inp(regime=_r, hyper=_h), {}, _exp(natural=True))
        CASES[f"la-n1000-tt2-{_t}"] = (_inp(n=1000, q=Q_NA, regime=_r, hyper=_h), {"AQ_TT": "2"}, _exp(tt=2))
        CASES[f"la-tt1-{_t}"] = (_inp(n=1000, q=Q_NA, regime=_r, hyper=_h), {"AQ_TT": "1", "AQ_LA_NOSPLIT": "1"}, _exp(tt=1))
        CASES[f"la-chain3-{_t}"] = (_inp(regime=_r, hyper=_h), {"AQ_CHAIN": "3"}, _exp(flags=SEG, chain=3))
        for _name, _env, _C, _geom in _SPLIT_FORMS:
            CASES[f"la-{_name}-{_t}"] = (_inp(regime=_r, hyper=_h), _env, _exp(parts=_C, geom=_geom))
        CASES[f"la-n1100-{_t}"] = (_inp(n=1100, regime=_r, hyper=_h), {}, _exp(parts=2, geom=(6, 6), natural=True))
        CASES[f"la-wide-c12-{_t}"] = (_inp(n=4000, regime=_r, hyper=_h), {"AQ_LA_C": "12"}, _exp(flags=WIDE, parts=12, geom=(4, 4)))
for _h in HYPERS:
    # MASK instances: all three regimes, the carriers of three rare SNPs missing in one trait each
    CASES[f"mask-host-{_h}"] = (_inp(q=Q_NA, na=NA, hyper=_h), {}, _exp(flags=MASK, natural=True))
    CASES[f"mask-n1000-{_h}"] = (_inp(n=1000, q=Q_NA, na=NA, hyper=_h), {}, _exp(flags=MASK, natural=True))
    CASES[f"mask-n1100-{_h}"] = (_inp(n=1100, q=Q_NA, na=NA, hyper=_h), {}, _exp(flags=MASK, parts=2, geom=(6, 6), natural=True))
    CASES[f"mask-chain3-{_h}"] = (_inp(q=Q_NA, na=NA, hyper=_h), {"AQ_CHAIN": "3"}, _exp(flags=MASK | SEG, chain=3))
    CASES[f"mask-c2-{_h}"] = (_inp(q=Q_NA, na=NA, hyper=_h), {"AQ_LA_C": "2"}, _exp(flags=MASK, parts=2, geom=(2, 2)))
    CASES[f"mask-wide-c12-{_h}"] = (_inp(n=4000, q=Q_NA, na=NA, hyper=_h), {"AQ_LA_C": "12"},
                                    _exp(flags=WIDE | MASK, parts=12, geom=(4, 4)))
# the generic and the masked two-barrier kernel
CASES["generic"] = (_inp(), {"AQ_KERNEL": "2"}, _exp(kernel=2))
CASES["generic-na"] = (_inp(q=Q_NA, na=NA), {"AQ_KERNEL": "2"}, _exp(kernel=2))
CASES["masked-na"] = (_inp(q=Q_NA, na=NA), {"AQ_KERNEL": "3"}, _exp(kernel=3))
# schemes
CASES["global"] = (_inp(scheme="global"), {}, _exp(natural=True))
CASES["df3-annealed"] = (_inp(df=3), {}, _exp(natural=True))
CASES["df5"] = (_inp(df=5, anneal=None), {}, _exp(natural=True))
# the input of the shard cases below, through one handle
CASES["shards-single"] = (_inp(q=Q_NA, regime=("scale",)), {}, _exp(natural=True))

SHARD_INPUT = CASES["shards-single"][0]
SHARD_RANGES = ((0, 24), (24, 40))     # VbRun over trait shards: the second starts in the middle of a trait tile


def input_id(inputs):
    (n, p, q), regime, na, hyper, anneal, df, scheme = inputs
    return f"n{n}-q{q}-{'+'.join(regime)}-na{na}-{hyper}-{'anneal' if anneal else 'noanneal'}-df{df}-{scheme}"


def sweep_counts(name):
    iid = input_id(CASES[name][0])
    return tuple(s for s in SWEEPS if (iid, s) not in EXCLUDED_RUNS)


def maxit_of(inputs, sweeps):
    anneal = inputs[4]
    if sweeps == WHOLE:
        return WHOLE_MAXIT
    return sweeps if sweeps != ELBO else (0 if anneal is None else int(anneal[2])) + ELBO_EVALS


def c_of_last_sweep(inputs, it):
    """Inverse temperature of sweep `it` (1-based)."""
    from oracle import atlasqtl_oracle as O
    anneal = inputs[4]
    if anneal is None:
        return 1.0
    ladder = O.get_annealing_ladder_(anneal)
    return float(ladder[it - 1]) if it - 1 < len(ladder) else 1.0


def all_inputs():
    """The distinct inputs of the file with the sweep counts they run for (what the CPU-side checks and the measurement of the
    bars iterate over)."""
    out = {}
    for name, (inputs, env, expect) in CASES.items():
        out.setdefault(inputs, set()).update(sweep_counts(name))
    return {k: sorted(v, key=str) for k, v in out.items()}


_problems = {}


def problem(inputs):
    from tests.util import make_regime_problem
    (n, p, q), regime, na, hyper = inputs[:4]
    key = inputs[:4]
    if key not in _problems:
        _problems[key] = make_regime_problem(n, p, q, regime, na_frac=na, hyper=hyper)
    return _problems[key]


_oracle_runs = {}


def run_oracle(inputs, sweeps, O=None):
    """(result, ELBO trace) of the oracle's Gram-space driver; computed once per (inputs, sweeps) and shared."""
    key = (inputs, sweeps)
    if O is None and key in _oracle_runs:
        return _oracle_runs[key]
    keep = O is None
    if O is None:
        from oracle import atlasqtl_oracle as O
    shape, regime, na, hyper, anneal, df, scheme = inputs
    prob = problem(inputs)
    tr = []
    ref = O.atlasqtl_global_local_core_(prob["Y"], prob["X"], shape[2], anneal, df, 0.1, maxit_of(inputs, sweeps), prob["list_hyper"],
                                        prob["list_init"], thinned_elbo_eval=sweeps in (1, 3, WHOLE), debug=True, trace=tr,
                                        full_output=True, scheme=scheme)
    out = (ref, np.array([r["lb"] for r in tr if r["lb"] is not None]))
    if keep:
        _oracle_runs[key] = out
    return out


def trait_sd(prob):
    return np.nanstd(prob["Y"], axis=0, ddof=1)


def x_norm_sq(prob):
    """X_norm_sq(j, k) = sum over the observed rows of trait k of x_ij^2: p x q (n - 1 everywhere for complete Y)."""
    return (prob["X"] ** 2).T @ (~np.isnan(prob["Y"])).astype(np.float64)


def mu_scale(inputs, prob, ref):
    """What |mu_beta_vb - ref| is divided by: |ref| + 1e-4 sd(y_k), with |ref| replaced by max(|ref|, posterior sd) on the
    entries whose observed rows hold no carrier."""
    mu = np.abs(ref["mu_beta_vb"])
    xn = x_norm_sq(prob)
    c = c_of_last_sweep(inputs, ref["it"])
    sd_post = 1.0 / np.sqrt(c * (xn + ref["sig2_inv_vb"]) * ref["tau_vb"][None, :])
    mu = np.where(xn < NO_CARRIER, np.maximum(mu, sd_post), mu)
    return mu + MU_ATOL_OVER_RTOL * trait_sd(prob)[None, :]


def deviations(inputs, ref, lref, got, lgot):
    """Every compared field's deviation of `got` from `ref`, in the metric of its bar."""
    prob = problem(inputs)
    out = {}
    for f, floor in FLOOR.items():
        if ref.get(f) is None or got.get(f) is None:
            continue
        out[f] = float(np.max(np.abs(got[f] - ref[f]) / np.maximum(np.abs(ref[f]), floor)))
    out["mu_beta_vb"] = float(np.max(np.abs(got["mu_beta_vb"] - ref["mu_beta_vb"]) / mu_scale(inputs, prob, ref)))
    out["gam_vb"] = float(np.max(np.abs(got["gam_vb"] - ref["gam_vb"])))
    m = compared(ref["gam_vb"])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = np.abs(logit(got["gam_vb"][m]) - logit(ref["gam_vb"][m])) - logit_grain(ref["gam_vb"][m])
    out["gam_logit"] = float(np.max(np.where(np.isnan(d), np.inf, np.maximum(d, 0.0)))) if m.any() else 0.0
    if lref.size:
        out["elbo"] = float(np.max(np.abs(lgot - lref) / np.abs(lref))) if lgot.shape == lref.shape else np.inf
    return out


def residual_drift(prob, got):
    """Largest |R in the handle - mis_pat .* (Y - X beta_vb)| relative to the trait's rms."""
    Y = np.array(prob["Y"], dtype=np.float64)
    obs = ~np.isnan(Y)
    Y[~obs] = 0.0
    fresh = obs * (Y - prob["X"] @ got["beta_vb"])
    rms = np.sqrt((Y ** 2).sum(0) / np.maximum(obs.sum(0), 1))
    return float(np.max(np.abs(got["residual"] - fresh) / rms[None, :]))


def _prove_instance(run, expect, n, pinned):
    st = run.status()
    flags, parts = expect["instance_flags"], expect["split_parts"]
    assert st["core_kernel"] == expect["core_kernel"], st
    if expect["core_kernel"] != 0:
        return st
    if expect["natural"] and not pinned:     # fewer CUs than the tables assume: the planner's own choice, of the same family
        assert st["instance_flags"] & MASK == flags & MASK, st
        return st
    if parts > 1:
        _assert_instance(run, flags, parts, *expect["geom"])
    got = {k: st[k] for k in ("instance_flags", "split_parts", "tiles_per_group", "chain_segments")}
    want = {k: expect[k] for k in got}
    assert got == want, f"the handle launches {got}, the case is written for {want}"
    assert st["n_pad"] >= n
    return st


def _hold(tag, inputs, sweeps, ref, lref, got, lgot, extra=""):
    dev = deviations(inputs, ref, lref, got, lgot)
    print(f"\nREGIME case={tag} sweeps={sweeps} it={ref['it']} {extra}"
          + " ".join(f"{f}={v:.3e}({v / bar(sweeps, f, inputs):.2f})" for f, v in dev.items()))
    for f in ("theta_vb", "zeta_vb", "mu_beta_vb", "tau_vb", "lam2_inv_vb", "gam_vb"):
        assert np.all(np.isfinite(got[f])), f
    assert lgot.shape == lref.shape
    over = {f: (v, bar(sweeps, f, inputs)) for f, v in dev.items() if not v <= bar(sweeps, f, inputs)}
    assert not over, f"beyond the bar (deviation, bar): {over}"


@pytest.mark.parametrize("name,sweeps", [(name, s) for name in sorted(CASES) for s in sweep_counts(name)])
def test_regime_matches_oracle(name, sweeps, monkeypatch):
    """Every run prints its deviations and their fractions of the bars before it asserts (pytest -s)."""
    from atlasqtl_amd.core import VbRun
    from tests.test_gpu_split_instances import _pin_256_cus
    inputs, env, expect = CASES[name]
    shape, regime, na, hyper, anneal, df, scheme = inputs
    for k, v in env.items():
        monkeypatch.setenv(k, v)       # read by aq_vb_create
    pinned = _pin_256_cus(monkeypatch)
    prob = problem(inputs)
    ref, lref = run_oracle(inputs, sweeps)
    maxit = maxit_of(inputs, sweeps)
    run = VbRun(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], anneal, 0.1, maxit, sweeps in (1, 3, WHOLE), True,
                scheme=scheme, df=df)
    try:
        st = _prove_instance(run, expect, shape[0], pinned)
        run.run()
        st2 = run.status()
        got = run.result(full_output=True)
        lgot = run.elbo_trace()[1]
        if sweeps == WHOLE:
            got["residual"] = run.residual()
    finally:
        run.close()
    assert st2["it"] == ref["it"]
    if sweeps == WHOLE:
        assert bool(st2["converged"]) and ref["converged"] and ref["it"] < WHOLE_MAXIT
    else:
        assert ref["it"] == maxit
    if sweeps == ELBO:
        assert lref.size >= ELBO_EVALS
    extra = (f"kernel={st['core_kernel']} flags={st['instance_flags']} C={st['split_parts']} TT={st['tiles_per_group']} "
             f"chain={st['chain_segments']} NT={st['tiles_matrix']}/{st['tiles_matrix2']}/{st['tiles_recurrence']} n_pad={st['n_pad']} ")
    if sweeps == WHOLE:
        drift = residual_drift(prob, got)
        extra += f"residual={drift:.3e} "
    _hold(name, inputs, sweeps, ref, lref, got, lgot, extra)
    if sweeps == WHOLE:
        assert drift < RESIDUAL_BAR


# ------------------------------------------------------------------------------------------------------------------------------
# Trait shards: the q-vectors of per-trait hyper-parameters must reach the shard's traits, not the first ones of the list

@pytest.mark.parametrize("sweeps", [3, ELBO, WHOLE])
@pytest.mark.parametrize("n_parts", [2, 3])
def test_run_multi_shards_match_single_handle_and_oracle(n_parts, sweeps):
    """aq_vb_run_multi with 2 and 3 trait shards on device 0 (q = 40: 16 + 24 and 16 + 16 + 8 traits), host-staged all-reduce:
    against the oracle at the bars, and against the single-handle run as tests/test_gpu_multi.py does."""
    import atlasqtl_amd as A
    from atlasqtl_amd.core import run_multi, vb_partition
    from tests.test_gpu_multi import _same
    inputs = SHARD_INPUT
    shape, regime, na, hyper, anneal, df, scheme = inputs
    prob = problem(inputs)
    parts = vb_partition(shape[2], n_parts)
    assert len({k0 for k0, k1 in parts}) == n_parts and parts[-1][1] == shape[2]
    ref, lref = run_oracle(inputs, sweeps)
    maxit, thinned = maxit_of(inputs, sweeps), sweeps in (1, 3, WHOLE)
    got = run_multi(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], anneal, 0.1, maxit, n_gpus=n_parts,
                    devices=[0] * n_parts, transport=1, thinned_elbo_eval=thinned, debug=True)
    one = A.atlasqtl_global_local_core_(prob["Y"], prob["X"], shape[2], anneal, 1, 0.1, maxit, 0, prob["list_hyper"],
                                        prob["list_init"], full_output=True, thinned_elbo_eval=thinned, debug=True)
    assert got["it"] == ref["it"]
    _hold(f"multi-{n_parts}", inputs, sweeps, ref, lref, got, got["elbo_trace"][1])
    _same(got, one)


def _shard_worker(rank, world, port, outdir, sweeps):
    from tests.util import gloo_rank, shard_lists
    dist = gloo_rank(rank, world, port)
    from atlasqtl_amd.core import VbRun
    from tests import test_gpu_regimes as T
    inputs = T.SHARD_INPUT
    shape, regime, na, hyper, anneal, df, scheme = inputs
    prob = T.problem(inputs)
    k0, k1 = T.SHARD_RANGES[rank]
    lh, li = shard_lists(prob["list_hyper"], prob["list_init"], k0, k1)
    run = VbRun(prob["Y"][:, k0:k1], prob["X"], lh, li, anneal, 0.1, T.maxit_of(inputs, sweeps), sweeps in (1, 3, T.WHOLE), True,
                q_total=shape[2], process_group=dist.group.WORLD, trait_offset=k0)
    try:
        run.run()
        got = run.result(full_output=True)
        np.savez(f"{outdir}/rank{rank}.npz", it=run.status()["it"], lb=run.elbo_trace()[1],
                 **{f: got[f] for f in ("gam_vb", "mu_beta_vb", "beta_vb", "theta_vb", "zeta_vb", "tau_vb", "lam2_inv_vb")})
    finally:
        run.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("sweeps", [ELBO])
def test_vbrun_over_trait_shards_matches_oracle(sweeps, tmp_path):
    """Two ranks share the GPU, each a VbRun over its own traits [0, 24) and [24, 40) with the q-vectors cut by
    tests.util.shard_lists: the second shard starts at trait 24, not a multiple of 16."""
    from tests.util import spawn_ranks
    inputs = SHARD_INPUT
    assert SHARD_RANGES[1][0] % 16 != 0
    ref, lref = run_oracle(inputs, sweeps)
    spawn_ranks(_shard_worker, 2, str(tmp_path), sweeps)
    r = [np.load(tmp_path / f"rank{i}.npz") for i in range(2)]
    assert int(r[0]["it"]) == int(r[1]["it"]) == ref["it"]
    np.testing.assert_array_equal(r[0]["lb"], r[1]["lb"])
    np.testing.assert_array_equal(r[0]["theta_vb"], r[1]["theta_vb"])
    got = {f: np.concatenate([r[0][f], r[1][f]], axis=-1) for f in ("gam_vb", "mu_beta_vb", "beta_vb", "zeta_vb", "tau_vb")}
    got.update(theta_vb=r[0]["theta_vb"], lam2_inv_vb=r[0]["lam2_inv_vb"])
    _hold("vbrun-shards", inputs, sweeps, ref, lref, got, r[0]["lb"])


# ------------------------------------------------------------------------------------------------------------------------------
# Operator level: coreDualLoop / coreDualMisLoop on the Gram matrix of an ld + rare X, tau_vb spread over 1e+-8

OP_BAR = 1e-11                         # of tests/test_gpu_parity.py::test_core_dual_loop_matches_oracle


def regime_operator_inputs(mis, seed=5):
    """tests.util.operator_inputs (p = 130, q = 24) with X replaced by the standardised ld + rare matrix of make_regime_problem
    (n = 300) and everything that derives from it rebuilt; tau_vb = 10^U(-8, 8) with both ends in the first trait tile, Y and
    mu_beta_vb scaled by tau_vb^-1/2 (so that the terms of the update keep their relative sizes), and sig2_beta_vb(j, k) =
    1 / ((X_norm_sq(j, k) + sig2_inv_vb) tau_k) as the driver sets it: with the random 0.005 ... 0.02 of operator_inputs, three to six
    times that, the coordinate-wise pass overshoots between SNPs in LD and diverges (|mu| reaches 1e54 in the oracle)."""
    from tests.util import make_regime_problem, operator_inputs
    prob = make_regime_problem(300, P, Q_LA, ("ld", "rare"))
    X = prob["X"]
    n, p, q = X.shape[0], X.shape[1], Q_LA
    a = operator_inputs(p, q, n=n, seed=seed, mis=mis, c=0.8)
    rng = np.random.default_rng(seed + 1)
    tau = 10.0 ** rng.uniform(-8.0, 8.0, size=q)
    tau[2], tau[13] = 1e-8, 1e8
    s = 1.0 / np.sqrt(tau)
    Y = a["Y"] * s[None, :]
    mu = np.asfortranarray(a["mu_beta_vb"] * s[None, :])
    gam = a["gam_vb"]
    m1 = np.asfortranarray(gam * mu)
    cp_X = np.asfortranarray(X.T @ X)
    sig2_inv = float(np.exp(a["log_sig2_inv_vb"]))
    a.update(X=X, Y=Y, mu_beta_vb=mu, m1_beta=m1, tau_vb=tau, log_tau_vb=np.log(tau) - 0.01, cp_X=cp_X)
    if mis:
        mis_pat = (rng.random((n, q)) > 0.1).astype(np.float64)
        rm = [np.asfortranarray(X[mis_pat[:, k] == 0].T @ X[mis_pat[:, k] == 0]) for k in range(q)]
        bx = cp_X.T @ m1 - np.stack([rm[k].T @ m1[:, k] for k in range(q)], axis=1)
        xn = (X ** 2).T @ mis_pat
        a.update(cp_X_rm=rm, cp_Y_X=np.asfortranarray((Y * mis_pat).T @ X), cp_betaX_X=np.asfortranarray(bx),
                 sig2_beta_vb=np.asfortranarray(1.0 / ((xn + sig2_inv) * tau[None, :])))
    else:
        a.update(cp_Y_X=np.asfortranarray(Y.T @ X), cp_betaX_X=np.asfortranarray(cp_X.T @ m1),
                 sig2_beta_vb=1.0 / ((n - 1.0 + sig2_inv) * tau))
    a["col_scale"] = s
    return a


@pytest.mark.parametrize("mis", [False, True])
def test_operators_on_ld_gram_and_spread_tau_match_oracle(mis):
    """aq_core_dual_loop / aq_core_dual_mis_loop against the C restatement of src/coreLoop.cpp on these inputs, at the bar of
    tests/test_gpu_parity.py, every column in units of its trait's scale."""
    import atlasqtl_amd as A
    from oracle import atlasqtl_oracle as O
    a = regime_operator_inputs(mis)
    b = {k: ([m.copy(order="F") for m in v] if isinstance(v, list) else v.copy(order="F") if isinstance(v, np.ndarray) and v.ndim == 2
             else v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    args = lambda d: ((d["cp_X"],) + ((d["cp_X_rm"],) if mis else ()) + (d["cp_Y_X"], d["gam_vb"], d["log_Phi"], d["log_1mPhi"],    # noqa: E731
                      d["log_sig2_inv_vb"], d["log_tau_vb"], d["m1_beta"], d["cp_betaX_X"], d["mu_beta_vb"], d["sig2_beta_vb"],
                      d["tau_vb"], d["shuffled_ind"], d["sample_q"]))
    (O.core_dual_mis_loop if mis else O.core_dual_loop)(*args(a), c=0.8)
    (A.coreDualMisLoop if mis else A.coreDualLoop)(*args(b), c=0.8)
    s = a["col_scale"][None, :]
    for key in ("gam_vb", "mu_beta_vb", "m1_beta", "cp_betaX_X"):
        unit = 1.0 if key == "gam_vb" else s
        dev = float(np.max(np.abs(b[key] - a[key]) / unit / np.maximum(np.abs(a[key]) / unit, 1e-6)))
        print(f"REGIME operator mis={mis} {key}={dev:.3e}")
        assert dev < OP_BAR, key
