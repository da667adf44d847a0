"""Randomised parity sweep: random small shapes (ragged n, p, q; with and without missing values; with and without
annealing) through the HIP path against the oracle.  usage: python tests/tools/fuzz_parity.py [ncases] [seed]
(AQ_FUZZ_NMAX / AQ_FUZZ_PMAX / AQ_FUZZ_QMAX widen the shape ranges, e.g. AQ_FUZZ_NMAX=1300 crosses the sample-split boundary;
AQ_FUZZ_LINK=1, or run(..., link_spread=True): every case also replaces the init's zeta_vb by a uniform draw in +-Z, Z in 0 ... 40,
and theta_vb by one in +-T, so that the probit link leaves the few table intervals the automatic init stays in.  T is drawn in
0 ... 40 without annealing; with annealing in 0 ... min(1, sqrt(1000 / (sig02_inv_vb q))), which keeps L_vb of the reference's
annealed update of lam2_inv_vb below 250 -- it returns NaN from about 745 on.  The gam_vb error is then reported on the logit
scale as well: tests/test_gpu_link_range.py says why and how.
AQ_FUZZ_REGIME=ld+rare+scale[:per_trait], or run(..., regime=("ld", "rare", "scale"), hyper="per_trait"): the cases are drawn
from tests/util.make_regime_problem instead of make_problem -- neighbouring SNPs in LD, rare variants, traits scaled by
10^U(-4, 4), optionally per-trait hyper-parameters; p is then at least 96, q at least 18 with a last trait tile of two, n at least
100, and mu_beta_vb is compared in the scale-following metric of tests/test_gpu_regimes.py.  Off by default: the cases of a
given seed are unchanged without it.)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import atlasqtl_amd as A
from oracle import atlasqtl_oracle as O
from tests.util import make_problem, make_regime_problem


def run(ncases=30, seed=2024, link_spread=None, regime=None, hyper="auto"):
    """Returns the worst errors; raises AssertionError on the first mismatch."""
    if link_spread is None:
        link_spread = os.environ.get("AQ_FUZZ_LINK", "0") not in ("", "0")
    if regime is None and os.environ.get("AQ_FUZZ_REGIME"):
        spec = os.environ["AQ_FUZZ_REGIME"].split(":")
        regime, hyper = tuple(spec[0].split("+")), (spec[1] if len(spec) > 1 else "auto")
    rng = np.random.default_rng(seed)
    worst = dict(elbo=0.0, mu=0.0, gam=0.0)
    if link_spread:
        worst["gam_logit"] = 0.0
    t0 = time.time()
    for c in range(ncases):
        n = int(rng.integers(20, int(os.environ.get("AQ_FUZZ_NMAX", 400))))
        p = int(rng.integers(12, int(os.environ.get("AQ_FUZZ_PMAX", 160))))
        q = int(rng.integers(1, int(os.environ.get("AQ_FUZZ_QMAX", 70))))
        na = float(rng.choice([0.0, 0.0, 0.05, 0.2]))
        anneal = [None, (1, 2, 10), (2, 3, 5), (3, 2, 4)][int(rng.integers(0, 4))]
        data_seed, init_seed = int(rng.integers(1, 10**6)), int(rng.integers(1, 10**6))
        if regime:       # (after the case's draws, which stay what they are without the knob)
            n, p = max(n, 100), max(p, 96)
            q = max(q, 18) + (2 if max(q, 18) % 16 in (0, 1) else 0)
            prob = make_regime_problem(n, p, q, regime, na_frac=na, hyper=hyper, seed=data_seed, init_seed=init_seed)
        else:
            prob = make_problem(n, p, q, p_act=max(1, min(8, p // 3)), prob_assoc=0.4, na_frac=na, seed=data_seed,
                                init_seed=init_seed, p0=(2, 6))
        spread = ""
        if link_spread:      # (drawn after everything else of the case, so that the knob leaves the cases' shapes and data as they are)
            li = dict(prob["list_init"])
            z_max = float(rng.uniform(0.0, 40.0))
            t_cap = 40.0 if anneal is None else min(1.0, float(np.sqrt(1000.0 / (float(li["sig02_inv_vb"]) * q))))
            t_max = float(rng.uniform(0.0, t_cap))
            li["zeta_vb"] = rng.uniform(-z_max, z_max, size=q)
            li["theta_vb"] = rng.uniform(-t_max, t_max, size=prob["p"])
            prob["list_init"] = li
            spread = f" zeta+-{z_max:.1f} theta+-{t_max:.2f}"
        tr = []
        args_ref = (prob["Y"], prob["X"], q, anneal, 1, 0.1, 300, prob["list_hyper"], prob["list_init"])
        args_hip = (prob["Y"], prob["X"], q, anneal, 1, 0.1, 300, 0, prob["list_hyper"], prob["list_init"])
        ref_exc = got_exc = ref = got = None
        try:
            ref = O.atlasqtl_global_local_core_(*args_ref, trace=tr, full_output=True, debug=True)
        except Exception as e:   # e.g. a non-monotone ELBO on a degenerate draw: both sides must then fail the same way
            ref_exc = e
        try:
            got = A.atlasqtl_global_local_core_(*args_hip, full_output=True, debug=True)
        except Exception as e:
            got_exc = e
        if ref_exc is not None or got_exc is not None:
            both = ref_exc is not None and got_exc is not None
            same = both and ("monotonically" in str(ref_exc)) == ("monotonically" in str(got_exc))
            assert same, f"case {c}: one-sided or different failure: oracle {ref_exc!r}, HIP {got_exc!r}"
            print(f"case {c}: n={n} p={prob['p']} q={q} na={na} anneal={anneal}: both raise ({got_exc})", flush=True)
            continue
        lref = np.array([r["lb"] for r in tr if r["lb"] is not None])
        e_elbo = float(np.max(np.abs(got["elbo_trace"][1] - lref) / np.abs(lref))) if lref.size else 0.0
        if regime:
            from tests.test_gpu_regimes import MU_ATOL_OVER_RTOL, NO_CARRIER, x_norm_sq
            xn, scale = x_norm_sq(prob), np.abs(ref["mu_beta_vb"])
            sd_post = 1.0 / np.sqrt((xn + ref["sig2_inv_vb"]) * ref["tau_vb"][None, :])
            scale = np.where(xn < NO_CARRIER, np.maximum(scale, sd_post), scale) + MU_ATOL_OVER_RTOL * np.nanstd(prob["Y"], axis=0, ddof=1)
            e_mu = float(np.max(np.abs(got["mu_beta_vb"] - ref["mu_beta_vb"]) / scale))
        else:
            e_mu = float(np.max(np.abs(got["mu_beta_vb"] - ref["mu_beta_vb"]) / np.maximum(np.abs(ref["mu_beta_vb"]), 1e-8)))
        e_g = float(np.max(np.abs(got["gam_vb"] - ref["gam_vb"])))
        ok = got["it"] == ref["it"] and e_elbo < 1e-8 and e_mu < 1e-6 and e_g < 1e-8
        worst.update(elbo=max(worst["elbo"], e_elbo), mu=max(worst["mu"], e_mu), gam=max(worst["gam"], e_g))
        if link_spread:
            from tests.test_gpu_link_range import compared, logit, logit_grain
            m = compared(ref["gam_vb"])
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                d = np.abs(logit(got["gam_vb"][m]) - logit(ref["gam_vb"][m])) - logit_grain(ref["gam_vb"][m])
            e_l = float(np.max(np.where(np.isnan(d), np.inf, np.maximum(d, 0.0)))) if m.any() else 0.0
            worst["gam_logit"] = max(worst["gam_logit"], e_l)
            spread += f" gam_logit {e_l:.1e}"
        print(f"case {c}: n={n} p={prob['p']} q={q} na={na} anneal={anneal}{spread} kernel={got['core_kernel']} it={got['it']}/{ref['it']} "
              f"elbo {e_elbo:.1e} mu {e_mu:.1e} gam {e_g:.1e} {'ok' if ok else 'MISMATCH'}", flush=True)
        assert ok, f"case {c} mismatch"
    print(f"{ncases} cases ok in {time.time() - t0:.0f} s; worst: {worst}")
    return worst


if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 30, int(sys.argv[2]) if len(sys.argv) > 2 else 2024)
