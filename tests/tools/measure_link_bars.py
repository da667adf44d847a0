"""Measures, on the CPU and from the reference side only, what the bars of tests/test_gpu_link_range.py are derived from.  For every
distinct input of that file, every sweep count and every compared field, in the metric of tests/test_gpu_link_range.deviations:
  (a) the oracle as it is (SciPy log_ndtr, double-precision inv_mills_ratio_) against the same oracle with these two functions
      replaced by 40-digit mpmath evaluations rounded to double: what the link's own rounding is worth in the state (the annealed
      update of lam2_inv_vb is taken at 60 digits as well: for df = 1 it is a quotient near 1 less 1 and loses about L_vb ulp, 6e-11
      at L_vb = 590; for df = 3 a quotient of differences of Kummer functions that loses e^L_vb ulp -- the larger part of the
      reference's own error in the annealed cases; and for df = 5, 7 compute_integral_hs_, a difference of large terms,
      is evaluated at 60 digits from the same text);
  (b) the oracle's Gram-space driver against its n-space form (oracle.sharded_oracle.run_sharded, which states the horseshoe
      with df = 1: the other inputs have no (b)): the reordering noise that the GPU's n-space sweep has as well.
Prints every figure and, at the end, the MEASURED table of the test file: the maxima over the inputs.
usage: python tests/tools/measure_link_bars.py [processes]"""
import importlib.util
import inspect
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np


def _mp_oracle():
    """A second instance of oracle/atlasqtl_oracle.py whose log_ndtr and inv_mills_ratio_ are evaluated with 40 digits."""
    import mpmath as mp
    from scipy import special as sp
    mp.mp.dps = 40
    spec = importlib.util.spec_from_file_location("atlasqtl_oracle_mp", os.path.join(ROOT, "oracle", "atlasqtl_oracle.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    half_log_2pi = mp.log(2 * mp.pi) / 2

    def log_ndtr_1(x):
        x = mp.mpf(float(x))
        return float(mp.log(mp.ncdf(x)) if x < 0 else mp.log1p(-mp.ncdf(-x)))

    def mills_1(U):      # phi(U) / Phi(U)
        U = mp.mpf(float(U))
        return float(mp.exp(-U * U / 2 - half_log_2pi) / mp.ncdf(U))

    v_log_ndtr = np.frompyfunc(log_ndtr_1, 1, 1)
    v_mills = np.frompyfunc(mills_1, 1, 1)

    class Special:
        def __getattr__(self, name):
            return getattr(sp, name)

        @staticmethod
        def log_ndtr(x):
            return v_log_ndtr(np.asarray(x, dtype=np.float64)).astype(np.float64)

    def inv_mills_ratio_(y, U, log_1_pnorm_U, log_pnorm_U):      # R/utils.R:172-191 with the quotient taken at 40 digits
        U = np.asarray(U, dtype=np.float64)
        if y == 1:
            m = v_mills(U).astype(np.float64)
            return np.where(m < -U, -U, m)
        m = -v_mills(-U).astype(np.float64)
        return np.where(m > -U, -U, m)

    def update_annealed_lam2_inv_vb_(L_vb, c, df=1, plain=M.update_annealed_lam2_inv_vb_):
        """The annealed update of lam2_inv_vb at 60 digits: the reference's own error in double.  df > 1: the quotient of Kummer
        functions of R/update_vb.R:76-81 loses about e^L_vb ulp to cancellation."""
        if df == 1:     # R/update_vb.R:70-75: Gamma(2 - c, L) / (Gamma(1 - c, L) L) - 1, a quotient near 1 less 1: about L_vb ulp are lost
            def one1(L):
                with mp.workdps(60):
                    L, cc = mp.mpf(float(L)), mp.mpf(float(c))
                    return float(mp.gammainc(2 - cc, L) / (mp.gammainc(1 - cc, L) * L) - 1)
            return np.array([one1(L) for L in np.asarray(L_vb, dtype=np.float64)])
        g, K = mp.gamma, mp.hyp1f1

        def one(L):
            with mp.workdps(60):
                L, cc = mp.mpf(float(L)), mp.mpf(float(c))
                num = (g(cc * (df - 1) / 2 + 2) * g(cc) * K(cc * (df - 1) / 2 + 2, 3 - cc, L) / (cc - 1) / (cc - 2) / g(cc * (df + 1) / 2)
                       + g(2 - cc) * L ** (cc - 2) * K(cc * (df + 1) / 2, cc - 1, L))
                den = (g(cc * (df - 1) / 2 + 1) * g(cc) * K(cc * (df - 1) / 2 + 1, 2 - cc, L) / (cc - 1) / g(cc * (df + 1) / 2)
                       + g(1 - cc) * L ** (cc - 1) * K(cc * (df + 1) / 2, cc, L))
                return float(num / den / df)
        return np.array([one(L) for L in np.asarray(L_vb, dtype=np.float64)])

    # df = 5, 7: compute_integral_hs_ (R/utils.R:425-568) is a difference of exp(log_sum_exp(.)) of large terms; the same text
    # evaluated at 60 digits shows what that cancellation costs the reference in double
    class MpNumpy:
        log, exp = staticmethod(mp.log), staticmethod(mp.exp)

    def log_sum_exp_mp(x):
        top = max(x)
        return mp.log(mp.fsum(mp.exp(v - top) for v in x)) + top

    ns = dict(np=MpNumpy, log_sum_exp_=log_sum_exp_mp, _lfactorial=lambda k: mp.loggamma(k + 1))
    exec(inspect.getsource(M.compute_integral_hs_), ns)

    def compute_integral_hs_(alpha, beta, m, n, Q_ab):
        with mp.workdps(60):
            return float(ns["compute_integral_hs_"](mp.mpf(float(alpha)), mp.mpf(float(beta)), m, n, mp.mpf(float(Q_ab))))

    M.compute_integral_hs_ = compute_integral_hs_
    M.update_annealed_lam2_inv_vb_ = update_annealed_lam2_inv_vb_
    M.sp = Special()
    M.inv_mills_ratio_ = inv_mills_ratio_
    return M


def measure(item):
    warnings.simplefilter("ignore")
    from oracle import sharded_oracle as S
    from tests import test_gpu_link_range as T
    inputs, sweeps_list = item
    shape, na, axis, anneal, df, scheme, fine_scale = inputs
    M = _mp_oracle()
    prob = T.problem(inputs)
    out = []
    for sweeps in sweeps_list:
        ref, lref = T.run_oracle(inputs, sweeps)
        alt, lalt = T.run_oracle(inputs, sweeps, O=M)
        a = T.deviations(ref, lref, alt, lalt)
        b = {}
        if df == 1 and scheme == "global_local":
            tr = []
            ns = S.run_sharded(prob["Y"], prob["X"], shape[2], anneal, 0.1, T.maxit_of(inputs, sweeps), prob["list_hyper"],
                               prob["list_init"], thinned_elbo_eval=sweeps != T.ELBO, debug=T.debug_of(inputs), trace=tr)
            b = T.deviations(ref, lref, ns, np.array([r["lb"] for r in tr if r["lb"] is not None]))
        out.append((inputs, sweeps, a, b))
    return out


def main(processes):
    from multiprocessing import Pool
    from tests import test_gpu_link_range as T
    items = list(T.all_inputs().items())
    with Pool(processes) as pool:
        results = [r for rs in pool.imap_unordered(measure, items) for r in rs]
    table = {}
    for inputs, sweeps, a, b in sorted(results, key=str):
        print(f"{inputs} sweeps={sweeps}\n    (a) " + " ".join(f"{k}={v:.2e}" for k, v in a.items())
              + "\n    (b) " + (" ".join(f"{k}={v:.2e}" for k, v in b.items()) or "-"), flush=True)
        t = table.setdefault(sweeps, {})
        for k in a:
            pa, pb = t.get(k, (0.0, 0.0))
            t[k] = (max(pa, a[k]), max(pb, b.get(k, 0.0)))
    print("\nMEASURED = {")
    for sweeps in sorted(table, key=str):
        print(f"    {sweeps!r}: dict(" + ", ".join(f"{k}=({a:.1e}, {b:.1e})" for k, (a, b) in table[sweeps].items()) + "),")
    print("}")
    print("\nbars = min(10 max(a, b), cap):")
    for sweeps in sorted(table, key=str):
        print(f"    {sweeps!r}: " + " ".join(f"{k}={min(10 * max(a, b), T.CAP[k]):.1e}" for k, (a, b) in table[sweeps].items()))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else min(8, os.cpu_count() or 1))
