"""Measures, on the CPU and from the reference side only, what the bars of tests/test_gpu_regimes.py are derived from.  For every
distinct input of that file, every sweep count and every compared field, in the metric of tests/test_gpu_regimes.deviations:
  (a) the oracle as it is (SciPy log_ndtr, double-precision inv_mills_ratio_) against the same oracle with these two functions
      (and the annealed update of lam2_inv_vb, compute_integral_hs_) evaluated with 40 to 60 digits: the _mp_oracle of
      tests/tools/measure_link_bars.py;
  (b) the oracle's Gram-space driver against its n-space form (oracle.sharded_oracle.run_sharded): the reordering noise that
      the GPU's n-space sweep has as well.  run_sharded states the horseshoe with df = 1: for an input with df > 1 both forms run
      the df = 1 twin -- same data, lists and ladder -- whose sweep over the p x q entries is the same code; the global scheme has
      no (b).
The inputs that run without a ladder get tables of their own (MEASURED_NOANNEAL): their first sweeps run at c = 1.
Prints every figure and, at the end, the MEASURED, MEASURED_NOANNEAL and WORST_OF_INPUT tables of the test file (over the runs the file holds) and
the runs whose own figures exceed a tenth of a cap, which the file must list as EXCLUDED_RUNS.
usage: python tests/tools/measure_regime_bars.py [processes [only]]   (only: measure the inputs whose id contains this text; the
tables then cover those inputs alone)"""
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np


def measure(item):
    warnings.simplefilter("ignore")
    from measure_link_bars import _mp_oracle
    from oracle import sharded_oracle as S
    from tests import test_gpu_regimes as T
    inputs, sweeps_list = item
    shape, regime, na, hyper, anneal, df, scheme = inputs
    M = _mp_oracle()
    prob = T.problem(inputs)
    out = []
    for sweeps in T.SWEEPS:          # the excluded runs too: the figures that exclude them are printed with the rest
        ref, lref = T.run_oracle(inputs, sweeps)
        alt, lalt = T.run_oracle(inputs, sweeps, O=M)
        a = T.deviations(inputs, ref, lref, alt, lalt)
        if alt["it"] != ref["it"]:
            a["elbo"] = np.inf
        b = {}
        if scheme == "global_local":
            twin = inputs[:5] + (1,) + inputs[6:]
            if df != 1:
                ref, lref = T.run_oracle(twin, sweeps)
            tr = []
            ns = S.run_sharded(prob["Y"], prob["X"], shape[2], anneal, 0.1, T.maxit_of(inputs, sweeps), prob["list_hyper"],
                               prob["list_init"], thinned_elbo_eval=sweeps in (1, 3, T.WHOLE), debug=True, trace=tr)
            b = T.deviations(twin, ref, lref, ns, np.array([r["lb"] for r in tr if r["lb"] is not None]))
            if ns["it"] != ref["it"]:
                b["elbo"] = np.inf
        out.append((inputs, sweeps, ref["it"], a, b))
    return out


def main(processes, only=""):
    from multiprocessing import Pool
    from tests import test_gpu_regimes as T
    items = sorted(T.all_inputs().items(), key=lambda kv: -kv[0][0][2] * (2 if kv[0][2] else 1))      # the long ones first
    items = [kv for kv in items if only in T.input_id(kv[0])]
    with Pool(processes) as pool:
        results = [r for rs in pool.imap_unordered(measure, items, chunksize=1) for r in rs]
    tables, worst, beyond = {True: {}, False: {}}, {}, {}
    input_id = T.input_id
    for inputs, sweeps, it, a, b in sorted(results, key=str):
        print(f"{input_id(inputs)} sweeps={sweeps} it={it}\n    (a) " + " ".join(f"{k}={v:.2e}" for k, v in a.items())
              + "\n    (b) " + (" ".join(f"{k}={v:.2e}" for k, v in b.items()) or "-"), flush=True)
        for k in a:
            if max(a[k], b.get(k, 0.0)) > T.CAP[k] / 10.0:
                beyond.setdefault((input_id(inputs), sweeps), {})[k] = max(a[k], b.get(k, 0.0))
        if (input_id(inputs), sweeps) in T.EXCLUDED_RUNS:
            continue
        t = tables[inputs[4] is not None].setdefault(sweeps, {})
        for k in a:
            pa, pb = t.get(k, (0.0, 0.0))
            t[k] = (max(pa, a[k]), max(pb, b.get(k, 0.0)))
            if np.isfinite(T.CAP[k]):
                w = worst.setdefault(input_id(inputs), {})
                w[k] = max(w.get(k, 0.0), max(a[k], b.get(k, 0.0)) / T.CAP[k])
    for name, table in (("MEASURED", tables[True]), ("MEASURED_NOANNEAL", tables[False])):
        print(f"\n{name} = {{")
        for sweeps in sorted(table, key=str):
            print(f"    {sweeps!r}: dict(" + ", ".join(f"{k}=({a:.1e}, {b:.1e})" for k, (a, b) in table[sweeps].items()) + "),")
        print("}")
    print("\nWORST_OF_INPUT = {")
    for name in sorted(worst):
        print(f"    {name!r}: dict(" + ", ".join(f"{k}={v:.1e}" for k, v in worst[name].items()) + "),")
    print("}")
    print("\nruns beyond cap / 10 (they may not run in the file; EXCLUDED_RUNS must list exactly these):")
    for key in sorted(beyond, key=str):
        print(f"    {key}: " + " ".join(f"{k}={v:.1e}" for k, v in beyond[key].items()))
    print("EXCLUDED_RUNS is", "right" if set(beyond) == set(T.EXCLUDED_RUNS) else f"WRONG: {sorted(T.EXCLUDED_RUNS, key=str)}")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else min(8, os.cpu_count() or 1), sys.argv[2] if len(sys.argv) > 2 else "")
