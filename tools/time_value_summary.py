#!/usr/bin/env python3
"""Host wall-clock of aq_vb_order_stats (the radix select behind summary()'s quartiles) for gam_vb and for beta_vb, and, in
the same process for comparison, of aq_vb_select_pairs in FDR mode at 0.05 -- the existing full sort of the same keys --
on one handle of bench.py's shape (n = 1000, p = 50 000, q = 10 000 unless AQ_BENCH_N/P/Q say otherwise; device-generated
initial values, a few sweeps).  One warm-up call, then three timed calls each; also one aq_vb_moments call and one
aq_vb_radix_hist pass per digit with the prefixes of the eight quartile ranks, timed singly, to set a pass against the
bytes it reads.  Prints one JSON line.

    python tools/time_value_summary.py [--sweeps 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=3)
    args = ap.parse_args()
    import torch
    from atlasqtl_amd import _lib
    from atlasqtl_amd.core import VbRun, quantile_ranks_, radix_select_
    from bench import build_problem
    n, p, q = (int(os.environ.get(k, d)) for k, d in (("AQ_BENCH_N", 1000), ("AQ_BENCH_P", 50000), ("AQ_BENCH_Q", 10000)))
    X, Y, lh, li = build_problem(n, p, q, 0, q, 0)
    run = VbRun(Y, X, lh, li, (1, 2, 10), tol=1e-12, maxit=args.sweeps + 5, thinned_elbo_eval=True, debug=False, q_total=q)
    del li
    torch.cuda.empty_cache()
    run.run_sweeps(args.sweeps)
    L = _lib.lib()
    i64p = C.POINTER(C.c_int64)
    ranks = np.asarray(quantile_ranks_(p * q), dtype=np.int64)
    out, mom = np.zeros(ranks.size), _lib.AqMoments()
    cap = 1 << 22
    snp, trait = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    ppi, beta, fdr = np.zeros(cap), np.zeros(cap), np.zeros(cap)
    cnt = C.c_int64(0)

    def order_stats(which):
        _lib.check(L.aq_vb_order_stats(run.h, which, ranks.size, ranks.ctypes.data_as(i64p), _lib.as_dp(out), C.byref(mom)),
                   "aq_vb_order_stats")

    def select_fdr():
        _lib.check(L.aq_vb_select_pairs(run.h, 0.05, 1, cap, _lib.as_ip(snp), _lib.as_ip(trait), _lib.as_dp(ppi),
                                        _lib.as_dp(beta), _lib.as_dp(fdr), C.byref(cnt)), "aq_vb_select_pairs")

    def clock(fn, *a):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn(*a)
        return round(time.perf_counter() - t, 5)

    def timed(fn, *a):
        fn(*a)                                  # warm-up
        return [clock(fn, *a) for _ in range(3)]

    tiles = (q + 15) // 16
    p_pad = (p + 15) // 16 * 16
    res = dict(n=n, p=p, q=q, sweeps=run.status()["it"], bits=_lib.AQ_RSEL_BITS, passes=64 // _lib.AQ_RSEL_BITS,
               storage_gb=round(tiles * p_pad * 16 * 8 / 1e9, 3))
    for which, name in ((0, "gam_vb"), (1, "beta_vb")):
        t = timed(order_stats, which)
        per_pass = []

        def hist_fn(prefixes, shift):
            pre = np.asarray(prefixes, dtype=np.uint64)
            hist = np.zeros((pre.size, 1 << _lib.AQ_RSEL_BITS), dtype=np.int64)
            per_pass.append((pre.size, clock(lambda: _lib.check(
                L.aq_vb_radix_hist(run.h, which, pre.size, pre.ctypes.data_as(C.POINTER(C.c_uint64)), int(shift),
                                   hist.ctypes.data_as(i64p)), "aq_vb_radix_hist"))))
            return hist
        vals = radix_select_(hist_fn, ranks.tolist())
        assert vals == out.tolist(), (vals, out)
        res[name] = dict(order_stats_s=t, moments_s=clock(lambda: _lib.check(L.aq_vb_moments(run.h, which, C.byref(mom)), "aq_vb_moments")),
                         pass_prefixes_s=per_pass, count=int(mom.count), min=mom.min, max=mom.max, mean=mom.sum / mom.count,
                         order_stats=out.tolist())
    res["select_pairs_fdr_0.05_s"] = timed(select_fdr)
    res["n_pairs_fdr_0.05"] = int(cnt.value)
    run.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
