#!/usr/bin/env python3
"""Host wall-clock of aq_vb_select_pairs against the nearest dense-path equivalent, aq_vb_hotspot_sizes, on one handle of
bench.py's shape (n = 1000, p = 50 000, q = 10 000 unless AQ_BENCH_N/P/Q say otherwise; device-generated initial values,
a few sweeps).  One warm-up call, then three timed calls each; prints one JSON line.

    python tools/time_select_pairs.py [--sweeps 3]
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
    from atlasqtl_amd.core import VbRun
    from bench import build_problem
    n, p, q = (int(os.environ.get(k, d)) for k, d in (("AQ_BENCH_N", 1000), ("AQ_BENCH_P", 50000), ("AQ_BENCH_Q", 10000)))
    X, Y, lh, li = build_problem(n, p, q, 0, q, 0)
    run = VbRun(Y, X, lh, li, (1, 2, 10), tol=1e-12, maxit=args.sweeps + 5, thinned_elbo_eval=True, debug=False, q_total=q)
    del li
    torch.cuda.empty_cache()
    run.run_sweeps(args.sweeps)
    L = _lib.lib()
    cap = 1 << 22
    snp, trait = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    ppi, beta, fdr = np.zeros(cap), np.zeros(cap), np.zeros(cap)
    rs = np.zeros(p, dtype=np.int64)
    cnt, tot = C.c_int64(0), C.c_int64(0)

    def select(thres, mode):
        _lib.check(L.aq_vb_select_pairs(run.h, thres, mode, cap, _lib.as_ip(snp), _lib.as_ip(trait), _lib.as_dp(ppi),
                                        _lib.as_dp(beta), _lib.as_dp(fdr), C.byref(cnt)), "aq_vb_select_pairs")

    def sizes(thres, mode):
        _lib.check(L.aq_vb_hotspot_sizes(run.h, thres, mode, rs.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(tot)),
                   "aq_vb_hotspot_sizes")

    def timed(fn, *a):
        fn(*a)                                  # warm-up
        out = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn(*a)
            out.append(round(time.perf_counter() - t, 4))
        return out

    res = dict(n=n, p=p, q=q, sweeps=run.status()["it"])
    for name, thres, mode in (("ppi_0.5", 0.5, 0), ("fdr_0.05", 0.05, 1)):
        t_sel, t_hs = timed(select, thres, mode), timed(sizes, thres, mode)
        assert cnt.value == tot.value, (cnt.value, tot.value)
        m = min(cnt.value, cap)
        assert np.array_equal(np.bincount(snp[:m], minlength=p), rs) or cnt.value > cap
        res[name] = dict(select_pairs_s=t_sel, hotspot_sizes_s=t_hs, n_pairs=int(cnt.value))
    run.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
