#!/usr/bin/env python3
"""Host wall-clock of aq_prepare_data_cov (covariates regressed out of X and Y on the GPU) against aq_prepare_data on the
same inputs -- the path that existed before, the yardstick -- in one process: n = 1000, p = 50 000 int8 dosages, q = 10 000
traits with 5 % NA, d = 20 covariates (AQ_BENCH_N / AQ_BENCH_P / AQ_BENCH_Q / AQ_BENCH_D say otherwise).  One warm-up call,
then three timed calls each, the clock around the C call (for the covariate call that includes the basis on the host; the
handle is destroyed outside the clock).  Prints one JSON line.  The two kernels alone are read
off a kernel trace of this tool:

    python tools/time_prepare_cov.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_prepare_cov.py      # aq_k_cov_residualise(_y) in the stats
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from atlasqtl_amd import _lib
    n, p, q, d = (int(os.environ.get(k, v)) for k, v in (("AQ_BENCH_N", 1000), ("AQ_BENCH_P", 50000), ("AQ_BENCH_Q", 10000),
                                                         ("AQ_BENCH_D", 20)))
    rng = np.random.default_rng(1)
    G = np.asfortranarray(rng.binomial(2, rng.uniform(0.05, 0.5, size=p)[None, :], size=(n, p)).astype(np.int8))
    Y = np.asfortranarray(rng.normal(size=(n, q)))
    Y[rng.random(Y.shape) < 0.05] = np.nan
    Z = np.asfortranarray(rng.normal(size=(n, d)))
    L = _lib.lib()
    pin = _lib.AqPrepInput()
    pin.n, pin.p, pin.q, pin.X, pin.X_i8, pin.Y, pin.device = n, p, q, None, G.ctypes.data_as(C.POINTER(C.c_int8)), _lib.as_dp(Y), 0
    cov = _lib.AqPrepCov()
    cov.d, cov.Z = d, _lib.as_dp(Z)

    def run_plain():
        h = C.c_void_p()
        t = time.perf_counter()
        rc = L.aq_prepare_data(C.byref(pin), C.byref(h))
        dt = time.perf_counter() - t
        _lib.check(rc, "aq_prepare_data")
        return dt, h

    def run_cov():
        h = C.c_void_p()
        t = time.perf_counter()
        rc = L.aq_prepare_data_cov(C.byref(pin), C.byref(cov), C.byref(h))
        dt = time.perf_counter() - t
        _lib.check(rc, "aq_prepare_data_cov")
        return dt, h

    def timed(fn):
        out, kept = [], None
        for it in range(4):                                      # the first call is the warm-up
            dt, h = fn()
            if it:
                out.append(round(dt, 5))
            pk = C.c_int32(0)
            _lib.check(L.aq_prep_info(h, C.byref(pk), None, None, None, None, None), "aq_prep_info")
            kept = int(pk.value)
            L.aq_prep_destroy(h)
        return out, kept

    t_plain, kept_plain = timed(run_plain)
    t_cov, kept_cov = timed(run_cov)
    print(json.dumps(dict(n=n, p=p, q=q, d=d, p_kept=kept_plain, p_kept_cov=kept_cov, prepare_data_s=t_plain, prepare_data_cov_s=t_cov,
                          extra_bytes_x=2 * 8 * n * p)))


if __name__ == "__main__":
    main()
