#!/usr/bin/env python3
"""Times aq_prep_grm, the genetic relationship matrix K = Xs Xs' / p1 of a prepared handle (csrc/aq_grm_kernels.h), at
bench.py's sample and predictor counts (n = 1000, p = 50 000) and at the largest n it serves (n = 10 240, p = 20 000), on
random int8 dosages.  Per shape: the two kernels alone (aq_prep_grm_time: events around `--reps` launches after a warm-up),
the whole entry with the copy of K to the host (wall clock, one warm-up), and numpy's Xs @ Xs.T on the host copy of the same
matrix with the BLAS threads the environment gives (OMP_NUM_THREADS; 16 where this was recorded).  TFLOP/s are the useful
n^2 p1 flop of one triangle over the kernel time, against the 78.6 TFLOP/s of the f64 matrix pipe; the flop the kernel
issues (whole tiles, the diagonal tiles in full) are given beside them.  --eigh also times numpy.linalg.eigh of K, the
host part of genotype_pcs().  Prints one JSON line per shape (profiles/grm_timing.json).

    python tools/time_grm.py [--reps 5] [--eigh] [--shapes 1000x50000,10240x20000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--eigh", action="store_true")
    ap.add_argument("--shapes", default="1000x50000,10240x20000")
    args = ap.parse_args()
    from atlasqtl_amd import _lib
    from atlasqtl_amd.prepare import prepare_on_device
    L = _lib.lib()
    for shape in args.shapes.split(","):
        n, p = (int(v) for v in shape.split("x"))
        G = np.asfortranarray(np.random.default_rng(n + p).integers(0, 3, size=(n, p), dtype=np.int8))
        prep = prepare_on_device(np.zeros((n, 1), order="F"), G)[0]
        del G
        p1 = prep.p
        ms, plan = C.c_double(0.0), _lib.AqGrmPlan()
        _lib.check(L.aq_prep_grm_time(prep.handle, args.reps, C.byref(ms), C.byref(plan)), "aq_prep_grm_time")
        K = prep.grm()                                          # warm-up of the whole entry
        wall = []
        for _ in range(3):
            t = time.perf_counter()
            K = prep.grm()
            wall.append(round(time.perf_counter() - t, 5))
        Xs = prep.X_host()
        prep.close()
        t = time.perf_counter()
        Kh = (Xs @ Xs.T) / p1
        numpy_s = time.perf_counter() - t
        useful = float(n) * n * p1
        issued = 2.0 * plan.n_tiles * plan.tile * plan.tile * p1
        res = dict(n=n, p=p, p1=p1, tile=plan.tile, n_tiles=plan.n_tiles, splits=plan.splits, chunks_per_split=plan.chunks_per_split,
                   scratch_mb=round(plan.scratch_bytes / 1e6, 1), k_mb=round(plan.k_bytes / 1e6, 1), reps=args.reps,
                   kernels_ms=round(ms.value, 4), useful_tflops=round(useful / (ms.value * 1e-3) / 1e12, 2),
                   fraction_of_peak=round(useful / (ms.value * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
                   issued_tflops=round(issued / (ms.value * 1e-3) / 1e12, 2), with_copy_out_s=wall,
                   numpy_threads=os.environ.get("OMP_NUM_THREADS"), numpy_s=round(numpy_s, 3),
                   max_abs_diff_to_numpy=float(np.max(np.abs(K - Kh))))
        del Xs, Kh
        if args.eigh:
            t = time.perf_counter()
            np.linalg.eigh(K)
            res["host_eigh_s"] = round(time.perf_counter() - t, 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
