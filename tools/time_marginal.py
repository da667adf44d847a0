#!/usr/bin/env python3
"""Times aq_prep_marginal, the marginal screen of a prepared handle (csrc/aq_mscreen_kernels.h, the tile loop in csrc/aq_screen_tile.h), at bench.py's shape
(n = 1000, p = 50 000, q = 10 000) on random int8 dosages and Gaussian traits: complete Y, and Y with 5 % of its values missing.
Per case: all kernels of one screen alone (aq_prep_marginal_time: events around `--reps` launches after a warm-up, counting
only), and the whole entry as marginal_screen() calls it, with its allocations and copies (wall clock, one warm-up).  TFLOP/s
count 2 n p1 q flop for complete Y and 6 n p1 q for masked Y (three products from the same operand reads), against the 78.6
TFLOP/s of the f64 matrix pipe; the flop of whole tiles that the kernel issues are given beside them.  The number to hold them
against is the rate of aq_prep_grm_time on the same machine (the same MFMA, a similar LDS pattern): --grm times it on the same
handle.  Prints one JSON line per case.

    python tools/time_marginal.py [--reps 5] [--grm] [--shape 1000x50000x10000]
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


def make_y(n, q, missing, seed):
    rng = np.random.default_rng(seed)
    Y = np.empty((n, q), order="F")
    for k0 in range(0, q, 512):
        k1 = min(q, k0 + 512)
        blk = rng.standard_normal((n, k1 - k0))
        if missing > 0:
            blk[rng.random(blk.shape) < missing] = np.nan
        Y[:, k0:k1] = blk
    return Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grm", action="store_true")
    ap.add_argument("--shape", default="1000x50000x10000")
    args = ap.parse_args()
    from atlasqtl_amd import _lib
    from atlasqtl_amd import marginal as M
    from atlasqtl_amd.prepare import prepare_on_device
    L = _lib.lib()
    n, p, q = (int(v) for v in args.shape.split("x"))
    G = np.asfortranarray(np.random.default_rng(n + p).integers(0, 3, size=(n, p), dtype=np.int8))
    for missing in (0.0, 0.05):
        prep = prepare_on_device(make_y(n, q, missing, 7), G)[0]
        p1 = prep.p
        ms, plan = C.c_double(0.0), _lib.AqMscreenPlan()
        _lib.check(L.aq_prep_marginal_time(prep.handle, args.reps, C.byref(ms), C.byref(plan)), "aq_prep_marginal_time")
        df = np.sum(~np.isnan(prep.Y), axis=0) - 2
        cut = M.r2_cutoff(0.05 / (p1 * q), df)
        out = prep.marginal(cut, M.INITIAL_CAP)                 # warm-up of the whole entry
        wall = []
        for _ in range(3):
            t = time.perf_counter()
            out = prep.marginal(cut, M.INITIAL_CAP)
            wall.append(round(time.perf_counter() - t, 5))
        streams = 3 if plan.masked else 1
        useful = 2.0 * streams * n * p1 * q
        issued = 2.0 * streams * n * plan.n_tiles * plan.tile * plan.tile
        res = dict(what="aq_prep_marginal", n=n, p=p, p1=p1, q=q, missing=missing, masked=plan.masked, tile=plan.tile,
                   tiles_p=plan.tiles_p, tiles_q=plan.tiles_q, n_tiles=plan.n_tiles, lds_bytes=plan.lds_bytes,
                   scratch_mb=round(plan.scratch_bytes / 1e6, 1), reps=args.reps, kernels_ms=round(ms.value, 4),
                   tflops=round(useful / (ms.value * 1e-3) / 1e12, 2),
                   fraction_of_peak=round(useful / (ms.value * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
                   issued_tflops=round(issued / (ms.value * 1e-3) / 1e12, 2), whole_entry_s=wall, n_pairs=out["n_pairs"],
                   n_undefined=out["n_undefined"])
        print(json.dumps(res), flush=True)
        if args.grm and missing == 0.0:
            gms, gplan = C.c_double(0.0), _lib.AqGrmPlan()
            _lib.check(L.aq_prep_grm_time(prep.handle, args.reps, C.byref(gms), C.byref(gplan)), "aq_prep_grm_time")
            g_issued = 2.0 * gplan.n_tiles * gplan.tile * gplan.tile * p1
            print(json.dumps(dict(what="aq_prep_grm", n=n, p1=p1, tile=gplan.tile, n_tiles=gplan.n_tiles, splits=gplan.splits,
                                  kernels_ms=round(gms.value, 4), useful_tflops=round(float(n) * n * p1 / (gms.value * 1e-3) / 1e12, 2),
                                  issued_tflops=round(g_issued / (gms.value * 1e-3) / 1e12, 2))), flush=True)
        prep.close()


if __name__ == "__main__":
    main()
