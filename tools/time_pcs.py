#!/usr/bin/env python3
"""Times aq_prep_grm_apply, one application Z = Xs (Xs' Q) / p1 of the relationship operator to a block of L vectors
(csrc/aq_pcs_kernels.h), and the subspace iteration built on it, on random int8 dosages.  Per shape: the kernels of one
application alone (aq_prep_grm_apply_time: events around `--reps` launches after a warm-up) against the two roofs -- the
4 n p1 lp flop they issue over the 78.6 TFLOP/s of the f64 matrix pipe, and the 16 n p1 bytes of the two reads of Xs over the
HBM rate --, then a whole subspace_pcs_ for k components with the time split into the kernels (calls x the time above), the
rest of the entry (allocation and the copies of Q and Z: wall clock of the calls minus the kernels) and the host (the n x L QR,
the L x L eigh and the products around them).  Prints one JSON line per shape (DESIGN.md sections 5 and 8;
profiles/pcs_timing.json).

    python tools/time_pcs.py [--reps 5] [--k 10] [--oversample 16] [--shapes 10240x20000,50000x20000]
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
HBM_GBPS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--oversample", type=int, default=16)
    ap.add_argument("--shapes", default="10240x20000,50000x20000")
    args = ap.parse_args()
    from atlasqtl_amd import _lib
    from atlasqtl_amd.prepare import prepare_on_device, subspace_pcs_
    lib = _lib.lib()
    L = args.k + args.oversample
    for shape in args.shapes.split(","):
        n, p = (int(v) for v in shape.split("x"))
        G = np.asfortranarray(np.random.default_rng(n + p).integers(0, 3, size=(n, p), dtype=np.int8))
        t = time.perf_counter()
        prep = prepare_on_device(np.zeros((n, 1), order="F"), G)[0]
        prepare_s = time.perf_counter() - t
        del G
        p1 = prep.p
        ms, plan = C.c_double(0.0), _lib.AqPcsPlan()
        _lib.check(lib.aq_prep_grm_apply_time(prep.handle, L, args.reps, C.byref(ms), C.byref(plan)), "aq_prep_grm_apply_time")
        flop = 4.0 * n * p1 * plan.lp
        xs_bytes = 16.0 * n * p1
        calls = []

        def apply(Q):
            t0 = time.perf_counter()
            Z = prep.grm_apply(Q)
            calls.append(time.perf_counter() - t0)
            return Z

        t = time.perf_counter()
        out = subspace_pcs_(apply, n, args.k, args.oversample, 1e-8, 300, 0)
        total_s = time.perf_counter() - t
        prep.close()
        kernels_s = len(calls) * ms.value * 1e-3
        res = dict(n=n, p=p, p1=p1, k=args.k, L=L, lp=plan.lp, n_panels=plan.n_panels, n_tiles=plan.n_tiles, splits=plan.splits,
                   chunks_per_split=plan.chunks_per_split, t_mb=round(plan.t_bytes / 1e6, 1), scratch_mb=round(plan.scratch_bytes / 1e6, 1),
                   reps=args.reps, apply_kernels_ms=round(ms.value, 4), tflops=round(flop / (ms.value * 1e-3) / 1e12, 2),
                   fraction_of_mfma_peak=round(flop / (ms.value * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
                   xs_gbps=round(xs_bytes / (ms.value * 1e-3) / 1e9, 1), fraction_of_hbm_peak=round(xs_bytes / (ms.value * 1e-3) / 1e9 / HBM_GBPS, 3),
                   prepare_s=round(prepare_s, 3), iterations=out["iterations"], converged=out["converged"],
                   residual_max=float(np.max(out["residuals"])), subspace_total_s=round(total_s, 3), device_kernels_s=round(kernels_s, 3),
                   transfer_and_alloc_s=round(sum(calls) - kernels_s, 3), host_qr_eigh_s=round(total_s - sum(calls), 3),
                   numpy_threads=os.environ.get("OMP_NUM_THREADS"))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
