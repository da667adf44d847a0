#!/usr/bin/env python3
"""Times aq_vb_predict's kernels, Yhat = Xt (gam_vb * mu_beta_vb) for n_new rows read in place from a handle
(csrc/aq_predict_kernels.h), through aq_vb_predict_time: the pre-pass and the two kernels, events around `--reps` launches
after one warm-up, without the copies from and to the host.  The handle is a fit on `--n-fit` samples whose p x q initial
values are drawn on the device and which runs no sweep: the product does not care what the values are.  Reports the
milliseconds per call, the 2 n_new p q flop over them against the 78.6 TFLOP/s of the f64 matrix pipe, and -- as a yardstick,
not a gate -- torch.matmul in fp64 on the same shapes on the same card.  Prints one JSON line per shape.

    python tools/time_predict.py [--reps 3] [--n-fit 64] [--shapes 1000x50000x10000] [--no-torch]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFLOPS = 78.6


def torch_matmul_ms(n_new, p, q, reps):
    import torch
    a = torch.randn(n_new, p, dtype=torch.float64, device="cuda")
    b = torch.randn(p, q, dtype=torch.float64, device="cuda")
    torch.matmul(a, b)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        torch.matmul(a, b)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n-fit", type=int, default=64)
    ap.add_argument("--shapes", default="1000x50000x10000")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from atlasqtl_amd import _lib
    from atlasqtl_amd import hyper_init as H
    from atlasqtl_amd.core import VbRun
    lib = _lib.lib()
    for shape in args.shapes.split(","):
        n_new, p, q = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(p + q)
        X = np.asfortranarray(rng.normal(size=(args.n_fit, p)))
        Y = np.asfortranarray(rng.normal(size=(args.n_fit, q)))
        rm = np.zeros(p, dtype=bool)
        p0 = (min(5, max(1, p // 8)), 25 if p >= 40 else 2)
        lh = H.prepare_list_hyper_(None, Y, p, p0, rm)
        li = H.prepare_list_init_(None, Y, p, p0, rm, q, 1, device_init=True)
        run = VbRun(Y, X, lh, li, None, 0.1, 1, True, True)
        try:
            ms, plan = C.c_double(0.0), _lib.AqPredictPlan()
            _lib.check(lib.aq_vb_predict_time(run.h, n_new, args.reps, C.byref(ms), C.byref(plan)), "aq_vb_predict_time")
        finally:
            run.close()
        flop = 2.0 * n_new * p * q
        res = dict(n_new=n_new, p=p, q=q, reps=args.reps, **{k: getattr(plan, k) for k, _ in _lib.AqPredictPlan._fields_},
                   ms_per_call=round(ms.value, 4), tflops=round(flop / (ms.value * 1e-3) / 1e12, 2),
                   fraction_of_mfma_peak=round(flop / (ms.value * 1e-3) / 1e12 / PEAK_TFLOPS, 3))
        if not args.no_torch:
            t_ms = torch_matmul_ms(n_new, p, q, args.reps)
            res.update(torch_matmul_ms=round(t_ms, 4), torch_matmul_tflops=round(flop / (t_ms * 1e-3) / 1e12, 2))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
