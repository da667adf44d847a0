#!/usr/bin/env python3
"""Times one IBSS iteration of the cis fine-mapping (aq_prep_cis_finemap_time: csrc/aq_finemap_kernels.h) on the inputs of
tools/time_cis.py, n = 1000, p = 50 000, q = 10 000, random int8 dosages and complete Gaussian traits, windows reaching
`--half` predictors to either side of the trait, cut at the ends of its chromosome (250 and 2500: about 470 and 2270 predictors
a window).  On one handle and in one process, `--repeats` times per width: the plain scan (aq_prep_cis_time), then the four
kernels of one iteration with L effects, all traits active: ms_xtr, ms_ser, ms_fit (L launches each) and ms_iter_end.  Beside
them ms_xtr / (L ms_scan), what the dense store and the missing epilogue make of the tile loop the two share; ms_fit / ms_xtr,
how far the banded product is from the loop it mirrors; and the TFLOP/s of the two matrix kernels, 2 n 64 64 flop per staged
work item and effect.  Prints one JSON line per figure.

    python tools/time_cis_finemap.py [--repeats 3] [--shape 1000x50000x10000] [--half 250,2500] [--L 10]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.time_marginal import make_y  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shape", default="1000x50000x10000")
    ap.add_argument("--half", default="250,2500")
    ap.add_argument("--L", type=int, default=10)
    args = ap.parse_args()
    from atlasqtl_amd import _lib
    from atlasqtl_amd.cis import cis_windows
    from atlasqtl_amd.prepare import prepare_on_device
    lib = _lib.lib()
    n, p, q = (int(v) for v in args.shape.split("x"))
    G = np.asfortranarray(np.random.default_rng(n + p).integers(0, 3, size=(n, p), dtype=np.int8))
    rng = np.random.default_rng(11)
    prep = prepare_on_device(make_y(n, q, 0.0, 7), G)[0]
    p1 = prep.p
    chrom = np.arange(p1) * 22 // p1
    first = np.searchsorted(chrom, np.arange(23))
    pos = 1000 * (np.arange(p1) - first[chrom])
    tchrom = rng.integers(0, 22, q)
    tpos = (rng.random(q) * 1000 * (first[tchrom + 1] - first[tchrom])).astype(np.int64)
    for half in (int(v) for v in args.half.split(",")):
        lo, hi = cis_windows(chrom, pos, tchrom, tpos, None, 1000 * half)
        plo, phi = _lib.as_ip(lo), _lib.as_ip(hi)
        seen = {}
        for _ in range(args.repeats):
            ms, ms2 = C.c_double(0.0), C.c_double(0.0)
            cp = _lib.AqCisPlan()
            _lib.check(lib.aq_prep_cis_time(prep.handle, plo, phi, 0, 10, C.byref(ms), C.byref(ms2), C.byref(cp)), "aq_prep_cis_time")
            t = [C.c_double(0.0) for _ in range(4)]
            pl = _lib.AqFinemapPlan()
            _lib.check(lib.aq_prep_cis_finemap_time(prep.handle, plo, phi, args.L, 5, *[C.byref(v) for v in t], C.byref(pl)),
                       "aq_prep_cis_finemap_time")
            xtr, ser, fit, end = (v.value for v in t)
            flop = 2.0 * n * 64 * 64 * pl.cis.n_items * args.L
            fig = dict(ms_scan=ms.value, ms_xtr=xtr, ms_ser=ser, ms_fit=fit, ms_iter_end=end, ms_iteration=xtr + ser + fit + end,
                       xtr_over_scan=xtr / (args.L * ms.value), fit_over_xtr=fit / xtr, tflops_xtr=flop / xtr * 1e-9,
                       tflops_fit=flop / fit * 1e-9)
            for k, v in fig.items():
                seen.setdefault(k, []).append(v)
            print(json.dumps(dict(what="aq_prep_cis_finemap", half=half, mean_window=round(float(np.mean(hi - lo)), 1), L=args.L,
                                  work_items=pl.cis.n_items, batch_tiles=pl.batch_tiles, n_batches=pl.n_batches,
                                  state_gib=round(pl.state_bytes / 2 ** 30, 3), **{k: round(v, 3) for k, v in fig.items()})), flush=True)
        print(json.dumps(dict(what="median", half=half, repeats=args.repeats,
                              **{k: round(float(np.median(v)), 3) for k, v in seen.items()})), flush=True)
    prep.close()


if __name__ == "__main__":
    main()
