#!/usr/bin/env python3
"""Times the interaction cis scan (aq_prep_cis_int_time: csrc/aq_cisint_kernels.h, aq_ms_tile_loop_x2 in csrc/aq_screen_tile.h) on the
inputs of tools/time_cis.py, n = 1000, p = 50 000, q = 10 000, random int8 dosages and complete Gaussian traits, windows
reaching `--half` predictors to either side of the trait (about 600 predictors with the default 300), with `--covariates` d
Gaussian covariates (default 0) and a binary and a continuous interaction variable.  On one handle and in one process,
`--repeats` times: the plain scan (aq_prep_cis_time), then the interaction scan for each e.  Per figure ms_stats (the
per-predictor kernel and the trait residuals), ms_scan (the tile kernel and the reduction of the bests) and the scan's ratio
to the plain scan's, beside 2, the ratio of the matrix instructions; the median over the repeats is printed last.  Prints one
JSON line per figure.

    python tools/time_cis_int.py [--repeats 5] [--shape 1000x50000x10000] [--half 300] [--covariates 0]
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", default="1000x50000x10000")
    ap.add_argument("--half", type=int, default=300)
    ap.add_argument("--covariates", type=int, default=0)
    args = ap.parse_args()
    from atlasqtl_amd import _lib
    from atlasqtl_amd.cis import cis_windows
    from atlasqtl_amd.cis_interaction import interaction_basis
    from atlasqtl_amd.prepare import prepare_on_device
    L = _lib.lib()
    n, p, q = (int(v) for v in args.shape.split("x"))
    d = args.covariates
    G = np.asfortranarray(np.random.default_rng(n + p).integers(0, 3, size=(n, p), dtype=np.int8))
    rng = np.random.default_rng(11)
    Z = np.asfortranarray(np.random.default_rng(13).standard_normal((n, d))) if d else None
    prep = prepare_on_device(make_y(n, q, 0.0, 7), G, covariates=Z)[0]
    p1 = prep.p
    chrom = np.arange(p1) * 22 // p1
    first = np.searchsorted(chrom, np.arange(23))
    pos = 1000 * (np.arange(p1) - first[chrom])
    tchrom = rng.integers(0, 22, q)
    tpos = (rng.random(q) * 1000 * (first[tchrom + 1] - first[tchrom])).astype(np.int64)
    lo, hi = cis_windows(chrom, pos, tchrom, tpos, None, 1000 * args.half)
    plo, phi = _lib.as_ip(lo), _lib.as_ip(hi)
    erng = np.random.default_rng(17)
    es = [("binary", (erng.random(n) < 0.5).astype(np.float64)), ("continuous", erng.standard_normal(n))]
    bases = [(name, interaction_basis(e, Z, n, d)) for name, e in es]
    ms, ms2 = C.c_double(0.0), C.c_double(0.0)
    seen = {}
    for _ in range(args.repeats):
        cp = _lib.AqCisPlan()
        _lib.check(L.aq_prep_cis_time(prep.handle, plo, phi, 0, 10, C.byref(ms), C.byref(ms2), C.byref(cp)), "aq_prep_cis_time")
        plain = ms.value
        seen.setdefault("plain ms_scan", []).append(plain)
        print(json.dumps(dict(what="aq_prep_cis", mean_window=round(float(np.mean(hi - lo)), 1), work_items=cp.n_items,
                              fill=round(cp.window_pairs / cp.staged_pairs, 4), ms_scan=round(plain, 3))), flush=True)
        for name, (B, m) in bases:
            pl = _lib.AqCisintPlan()
            _lib.check(L.aq_prep_cis_int_time(prep.handle, plo, phi, _lib.as_dp(B), B.shape[0], _lib.as_dp(m), 10, C.byref(ms), C.byref(ms2),
                                              C.byref(pl)), "aq_prep_cis_int_time")
            seen.setdefault(f"{name} ms_stats", []).append(ms.value)
            seen.setdefault(f"{name} ms_scan", []).append(ms2.value)
            seen.setdefault(f"{name} scan_over_plain", []).append(ms2.value / plain)
            print(json.dumps(dict(what="aq_prep_cis_int", e=name, n_basis=pl.n_basis, streams=pl.streams, lds_bytes=pl.lds_bytes,
                                  work_items=pl.cis.n_items, ms_stats=round(ms.value, 3), ms_scan=round(ms2.value, 3),
                                  scan_over_plain=round(ms2.value / plain, 3))), flush=True)
    print(json.dumps(dict(what="median", repeats=args.repeats, **{k: round(float(np.median(v)), 3) for k, v in seen.items()},
                          **{k + " min_max": [round(float(min(v)), 3), round(float(max(v)), 3)] for k, v in seen.items()})), flush=True)
    prep.close()


if __name__ == "__main__":
    main()
