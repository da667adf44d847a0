#!/usr/bin/env python3
"""Host wall-clock of aq_prep_ld_prune (LD pruning of the prepared matrix: band Gram on the f64 matrix pipe, bit rows, greedy
scan, tag r^2, gather) next to aq_prepare_data alone on the same input, in one process, at the X of bench.py's shape
(n = 1000, p = 50 000 unless AQ_BENCH_N/P say otherwise; window = 500 unless AQ_LD_WINDOW; r2 = 0.8; q = 8 traits).
Genotypes are haplotype copies: on each of two haplotypes a SNP copies its predecessor with every sample flipped with a
per-SNP probability between 0.002 and 0.45, so that r^2 between neighbours spreads over (0, 1).  One warm-up call, then three
timed calls each, the clock around the C call (the prune synchronises: it copies its results back); every prune runs on a
fresh handle made outside the clock.  Prints one JSON line; the band kernel's share and rate are read off a kernel trace:

    python tools/time_ld_prune.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_ld_prune.py      # aq_k_ld_band, aq_k_ld_scan in the stats
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def haplotype_copies(n, p, rng):
    rho = np.exp(rng.uniform(np.log(0.002), np.log(0.45), size=p))
    G = np.zeros((n, p), dtype=np.int8, order="F")
    for _ in range(2):
        h = rng.random(n) < 0.3
        for j in range(p):
            if j:
                h = h ^ (rng.random(n) < rho[j])
            G[:, j] += h
    return G


def main():
    from atlasqtl_amd import _lib
    n, p, window = (int(os.environ.get(k, d)) for k, d in (("AQ_BENCH_N", 1000), ("AQ_BENCH_P", 50000), ("AQ_LD_WINDOW", 500)))
    q, r2 = 8, 0.8
    rng = np.random.default_rng(1)
    G = haplotype_copies(n, p, rng)
    Y = np.asfortranarray(rng.normal(size=(n, q)))
    L = _lib.lib()

    def prepare():
        pin = _lib.AqPrepInput()
        pin.n, pin.p, pin.q, pin.X, pin.X_i8, pin.Y, pin.device = n, p, q, None, G.ctypes.data_as(C.POINTER(C.c_int8)), _lib.as_dp(Y), 0
        h = C.c_void_p()
        t = time.perf_counter()
        rc = L.aq_prepare_data(C.byref(pin), C.byref(h))
        dt = time.perf_counter() - t
        _lib.check(rc, "aq_prepare_data")
        return dt, h

    def kept(h):
        pk = C.c_int32(0)
        _lib.check(L.aq_prep_info(h, C.byref(pk), None, None, None, None, None), "aq_prep_info")
        return int(pk.value)

    t_prep, t_prune, p1, p2 = [], [], None, None
    for it in range(4):                                          # the first round is the warm-up
        dt_prep, h = prepare()
        p1 = kept(h)
        ld = _lib.AqPrepLd()
        ld.window, ld.r2, ld.group, ld.pos, ld.window_bp = window, r2, None, None, 0
        t = time.perf_counter()
        rc = L.aq_prep_ld_prune(h, C.byref(ld))
        dt_prune = time.perf_counter() - t
        _lib.check(rc, "aq_prep_ld_prune")
        p2 = kept(h)
        L.aq_prep_destroy(h)
        if it:
            t_prep.append(round(dt_prep, 5))
            t_prune.append(round(dt_prune, 5))
    flop = 2.0 * n * p1 * window
    print(json.dumps(dict(n=n, p=p, q=q, window=window, r2=r2, p_before=p1, p_after=p2, prepare_data_int8_s=t_prep,
                          ld_prune_s=t_prune, band_flop=flop, band_flop_issued=flop * 1.25 * (64 * ((window + 63) // 64)) / window,
                          whole_prune_tflops=[round(flop / t / 1e12, 3) for t in t_prune])))


if __name__ == "__main__":
    main()
