#!/usr/bin/env python3
"""Times the conditional cis scan (aq_prep_cis_cond_time: csrc/aq_ciscond_kernels.h, the tile loop in csrc/aq_screen_tile.h) on the inputs of tools/time_cis.py,
n = 1000, p = 50 000, q = 10 000, random int8 dosages and complete Gaussian traits, windows reaching `--half` predictors to
either side of the trait (about 600 predictors with the default 300).  On one handle and in one process, `--repeats` times:
the plain scan (aq_prep_cis_time: max k = 0), then the conditional scan with every trait conditioned on k = 1, 2 and 4
variants of its own window, and with a mixed load (a quarter of the traits each with 0, 1, 2 and 4).  Per figure the basis
kernel's milliseconds, the scan's, and the scan's ratio to the plain scan's, beside 1 + KC, the ratio of the matrix
instructions.  Prints one JSON line per figure.

    python tools/time_cis_cond.py [--repeats 3] [--shape 1000x50000x10000] [--half 300]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.time_marginal import make_y  # noqa: E402


def lists(rng, lo, hi, k):
    """(cond_ptr, cond_idx): trait t conditions on k[t] distinct variants of its own window (fewer where it is narrower)."""
    ptr, idx = [0], []
    for t in range(lo.size):
        w = int(hi[t] - lo[t])
        kt = min(int(k[t]), w)
        idx += [int(lo[t] + v) for v in rng.permutation(w)[:kt]]
        ptr.append(len(idx))
    return np.asarray(ptr, dtype=np.int32), np.asarray(idx + [0], dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shape", default="1000x50000x10000")
    ap.add_argument("--half", type=int, default=300)
    args = ap.parse_args()
    from atlasqtl_amd import _lib
    from atlasqtl_amd.cis import cis_windows
    from atlasqtl_amd.prepare import prepare_on_device
    L = _lib.lib()
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
    lo, hi = cis_windows(chrom, pos, tchrom, tpos, None, 1000 * args.half)
    plo, phi = _lib.as_ip(lo), _lib.as_ip(hi)
    loads = [("k1", np.full(q, 1)), ("k2", np.full(q, 2)), ("k4", np.full(q, 4)), ("mixed", np.array([0, 1, 2, 4])[np.arange(q) % 4])]
    loads = [(name, lists(rng, lo, hi, k)) for name, k in loads]
    ms, ms2 = C.c_double(0.0), C.c_double(0.0)
    for _ in range(args.repeats):
        cp = _lib.AqCisPlan()
        _lib.check(L.aq_prep_cis_time(prep.handle, plo, phi, 0, 10, C.byref(ms), C.byref(ms2), C.byref(cp)), "aq_prep_cis_time")
        plain = ms.value
        print(json.dumps(dict(what="aq_prep_cis", mean_window=round(float(np.mean(hi - lo)), 1), work_items=cp.n_items,
                              fill=round(cp.window_pairs / cp.staged_pairs, 4), ms_scan=round(plain, 3))), flush=True)
        for name, (ptr, idx) in loads:
            pl = _lib.AqCiscondPlan()
            _lib.check(L.aq_prep_cis_cond_time(prep.handle, plo, phi, _lib.as_ip(ptr), _lib.as_ip(idx), 10, C.byref(ms), C.byref(ms2),
                                               C.byref(pl)), "aq_prep_cis_cond_time")
            print(json.dumps(dict(what="aq_prep_cis_cond", lists=name, kc=pl.kc, streams=pl.streams, lds_bytes=pl.lds_bytes,
                                  work_items=pl.cis.n_items, panels_mb=round(1e-6 * (pl.qo_bytes + pl.yo_bytes), 1),
                                  ms_basis=round(ms.value, 3), ms_scan=round(ms2.value, 3), scan_over_plain=round(ms2.value / plain, 3))),
                  flush=True)
    prep.close()


if __name__ == "__main__":
    main()
