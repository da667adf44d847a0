#!/usr/bin/env python3
"""Times the cis scan (aq_prep_cis_time: csrc/aq_cis_kernels.h, the tile loop in csrc/aq_screen_tile.h) on the inputs of tools/time_marginal.py, n = 1000,
p = 50 000, q = 10 000, random int8 dosages and Gaussian traits, complete Y and Y with 5 % of its values missing.  The
predictors sit evenly on 22 "chromosomes", 1000 base pairs apart, and the traits at random positions; the windows reach
`--half` predictors to either side of the trait, cut at the ends of its chromosome (a chromosome holds p / 22 predictors, so
the wider setting is mostly the whole chromosome).  Per case and window width: the plan's fill, the milliseconds of one scan
(the ordered copy of Y, the column sums, the tile kernel, the reduction of the bests) and of one permutation for every PB
instance (AQ_CIS_PB), `--repeats` times; beside them, in the same process and on the same handle, the plain screen forced to
AQ_MSCREEN_TILE=64 (aq_prep_marginal_time) and aq_prep_marginal_perm_time at tile 64 with the same PB.  The yardstick is the
existing kernels' time per staged 64 x 64 tile, never the new code's own: us_per_tile = 1000 ms / tiles, for the plain grid
ceil(p / 64) ceil(q / 64) tiles and for the band W work items.  What a call pays whatever the width of the band -- the ordered
copy of Y (per scan) or the gather of the permuted panels (per permutation), the column sums over all p predictors, the
reduction, the launches -- is measured on its own, by the same entry with every window cut to its first predictor: the rows
"fixed".  Their W0 work items are the fewest the trait tiles allow (the first predictors of a tile's 64 traits still span a
few items), so us_per_tile_net = 1000 (ms - ms of the fixed row) / (W - W0) is the time of the work items that the width of
the windows adds.  Prints one JSON line per figure.

    python tools/time_cis.py [--repeats 3] [--shape 1000x50000x10000] [--half 250,2500]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.time_marginal import make_y  # noqa: E402

PBS = {0: (1, 2, 4), 1: (1, 2)}
HOOKS = ("AQ_MSCREEN_TILE", "AQ_MSPERM_PB", "AQ_MSPERM_BATCH", "AQ_CIS_PB", "AQ_CIS_BATCH")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shape", default="1000x50000x10000")
    ap.add_argument("--half", default="250,2500")
    args = ap.parse_args()
    from atlasqtl_amd import _lib
    from atlasqtl_amd.cis import cis_windows
    from atlasqtl_amd.prepare import prepare_on_device
    L = _lib.lib()
    n, p, q = (int(v) for v in args.shape.split("x"))
    G = np.asfortranarray(np.random.default_rng(n + p).integers(0, 3, size=(n, p), dtype=np.int8))
    rng = np.random.default_rng(11)
    for missing in (0.0, 0.05):
        prep = prepare_on_device(make_y(n, q, missing, 7), G)[0]
        p1 = prep.p
        chrom = np.arange(p1) * 22 // p1
        first = np.searchsorted(chrom, np.arange(23))
        pos = 1000 * (np.arange(p1) - first[chrom])
        tchrom = rng.integers(0, 22, q)
        tpos = (rng.random(q) * 1000 * (first[tchrom + 1] - first[tchrom])).astype(np.int64)
        ms, ms2 = C.c_double(0.0), C.c_double(0.0)
        masked = None
        for _ in range(args.repeats):
            for name in HOOKS:
                os.environ.pop(name, None)
            os.environ["AQ_MSCREEN_TILE"] = "64"
            plan = _lib.AqMscreenPlan()
            _lib.check(L.aq_prep_marginal_time(prep.handle, 10, C.byref(ms), C.byref(plan)), "aq_prep_marginal_time")
            masked = int(plan.masked)
            print(json.dumps(dict(what="aq_prep_marginal", missing=missing, masked=masked, tile=plan.tile, tiles=plan.n_tiles,
                                  ms=round(ms.value, 3), us_per_tile=round(1000 * ms.value / plan.n_tiles, 4))), flush=True)
            for pb in PBS[masked]:
                os.environ["AQ_MSPERM_PB"] = str(pb)
                pp = _lib.AqMspermPlan()
                n_perm = max(pb, ((1 << 30) // (8 * q * n)) // pb * pb)
                _lib.check(L.aq_prep_marginal_perm_time(prep.handle, n_perm, 2, C.byref(ms), C.byref(pp)), "aq_prep_marginal_perm_time")
                tiles = pp.tiles_p * pp.tiles_q
                print(json.dumps(dict(what="aq_prep_marginal_perm", missing=missing, masked=masked, tile=pp.tile, pb=pp.pb, batch=pp.batch,
                                      tiles=tiles, ms_per_permutation=round(ms.value, 3),
                                      us_per_tile=round(1000 * ms.value / tiles, 4))), flush=True)
            os.environ.pop("AQ_MSPERM_PB", None)
            fixed = {}
            for half in [0] + [int(v) for v in args.half.split(",")]:
                lo, hi = cis_windows(chrom, pos, tchrom, tpos, None, 1000 * max(half, 1))
                if half == 0:                                              # every window cut to its first predictor: the fixed costs
                    hi = np.minimum(hi, lo + 1).astype(np.int32)
                plo, phi = _lib.as_ip(lo), _lib.as_ip(hi)
                cp = _lib.AqCisPlan()
                _lib.check(L.aq_prep_cis_time(prep.handle, plo, phi, 0, 10, C.byref(ms), C.byref(ms2), C.byref(cp)), "aq_prep_cis_time")
                W = cp.n_items
                print(json.dumps(dict(what="aq_prep_cis", missing=missing, masked=masked, half=half,
                                      mean_window=round(float(np.mean(hi - lo)), 1), work_items=W, trait_tiles=cp.trait_tiles,
                                      fill=round(cp.window_pairs / cp.staged_pairs, 4),
                                      share_of_plain_grid=round(W / (-(-p1 // 64) * -(-q // 64)), 4),
                                      ordered_copy_mb=round(8e-6 * cp.q_active * n, 1), ms_scan=round(ms.value, 3),
                                      **({"fixed": True} if half == 0 else
                                         {"us_per_tile": round(1000 * ms.value / W, 4),
                                          "us_per_tile_net": round(1000 * (ms.value - fixed["scan"]) / (W - fixed["W"]), 4)}))),
                      flush=True)
                if half == 0:
                    fixed["scan"], fixed["W"] = ms.value, W
                for pb in PBS[masked]:
                    os.environ["AQ_CIS_PB"] = str(pb)
                    n_perm = max(pb, ((1 << 30) // (8 * q * n)) // pb * pb)
                    _lib.check(L.aq_prep_cis_time(prep.handle, plo, phi, n_perm, 2, C.byref(ms), C.byref(ms2), C.byref(cp)),
                               "aq_prep_cis_time")
                    print(json.dumps(dict(what="aq_prep_cis_perm", missing=missing, masked=masked, half=half, pb=cp.pb, batch=cp.batch,
                                          launches=cp.launches, lds_bytes=cp.perm_lds_bytes, work_items=W,
                                          ms_per_permutation=round(ms2.value, 3),
                                          **({"fixed": True} if half == 0 else
                                             {"us_per_tile": round(1000 * ms2.value / W, 4),
                                              "us_per_tile_net": round(1000 * (ms2.value - fixed[pb]) / (W - fixed["W"]), 4)}))),
                          flush=True)
                    if half == 0:
                        fixed[pb] = ms2.value
                os.environ.pop("AQ_CIS_PB", None)
        prep.close()


if __name__ == "__main__":
    main()
