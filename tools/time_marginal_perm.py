#!/usr/bin/env python3
"""Times aq_prep_marginal_perm, the permutation nulls of the marginal screen (csrc/aq_msperm_kernels.h, the tile loop in csrc/aq_screen_tile.h), at bench.py's shape
(n = 1000, p = 50 000, q = 10 000) on random int8 dosages and Gaussian traits: complete Y, and Y with 5 % of its values missing.
Per case and per instance of the tile kernel (complete: tile 128 with PB 1 and tile 64 with PB 1, 2, 4; masked: PB 1, 2;
forced through AQ_MSCREEN_TILE and AQ_MSPERM_PB) the kernels of one full batch of permutations -- gather, tile, reduce -- per
permutation (aq_prep_marginal_perm_time), `--repeats` times, beside the plain screen's kernels on the same handle in the same
process (aq_prep_marginal_time), as often.  The expectation to hold them against: one permutation, gather included, costs no
more than one plain screen, within the spread of the plain screen's own repeats.  Prints one JSON line per case and instance
(DESIGN.md section 9, N1).

    python tools/time_marginal_perm.py [--repeats 3] [--shape 1000x50000x10000]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.time_marginal import make_y  # noqa: E402

INSTANCES = {0: [(128, 1), (64, 1), (64, 2), (64, 4)], 1: [(64, 1), (64, 2)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shape", default="1000x50000x10000")
    args = ap.parse_args()
    from atlasqtl_amd import _lib
    from atlasqtl_amd.prepare import prepare_on_device
    L = _lib.lib()
    n, p, q = (int(v) for v in args.shape.split("x"))
    G = np.asfortranarray(np.random.default_rng(n + p).integers(0, 3, size=(n, p), dtype=np.int8))
    for missing in (0.0, 0.05):
        prep = prepare_on_device(make_y(n, q, missing, 7), G)[0]
        ms, plan = C.c_double(0.0), _lib.AqMscreenPlan()
        plain, got, plans = [], {}, {}
        for _ in range(args.repeats):                                  # the plain screen and every instance in turn, repeatedly
            for name in ("AQ_MSCREEN_TILE", "AQ_MSPERM_PB", "AQ_MSPERM_BATCH"):
                os.environ.pop(name, None)
            _lib.check(L.aq_prep_marginal_time(prep.handle, 10, C.byref(ms), C.byref(plan)), "aq_prep_marginal_time")
            plain.append(round(ms.value, 3))
            for tile, pb in INSTANCES[int(plan.masked)]:
                if not plan.masked:
                    os.environ["AQ_MSCREEN_TILE"] = str(tile)
                os.environ["AQ_MSPERM_PB"] = str(pb)
                pp = _lib.AqMspermPlan()
                n_perm = max(pb, ((1 << 30) // (8 * q * n)) // pb * pb)    # one full batch of this PB: Yp within 1 GiB
                _lib.check(L.aq_prep_marginal_perm_time(prep.handle, n_perm, 2, C.byref(ms), C.byref(pp)), "aq_prep_marginal_perm_time")
                assert (pp.tile, pp.pb, pp.launches, pp.batch) == (tile, pb, 1, n_perm), (pp.tile, pp.pb, pp.launches, pp.batch)
                got.setdefault((tile, pb), []).append(round(ms.value, 3))
                plans[(tile, pb)] = pp
        print(json.dumps(dict(what="aq_prep_marginal", n=n, p1=prep.p, q=q, missing=missing, masked=plan.masked, tile=plan.tile,
                              kernels_ms=plain)), flush=True)
        for (tile, pb), pp in plans.items():
            print(json.dumps(dict(what="aq_prep_marginal_perm", missing=missing, masked=pp.masked, tile=pp.tile, pb=pp.pb, batch=pp.batch,
                                  lds_bytes=pp.lds_bytes, yp_mb=round(pp.yp_bytes / 1e6, 1), ms_per_permutation=got[(tile, pb)],
                                  ratio_to_plain=round(min(got[(tile, pb)]) / min(plain), 3))), flush=True)
        prep.close()


if __name__ == "__main__":
    main()
