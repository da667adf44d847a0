"""Child process of tests/test_gpu_pcs_subspace.py: aq_prep_grm_apply at the shapes given on the command line under the
AQ_PCS_SPLITS of its environment, read when the entry runs.  Writes Z, the trace and the splits of the plan used per shape to
the .npz named first.  Usage: python -m tests.pcs_apply_child OUT.npz n,p,L [n,p,L ...]"""
import ctypes as C
import sys

import numpy as np


def main(out, shapes):
    from atlasqtl_amd import _lib
    from atlasqtl_amd import prepare as P
    from tests import pcs_util as PU
    res = {}
    for shape in shapes:
        n, p, L = (int(v) for v in shape.split(","))
        X, Q = PU.apply_case(n, p, L)
        prep = P.prepare_on_device(np.zeros((n, 1), order="F"), X)[0]
        try:
            Z, tr = prep.grm_apply(Q, return_trace=True)
            ms, pl = C.c_double(0.0), _lib.AqPcsPlan()
            _lib.check(_lib.lib().aq_prep_grm_apply_time(prep.handle, L, 1, C.byref(ms), C.byref(pl)), "aq_prep_grm_apply_time")
            res[f"Z_{shape}"], res[f"tr_{shape}"], res[f"splits_{shape}"], res[f"p1_{shape}"] = Z, tr, pl.splits, prep.p
        finally:
            prep.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
