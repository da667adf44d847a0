"""Child process of tests/test_gpu_ytrans.py: aq_rank_int at the shapes given on the command line under the AQ_YT_PATH of its
environment, read when the entry runs.  Writes the transformed columns, the counts and the path of the plan per shape to the
.npz named first.  Usage: python -m tests.yt_path_child OUT.npz n,q [n,q ...]"""
import ctypes as C
import sys

import numpy as np


def main(out, shapes):
    import atlasqtl_amd as A
    from atlasqtl_amd import _lib
    from tests import yt_util as YU
    res = {}
    for shape in shapes:
        n, q = (int(v) for v in shape.split(","))
        got = A.rank_normalize(YU.columns(n, q))
        pl = _lib.AqYtransPlan()
        _lib.check(_lib.lib().aq_ytrans_plan_query(n, q, 1 << 30, C.byref(pl)), "aq_ytrans_plan_query")
        res[f"Y_{shape}"], res[f"n_obs_{shape}"], res[f"n_tied_{shape}"], res[f"path_{shape}"] = got["Y"], got["n_obs"], got["n_tied"], pl.path
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
