"""Child process of tests/test_gpu_finemap.py: PreparedData.cis_finemap at the runs given on the command line under the
AQ_FM_BATCH_TILES of its environment, read when the entry runs.  Writes the dense alpha and mu, the per-trait outputs and the
plan's batch_tiles and n_batches per run to the .npz named first.
Usage: python -m tests.finemap_child OUT.npz n,p,q,pattern,L,max_iter [...]"""
import sys

import numpy as np


def main(out, runs):
    from tests import test_gpu_finemap as T
    res = {}
    for run in runs:
        n, p, q, pattern, L, iters = run.split(",")
        shape = (int(n), int(p), int(q))
        got = T.fit(shape, pattern, int(L), tol=0.0, max_iter=int(iters))
        for key in T.STATE + ("batch_tiles", "n_batches"):
            res[f"{key}_{run}"] = got[key] if key in got else got["plan"][key]
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
