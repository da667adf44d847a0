"""Child process of tests/test_gpu_predict.py: predict_util.run_shape at the shapes given on the command line under the
AQ_PREDICT_SPLITS / AQ_KERNEL of its environment, read when the handle is created and when the entries run.  Writes what
run_shape returns per shape to the .npz named first.  A fourth number 1 asks for Y with missing
values.  Usage: python -m tests.predict_child OUT.npz n_new,p,q[,na] [n_new,p,q[,na] ...]"""
import sys

import numpy as np


def main(out, shapes):
    from tests import predict_util as PU
    res = {}
    for shape in shapes:
        n_new, p, q, *na = (int(v) for v in shape.split(","))
        for k, v in PU.run_shape(n_new, p, q, na=bool(na and na[0])).items():
            res[f"{k}_{shape}"] = v
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
