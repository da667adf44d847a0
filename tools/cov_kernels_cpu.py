#!/usr/bin/env python3
"""The covariate kernels (atlasqtl_amd/csrc/aq_cov_kernels.h) run on the CPU by tools/cov_kernels_cpu.cpp and put through
the assertions of tests/test_gpu_covariates.py::test_residuals_match_the_long_double_truth: a check of the kernels' source
for a machine without a GPU.  Needs g++ with C++20 and the built library (for aq_cov_basis).  Minutes, not seconds: every
workgroup is 256 host threads.

    python tools/cov_kernels_cpu.py            # (n, p, q, d, na) = (50, 16, 3, 1, 0), (333, 100, 7, 5, 0.1), (200, 64, 4, 96, 0.2)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(tmp):
    src = open(os.path.join(ROOT, "atlasqtl_amd", "csrc", "aq_cov_kernels.h")).read()
    src = src.replace("extern __shared__ double lds[];", "extern double lds[];").replace("#pragma unroll", "")
    with open(os.path.join(tmp, "aq_cov_kernels_host.h"), "w") as f:
        f.write(src)
    out = os.path.join(tmp, "libcovcpu.so")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-I", tmp, "-I", os.path.join(ROOT, "atlasqtl_amd", "csrc"),
                           "-o", out,
                           os.path.join(ROOT, "tools", "cov_kernels_cpu.cpp")])
    return C.CDLL(out)


def main():
    from atlasqtl_amd import _lib
    from oracle import prepare_oracle as PO
    import tests.test_gpu_covariates as T
    with tempfile.TemporaryDirectory() as tmp:
        E = build(tmp)

        def vp(a):
            return C.c_void_p(a.ctypes.data)

        def prepared(Y, X, Z):
            Zf = np.asfortranarray(Z, dtype=np.float64)
            n, d = Zf.shape
            Q = np.empty((n, d + 1), order="F")
            _lib.check(_lib.lib().aq_cov_basis(_lib.as_dp(Zf), n, d, _lib.as_dp(Q), None), "aq_cov_basis")
            Xa = np.asfortranarray(X)
            p = Xa.shape[1]
            Xr, ab, r2 = np.full((n, p), np.nan, order="F"), np.zeros(p, np.uint8), np.zeros(p)
            (E.run_x_i8 if Xa.dtype == np.int8 else E.run_x_f64)(vp(Xa), n, p, d + 1, vp(Q), vp(Xr), vp(ab), vp(r2))
            Yf = np.asfortranarray(Y, dtype=np.float64)
            q = Yf.shape[1]
            Yc, nobs, flag = np.full((n, q), 7.0, order="F"), np.zeros(q, np.int32), np.full(q, 9, np.int32)
            E.run_y(vp(Yf), n, q, d + 1, vp(Q), vp(Yc), vp(nobs), vp(flag))
            assert (flag == 0).all() and (nobs == (~np.isnan(Yf)).sum(0)).all()
            Xs, _, cst, coll_kept = PO.prepare_xy(Yc, Xr)            # the pipeline that follows on the device, restated
            coll = np.zeros_like(cst)
            coll[~cst] = coll_kept
            dup = np.full(p, -1, dtype=np.int32)
            dup[[7, 11, p - 1]] = 1, 1, 4
            return dict(cst=cst, coll=coll, dup=dup, Xs=Xs, Yc=Yc, p=Xs.shape[1], n_cov=d, absorbed=ab.astype(bool), r2=r2)

        T._prepared = prepared
        for case in ((50, 16, 3, 1, 0.0), (333, 100, 7, 5, 0.1), (200, 64, 4, 96, 0.2)):
            T.test_residuals_match_the_long_double_truth(*case)
            print("ok", case, flush=True)


if __name__ == "__main__":
    main()
