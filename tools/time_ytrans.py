"""Measurement of transform_y: a host clock around aq_rank_int at (n, q) = (1000, 10 000), (5000,
20 000) and (82 944, 64) -- one warm-up and three calls in one process, the copies of Y to and from the device included;
the kernels alone as the difference of prepare_on_device with and without the transform on eight predictors, which makes
the same copies on both sides -- beside the host route it replaces (scipy.stats.rankdata + scipy.special.ndtri per column, on the CPUs this process may
use, 16 at most), and around aq_prepare_data_opt at C3 (n = 1000, p = 50 000 int8 dosages, q = 10 000) with and without the
transform.  Prints one JSON line per measurement.

    python tools/time_ytrans.py [--quick]        (--quick: a tenth of the traits and predictors, to try the tool out)
"""
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1000, 10000), (5000, 20000), (82944, 64)]
C3 = (1000, 50000, 10000)
_Y = _OUT = None


def make_y(n, q, seed=0):
    """Skewed, heavy-tailed traits with 2 % missing values, in Fortran order."""
    rng = np.random.default_rng(seed)
    Y = np.empty((n, q), order="F")
    for k0 in range(0, q, 256):
        k1 = min(q, k0 + 256)
        blk = np.exp(rng.standard_normal((n, k1 - k0)))
        blk[rng.random(blk.shape) < 0.02] = np.nan
        Y[:, k0:k1] = blk
    return Y


def _host_columns(rng_):
    from scipy.special import ndtri
    from scipy.stats import rankdata
    k0, k1 = rng_
    for k in range(k0, k1):
        col = _Y[:, k]
        obs = ~np.isnan(col)
        m = int(obs.sum())
        res = np.full(col.shape, np.nan)
        res[obs] = ndtri((rankdata(col[obs], method="average") - 0.375) / (m + 0.25))
        _OUT[:, k] = res


def host_route(Y, workers):
    """rankdata + ndtri per column over `workers` forked processes that write into one shared n x q array; seconds of the
    best of three."""
    global _Y, _OUT
    n, q = Y.shape
    _Y = Y
    _OUT = np.frombuffer(mp.RawArray("d", n * q), dtype=np.float64).reshape((n, q), order="F")
    step = max(1, -(-q // (4 * workers)))
    parts = [(k0, min(q, k0 + step)) for k0 in range(0, q, step)]
    best = np.inf
    with mp.get_context("fork").Pool(workers) as pool:
        for _ in range(3):
            t0 = time.perf_counter()
            pool.map(_host_columns, parts)
            best = min(best, time.perf_counter() - t0)
    return best


def clock(fn, reps=3):
    fn()                                                       # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def main(quick):
    workers = min(16, len(os.sched_getaffinity(0)))
    shapes = [(n, max(4, q // 10)) for n, q in SHAPES] if quick else SHAPES
    n3, p3, q3 = (C3[0], C3[1] // 10, C3[2] // 10) if quick else C3
    data = {s: make_y(*s) for s in shapes}
    host = {s: host_route(Y, workers) for s, Y in data.items()}   # before the GPU is opened: the pool is forked
    import ctypes as C
    from atlasqtl_amd import _lib
    from atlasqtl_amd import prepare as P
    L = _lib.lib()
    for (n, q), Y in data.items():
        out = np.empty_like(Y)
        pl = _lib.AqYtransPlan()
        _lib.check(L.aq_ytrans_plan_query(n, q, 1 << 34, C.byref(pl)), "aq_ytrans_plan_query")
        ts = clock(lambda: _lib.check(L.aq_rank_int(_lib.as_dp(Y), n, q, 0.375, _lib.as_dp(out), None, None, 0), "aq_rank_int"))
        t = float(np.median(ts))
        # the kernel without the copies of Y, which both sides of this difference make: prepare with and without the transform
        # on eight predictors
        X8 = np.asfortranarray(np.random.default_rng(3).binomial(2, 0.3, size=(n, 8)).astype(np.int8))
        d = [float(np.median(clock(lambda: P.prepare_on_device(Y, X8, transform_y=o)[0].close()))) for o in ("int", None)]
        k = d[0] - d[1]
        print(json.dumps(dict(what="aq_rank_int", n=n, q=q, path="global" if pl.path else "lds", n_pad=pl.n_pad, seconds=ts,
                              median_s=t, gbytes_per_s=16.0 * n * q / t / 1e9, host_route_s=host[(n, q)], host_workers=workers,
                              speedup=host[(n, q)] / t, kernel_s_by_difference=k, kernel_gbytes_per_s=16.0 * n * q / k / 1e9,
                              kernel_ns_per_key=k / (n * q) * 1e9)), flush=True)
    del data
    rng = np.random.default_rng(1)
    X = np.asfortranarray(rng.binomial(2, 0.3, size=(n3, p3)).astype(np.int8))
    Y = make_y(n3, q3, seed=2)

    def prepare(transform_y):
        P.prepare_on_device(Y, X, transform_y=transform_y)[0].close()

    t_with, t_without = clock(lambda: prepare("int")), clock(lambda: prepare(None))
    a, b = float(np.median(t_with)), float(np.median(t_without))
    print(json.dumps(dict(what="aq_prepare_data_opt", n=n3, p=p3, q=q3, with_transform_s=t_with, without_s=t_without,
                          median_with_s=a, median_without_s=b, transform_share=(a - b) / a)), flush=True)


if __name__ == "__main__":
    main("--quick" in sys.argv[1:])
