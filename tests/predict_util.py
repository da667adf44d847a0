"""Shared by tests/test_gpu_predict.py and its child process tests/predict_child.py: small problems with exact shapes, the
yardstick of a prediction and its bound, and the one routine that runs a shape through a handle.

The yardstick is computed independently of the package: Xt = (X_new - center) / scale and Xt @ beta_vb in numpy.longdouble,
beta_vb the dense result of the same run.  The bound per entry is (p + 8) 2^-53 sum_s |Xt_is beta_st| + 1e-300: p 2^-53 is the
bound of a dot product of p terms in any summation order, and 8 covers the roundings outside it -- 1 / scale, x - center, their
product, gam * mu (1 each), the additions of the partial sums of up to 64 splits being part of the summation order."""
import ctypes as C
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SHAPES = [(1, 5, 1), (15, 16, 16), (17, 33, 17), (130, 257, 40), (64, 1000, 130)]      # (n_new, p, q)
N_FIT = 48


def dosages(n, p, seed):
    """n x p int8 dosages (0 / 1 / 2) whose columns are all different and none constant, whatever n >= 16 and p <= 4096 are:
    rows 0 ... 11 spell the column's index in binary, rows 12 and 13 hold 2 and 0."""
    assert n >= 16 and p <= 4096
    rng = np.random.default_rng(seed)
    G = rng.binomial(2, 0.3, size=(n, p)).astype(np.int8)
    j = np.arange(p)
    for b in range(12):
        G[b] = (j >> b) & 1
    G[12], G[13] = 2, 0
    return np.asfortranarray(G)


def yardstick(X_new, center, scale, beta):
    """(Xt @ beta in long double, the bound per entry) for X_new with the columns of beta's rows."""
    Xt = (np.asarray(X_new).astype(LD) - np.asarray(center, dtype=LD)) / np.asarray(scale, dtype=LD)
    B = np.asarray(beta).astype(LD)
    p = B.shape[0]
    return Xt @ B, (p + 8) * LD(U) * (np.abs(Xt) @ np.abs(B)) + LD(1e-300)


def assert_within(got, want, bound, what):
    err = np.abs(np.asarray(got).astype(LD) - want)
    worst = float(np.max(err / bound))
    print(f"{what}: max |err| / bound = {worst:.3g} (max |err| = {float(err.max()):.3g})")
    assert np.isfinite(np.asarray(got)).all() and worst <= 1.0, (what, worst)


@functools.lru_cache(maxsize=None)
def fit_case(p, q, na=False):
    """A problem with exactly p predictors and q traits for a handle: standardised X (host), centred Y, the two lists, and the
    standardisation (center, scale) of the raw dosages G."""
    from atlasqtl_amd import hyper_init as H
    G = dosages(N_FIT, p, seed=1000 + p)
    Gd = G.astype(np.float64)
    center, scale = Gd.mean(axis=0), Gd.std(axis=0, ddof=1)
    X = np.asfortranarray((Gd - center) / scale)
    rng = np.random.default_rng(7 + q)
    act = rng.choice(p, size=min(p, 3), replace=False)
    Y = X[:, act] @ rng.normal(size=(act.size, q)) + rng.normal(size=(N_FIT, q))
    if na:
        Y[rng.random(Y.shape) < 0.1] = np.nan
    Y = np.asfortranarray(Y - np.nanmean(Y, axis=0))
    p0 = (1, 2) if p < 20 else (5, 25)
    rm = np.zeros(p, dtype=bool)
    lh = H.prepare_list_hyper_(None, Y, p, p0, rm)
    li = H.prepare_list_init_(None, Y, p, p0, rm, q, 456)
    for a in (G, X, Y, center, scale):
        a.setflags(write=False)
    return dict(G=G, X=X, Y=Y, center=center, scale=scale, list_hyper=lh, list_init=li)


def new_rows(n_new, p):
    """New int8 dosages for a fit on p predictors."""
    return np.asfortranarray(np.random.default_rng(5000 + 31 * n_new + p).binomial(2, 0.3, size=(n_new, p)).astype(np.int8))


def run_shape(n_new, p, q, na=False, sweeps=2, ncu=None):
    """A handle for fit_case(p, q, na) after `sweeps` sweeps, applied to new_rows(n_new, p) given as int8 and as fp64, twice each:
    dict(beta: the dense beta_vb of the same handle, y8, y8b, y64, yd: predict() on that beta_vb as a dense result (the
    instances without mu), splits, sample_tiles, trait_tiles: of the plan the entries used, core_kernel).  ncu: AQ_NCU for the
    prediction calls alone, set once the sweeps have run (the hook is the sweep's planner's too)."""
    import os
    from atlasqtl_amd import _lib, prediction
    from atlasqtl_amd.core import VbRun
    c = fit_case(p, q, na)
    Xn = new_rows(n_new, p)
    run = VbRun(c["Y"], c["X"], c["list_hyper"], c["list_init"], None, 0.1, sweeps, True, True)
    try:
        run.run()
        beta = run.result()["beta_vb"]
        if ncu is not None:
            os.environ["AQ_NCU"] = str(ncu)
        y8 = run.predict(Xn, c["center"], c["scale"])
        y8b = run.predict(Xn, c["center"], c["scale"])
        y64 = run.predict(Xn.astype(np.float64), c["center"], c["scale"])
        ms, pl = C.c_double(0.0), _lib.AqPredictPlan()
        _lib.check(_lib.lib().aq_vb_predict_time(run.h, n_new, 1, C.byref(ms), C.byref(pl)), "aq_vb_predict_time")
        dense = dict(beta_vb=beta, predictor=prediction.predictor_of(np.zeros(p, dtype=bool), c["center"], c["scale"]))
        yd = prediction.predict(dense, Xn)
        return dict(beta=beta, y8=y8, y8b=y8b, y64=y64, yd=yd, splits=pl.splits, sample_tiles=pl.sample_tiles, trait_tiles=pl.trait_tiles,
                    core_kernel=run.status()["core_kernel"])
    finally:
        if ncu is not None:
            os.environ.pop("AQ_NCU", None)
        run.close()


def check_shape(out, n_new, p, q, what, na=False):
    """The result of run_shape against the yardstick."""
    c = fit_case(p, q, na)
    want, bound = yardstick(new_rows(n_new, p), c["center"], c["scale"], out["beta"])
    assert out["y8"].shape == (n_new, q) and np.abs(out["beta"]).max() > 0
    assert_within(out["y8"], want, bound, what)
    assert_within(out["yd"], want, bound, what + " (dense result)")
    # the int8 dosages convert to fp64 exactly, so the two inputs give the same bits; so do two calls
    assert out["y64"].tobytes() == out["y8"].tobytes() and out["y8b"].tobytes() == out["y8"].tobytes()
