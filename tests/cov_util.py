"""The truth for the covariate tests: the definition of aq_prepare_data_cov (include/atlasqtl_hip.h) restated in plain NumPy
with np.longdouble, independent of the library.  Results are rounded to fp64 and then go through oracle.prepare_oracle.prepare_xy,
the restatement of the unchanged pipeline.  np.linalg.lstsq is NOT the truth: in fp64 it is 2e-13 to 1.3e-12 off on these
covariates (an age-like 50 +- 10 column, a column on a 1e3 scale), which is the size of the bars themselves."""
import numpy as np

LD = np.longdouble
TOL = 1e-10           # absorbed column of X / collinear covariate: the rule of the header, not a tolerance of the tests


def covariates(n, d, rng):
    """The ill-scaled covariate set: standard normal; column 1 binary; column 2 age-like; column 3 on a 1e3 scale."""
    Z = rng.normal(size=(n, d))
    if d > 1:
        Z[:, 1] = (rng.random(n) < 0.4).astype(float)
    if d > 2:
        Z[:, 2] = 50.0 + 10.0 * rng.normal(size=n)
    if d > 3:
        Z[:, 3] = 1e3 * rng.normal(size=n) + Z[:, 0]
    return Z


def with_intercept(Z):
    Z = np.asarray(Z, dtype=np.float64)
    return np.column_stack([np.ones(Z.shape[0]), Z])


def basis_ld(W):
    """Orthonormal basis of W's columns, in order, by modified Gram-Schmidt applied twice, in long double.  Returns
    (Q, bad): bad is the first column whose remainder has a squared norm <= TOL times its own, else None."""
    W = np.asarray(W).astype(LD)
    n, D = W.shape
    Q = np.zeros((n, D), dtype=LD)
    for l in range(D):
        v = W[:, l].copy()
        own = v @ v
        for _ in range(2):
            for k in range(l):
                v -= Q[:, k] * (Q[:, k] @ v)
        rem = v @ v
        if not rem > LD(TOL) * own:
            return Q, l
        Q[:, l] = v / np.sqrt(rem)
    return Q, None


def residualise_x(X, Z):
    """x_j - Q (Q' x_j) applied twice; absorbed and constant columns become 0.0.  Returns (Xr fp64, absorbed, r2)."""
    Q, bad = basis_ld(with_intercept(Z))
    assert bad is None
    X = np.asarray(X, dtype=np.float64)
    Xl = X.astype(LD)
    cst = X.max(axis=0) == X.min(axis=0)
    s0 = ((Xl - Xl.mean(axis=0)) ** 2).sum(axis=0)
    R = Xl.copy()
    for _ in range(2):
        R -= Q @ (Q.T @ R)
    s1 = (R ** 2).sum(axis=0)
    absorbed = ~cst & (s1 <= LD(TOL) * s0)
    R[:, cst | absorbed] = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        r2 = np.where(cst, np.nan, (1 - s1 / np.where(cst, 1, s0)).astype(np.float64))
    return R.astype(np.float64), absorbed, r2


def residualise_y(Y, Z):
    """Per trait, the least-squares residual on [1, Z] over its observed rows (MGS twice on those rows); NaN stays NaN."""
    Y = np.asarray(Y, dtype=np.float64)
    W = with_intercept(Z)
    out = np.full(Y.shape, np.nan)
    complete = None
    for k in range(Y.shape[1]):
        obs = ~np.isnan(Y[:, k])
        if obs.all():
            if complete is None:
                complete = basis_ld(W)
            Q, bad = complete
        else:
            Q, bad = basis_ld(W[obs])
        assert bad is None, (k, bad)
        e = Y[obs, k].astype(LD)
        for _ in range(2):
            e -= Q @ (Q.T @ e)
        out[obs, k] = e.astype(np.float64)
    return out


def truth(Y, X, Z):
    """What prepare_on_device(Y, X, covariates=Z) must return: dict(Xs, Yc, cst, coll (original numbering), absorbed, r2, Q)."""
    from oracle import prepare_oracle as PO
    Xr, absorbed, r2 = residualise_x(X, Z)
    Yr = residualise_y(Y, Z)
    Xs, Yc, cst, coll_kept = PO.prepare_xy(Yr, Xr)
    coll = np.zeros_like(cst)
    coll[~cst] = coll_kept
    Q, _ = basis_ld(with_intercept(Z))
    return dict(Xs=Xs, Yc=Yc, cst=cst, coll=coll, absorbed=absorbed, r2=r2, Q=Q.astype(np.float64), Xr=Xr)
