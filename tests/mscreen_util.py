"""The marginal screen restated for the tests, independent of atlasqtl_amd: the correlation of every predictor with every
trait in np.longdouble on a handle's own matrices (prep.X_host() and prep.Y, so that the preparation is not tested again), the
elementwise error bound of an fp64 evaluation in any order, the selection read off the reference, and inputs to run it on.

Definition (include/atlasqtl_hip.h, aq_prep_marginal).  For predictor s and trait t, over the m_t rows O_t where the trait is
observed: Sxy = sum x y, Sx = sum x, Sxx = sum x^2, Syy = sum y^2; Vx = Sxx - Sx^2 / m_t; r = Sxy / sqrt(Vx Syy);
df_t = m_t - 2 - n_cov.  Undefined (NaN) when Vx <= 1e-10 Sxx, Syy = 0 or df_t < 1."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
FACTOR = 2.0      # on the first-order bound: the epilogue's few roundings (a division, a product, a square root, a division) and
                  # second-order terms


def reference(Xs, Yc, n_cov=0):
    """(r_ref [p x q, long double, NaN where undefined], bound [p x q], m [q], df [q]).

    bound: every m-term fp64 sum, in any order and with one rounding per term, is within (m + 2) 2^-53 sum |terms| of the exact
    value (the form of tests/grm_util.grm_bound).  Propagated through r = Sxy (Vx Syy)^(-1/2) to first order:
      dVx <= dSxx + 2 |Sx| dSx / m,     dr <= dSxy / sqrt(Vx Syy) + |r| / 2 (dVx / Vx + dSyy / Syy),
    times FACTOR."""
    Xl = np.asarray(Xs, dtype=LD)
    Yl = np.asarray(Yc, dtype=LD)
    n, p = Xl.shape
    q = Yl.shape[1]
    r = np.full((p, q), np.nan, dtype=LD)
    B = np.full((p, q), np.nan, dtype=LD)
    m = np.zeros(q, dtype=np.int64)
    for t in range(q):
        obs = ~np.isnan(Yc[:, t])
        m[t] = int(obs.sum())
        df = m[t] - 2 - n_cov
        if m[t] == 0:
            continue
        Xo, y = Xl[obs], Yl[obs, t]
        sxy, axy = y @ Xo, np.abs(y) @ np.abs(Xo)
        sx, ax = Xo.sum(axis=0), np.abs(Xo).sum(axis=0)
        sxx = (Xo * Xo).sum(axis=0)
        syy = (y * y).sum()
        vx = sxx - sx * sx / LD(m[t])
        ok = (vx > LD(1e-10) * sxx) & (syy > 0) & (df >= 1)
        e = LD((m[t] + 2) * U)
        with np.errstate(divide="ignore", invalid="ignore"):
            den = np.sqrt(vx * syy)
            rt = sxy / den
            dvx = e * sxx + 2 * np.abs(sx) * e * ax / LD(m[t])
            bt = e * axy / den + np.abs(rt) / 2 * (dvx / vx + e)          # dSyy / Syy = e: every term of Syy is positive
        r[ok, t] = rt[ok]
        B[ok, t] = LD(FACTOR) * bt[ok]
    return r, B, m, m - 2 - n_cov


def selection(r_ref, cut):
    """What aq_prep_marginal returns for the reference r: (set of (snp, trait), rs [p], n_undefined, best_snp [q])."""
    r = np.asarray(r_ref, dtype=np.float64)
    defined = ~np.isnan(r)
    r2 = np.where(defined, r * r, -1.0)
    sel = defined & (r2 >= np.asarray(cut)[None, :])
    rows = set(zip(*(int_list(a) for a in np.nonzero(sel))))
    best = np.where(defined.any(axis=0), np.argmax(r2, axis=0), -1)     # argmax: the first of equal values
    return rows, sel.sum(axis=1).astype(np.int64), int((~defined).sum()), best.astype(np.int32)


def int_list(a):
    return [int(v) for v in a]


def clear_cutoffs(r_ref, quantile=0.8, margin=1e-9):
    """A cutoff on r^2 per trait from which no reference r^2 of the trait lies within 4 `margin`: of the midpoints of the gaps
    wider than 8 margin between neighbouring order statistics of the defined r^2, half the smallest value and one above the
    largest, the candidate nearest to the `quantile` of the values.  +inf for a trait without a defined pair."""
    r = np.asarray(r_ref, dtype=np.float64)
    q = r.shape[1]
    cut = np.full(q, np.inf)
    for t in range(q):
        v = np.sort(r[~np.isnan(r[:, t]), t] ** 2)
        if v.size == 0:
            continue
        gaps = np.diff(v)
        wide = gaps > 8 * margin
        cands = list(0.5 * (v[:-1] + v[1:])[wide]) + [v[-1] + 1.0] + ([0.5 * v[0]] if v[0] > 8 * margin else [])
        target = v[int(round(quantile * (v.size - 1)))]
        cut[t] = min(cands, key=lambda c: abs(c - target))
    return cut


def cutoffs_are_clear(r_ref, cut, margin=1e-9):
    r = np.asarray(r_ref, dtype=np.float64)
    d = np.abs(r * r - np.asarray(cut)[None, :])
    return bool(np.all(d[~np.isnan(r)] > margin))


MISSING_KINDS = ("random", "one_complete", "few")


def case(n, p, q, missing=None, seed=0, few_m=None):
    """Raw inputs (X float64 n x p, Y n x q) with what the tests look for planted:
      - predictors 0 and 1 are x and -x, and trait 0 is 3 x + noise: the two share the trait's largest r^2 exactly, and the
        lower index must win (two identical predictors would not survive the duplicate removal);
      - with missing values, predictor 2 varies overall but is constant over the observed rows of the last trait: undefined there.
    missing: None (complete); "random": 10 % NaN at random; "one_complete": the same with trait 0 fully observed;
    "few": the same, and the last trait keeps only its first m rows, m = max(3, ceil(0.025 n)) -- three where the preparation's
    guard against traits with more than 97.5 % missing values allows it (n <= 120), else the fewest it allows; few_m sets m."""
    rng = np.random.default_rng(seed + 7919 * n + 31 * p + q)
    X = rng.standard_normal((n, p))
    X[:, 1] = -X[:, 0]
    Y = rng.standard_normal((n, q)) + 0.3 * X[:, [j % p for j in range(q)]]
    Y[:, 0] = 3.0 * X[:, 0] + 0.5 * rng.standard_normal(n)
    if missing is not None:
        assert missing in MISSING_KINDS
        mask = rng.random((n, q)) < 0.10
        mask[:3] = False                                       # every trait keeps three observed rows
        if missing == "one_complete":
            mask[:, 0] = False
        last = q - 1
        if missing == "few":
            m = max(3, int(np.ceil(0.025 * n))) if few_m is None else int(few_m)
            mask[:, last] = True
            mask[:m, last] = False
        if not mask[:, last].any():
            mask[n - 1, last] = True
        Y[mask] = np.nan
        X[:, 2] = np.where(mask[:, last], 1.0 + rng.random(n), 0.0)    # constant (0) where the last trait is observed
    return np.asfortranarray(X), np.asfortranarray(Y)
