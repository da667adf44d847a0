"""The marginal screen: every predictor tested against every trait on its own (the univariate scan in the style of Matrix
eQTL that a joint fit is compared with), on the GPU from a prepare handle (aq_prep_marginal, csrc/aq_prep_marginal.hip).

The GPU does the p q work -- the correlations on the f64 matrix pipe and the selection in registers -- and returns the selected
pairs, the per-predictor counts and each trait's best predictor.  The host does O(q) and O(selected pairs) work, all of it
here: the user's threshold as a per-trait cutoff on r^2, and t, the p-value and the Benjamini-Hochberg q-value of the rows
that came back.

Definition (include/atlasqtl_hip.h).  Over the m_t observed rows of trait t: r = Sxy / sqrt(Vx Syy_t) with
Vx = Sxx - Sx^2 / m_t; df_t = m_t - 2 - n_cov; t = r sqrt(df_t / (1 - r^2)); the p-value is two-sided Student's t with df_t
degrees of freedom.  A pair is undefined (r NaN, never selected) when the predictor is constant over the trait's observed rows
(Vx <= 1e-10 Sxx), when Syy_t = 0 or when df_t < 1.
"""
from __future__ import annotations

import numpy as np

from .prepare import AtlasqtlError, _is_whole, prepare_data_

DENSE_MAX = 1 << 27           # entries of the dense r that dense=True returns (1 GiB of fp64)
INITIAL_CAP = 1 << 16         # rows of the first call's table; a second call with cap = n_pairs follows when they do not suffice
SCREEN_KEYS = ("p_value", "fdr", "max_pairs")


def _is_level(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_)) and 0.0 < float(x) <= 1.0


def screen_options(p_value=None, fdr=None, max_pairs=None, dense=False, p=None, q=None):
    """The threshold arguments of marginal_screen() checked on the host.  At most one of p_value and fdr, each in (0, 1];
    neither means Bonferroni, p_value = 0.05 / (p q), resolved once p and q are known.  max_pairs: None or a whole number
    >= 1.  dense=True is refused above 2^27 entries.  Returns dict(mode "p_value" | "fdr" | "bonferroni", level (None until p
    and q are known, for Bonferroni), max_pairs, dense)."""
    if p_value is not None and fdr is not None:
        raise AtlasqtlError("marginal_screen: at most one of p_value and fdr may be given.")
    for name, v in (("p_value", p_value), ("fdr", fdr)):
        if v is not None and not _is_level(v):
            raise AtlasqtlError(f"marginal_screen: {name} must be a number in (0, 1], not {v!r}.")
    if max_pairs is not None and (not _is_whole(max_pairs) or int(max_pairs) < 1):
        raise AtlasqtlError(f"marginal_screen: max_pairs must be None or a whole number >= 1, not {max_pairs!r}.")
    if not isinstance(dense, (bool, np.bool_)):
        raise AtlasqtlError(f"marginal_screen: dense must be True or False, not {dense!r}.")
    known = p is not None and q is not None
    if dense and known and int(p) * int(q) > DENSE_MAX:
        raise AtlasqtlError(f"marginal_screen: dense=True would return {int(p) * int(q)} correlations, at most {DENSE_MAX} "
                            "(2^27) are supported; read the selected pairs off `assoc` instead.")
    if p_value is not None:
        mode, level = "p_value", float(p_value)
    elif fdr is not None:
        mode, level = "fdr", float(fdr)
    else:
        mode, level = "bonferroni", (0.05 / (int(p) * int(q)) if known else None)
    return dict(mode=mode, level=level, max_pairs=None if max_pairs is None else int(max_pairs), dense=bool(dense))


def screen_arg(marginal_screen):
    """The `marginal_screen` argument of atlasqtl(): None (no screen), True, or a dict with keys among 'p_value', 'fdr',
    'max_pairs'.  Returns None or the keyword arguments of screen_options, checked."""
    if marginal_screen is None or marginal_screen is False:
        return None
    if marginal_screen is True:
        marginal_screen = {}
    if not isinstance(marginal_screen, dict) or set(marginal_screen) - set(SCREEN_KEYS):
        raise AtlasqtlError("marginal_screen must be None, True or a dict with keys among 'p_value', 'fdr', 'max_pairs'.")
    screen_options(**marginal_screen)
    return dict(marginal_screen)


def r2_cutoff(level, df):
    """The cutoff on r^2 of a two-sided p-value `level` per trait: with t_c = isf(level / 2) of Student's t with df_t degrees
    of freedom, r^2_c = t_c^2 / (t_c^2 + df_t), so that p <= level exactly when r^2 >= r^2_c.  +inf where df_t < 1; level = 1
    is the cutoff 0, which every defined pair passes."""
    from scipy.stats import t as student
    df = np.atleast_1d(np.asarray(df, dtype=np.float64))
    out = np.full(df.shape, np.inf)
    ok = df >= 1
    if float(level) >= 1.0:
        out[ok] = 0.0
        return out
    tc = student.isf(0.5 * float(level), df[ok])
    out[ok] = np.where(np.isinf(tc), 1.0, tc * tc / (tc * tc + df[ok]))
    return out


def t_and_pvalue(r, df):
    """(t, two-sided p-value) of correlations r with df degrees of freedom each: t = r sqrt(df / (1 - r^2)), +-inf and p = 0
    where r^2 >= 1."""
    from scipy.stats import t as student
    r = np.asarray(r, dtype=np.float64)
    df = np.broadcast_to(np.asarray(df, dtype=np.float64), r.shape)
    one = 1.0 - r * r
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(one > 0, r * np.sqrt(df / np.where(one > 0, one, 1.0)), np.sign(r) * np.inf)
    return t, 2.0 * student.sf(np.abs(t), df)


def bh_qvalues(pvalue_sorted, n_tests):
    """Benjamini-Hochberg q-values of the k smallest p-values of n_tests tests, given in ascending order:
    q_i = min over j >= i of p_j n_tests / j, at most 1.  Tied p-values get one q-value.  The minimum runs over the k values
    given: where every p-value not given exceeds a level alpha, q_i is exact wherever it is <= alpha and an upper bound
    elsewhere, so the set {q <= alpha} is exactly the Benjamini-Hochberg set at alpha."""
    pv = np.asarray(pvalue_sorted, dtype=np.float64)
    if pv.size == 0:
        return pv.copy()
    if np.any(np.diff(pv) < 0):
        raise ValueError("bh_qvalues needs the p-values in ascending order")
    raw = pv * float(n_tests) / np.arange(1, pv.size + 1)
    return np.minimum(np.minimum.accumulate(raw[::-1])[::-1], 1.0)


def table_order(pvalue, t, snp, trait, p):
    """The order of the table: by p-value, then by decreasing |t| (p-values underflow to equal zeros before |t| stops
    telling pairs apart), then by the position snp + p trait in the p x q matrix."""
    pos = np.asarray(snp, dtype=np.int64) + int(p) * np.asarray(trait, dtype=np.int64)
    return np.lexsort((pos, -np.abs(np.asarray(t, dtype=np.float64)), np.asarray(pvalue, dtype=np.float64)))


def screen_handle(prep, names_x, names_y, p_value=None, fdr=None, max_pairs=None, dense=False):
    """The screen on a PreparedData as it stands: marginal_screen() without the preparation.  Returns the result dict without
    the rmvd_* fields."""
    from .api import AtlasqtlResult
    p, q = int(prep.p), int(prep.q)
    o = screen_options(p_value, fdr, max_pairs, dense, p, q)
    n_obs = np.sum(~np.isnan(prep.Y), axis=0).astype(np.int64)
    df = n_obs - 2 - int(prep.n_cov)
    cut = r2_cutoff(o["level"], df)
    cap = int(min(p * q, INITIAL_CAP))
    out = prep.marginal(cut, cap, dense=o["dense"])
    if out["n_pairs"] > cap:                                  # the complete set, whatever order the first call filled its rows in
        out = prep.marginal(cut, out["n_pairs"], dense=o["dense"])
    snp, trait, r = out["snp"], out["trait"], out["r"]
    dfr = df[trait].astype(np.float64)
    t, pv = t_and_pvalue(r, dfr)
    order = table_order(pv, t, snp, trait, p)
    snp, trait, r, t, pv, dfr = snp[order], trait[order], r[order], t[order], pv[order], dfr[order]
    n_tests = p * q - int(out["n_undefined"])
    qv = bh_qvalues(pv, n_tests)
    rs = np.asarray(out["rs"], dtype=np.int64)
    if o["mode"] == "fdr":                                    # the device selected p <= alpha, a superset of the BH set
        keep = int(np.sum(qv <= o["level"]))                  # q is non-decreasing along the table
        snp, trait, r, t, pv, dfr, qv = (a[:keep] for a in (snp, trait, r, t, pv, dfr, qv))
        rs = np.bincount(snp, minlength=p).astype(np.int64)
    n_pairs = int(snp.size)
    m = n_pairs if o["max_pairs"] is None else min(n_pairs, o["max_pairs"])
    assoc = dict(snp=snp[:m], trait=trait[:m], r=r[:m], t=t[:m], df=dfr[:m].astype(np.int64), pvalue=pv[:m], qvalue=qv[:m],
                 snp_name=np.asarray(names_x, dtype=object)[snp[:m]], trait_name=np.asarray(names_y, dtype=object)[trait[:m]],
                 n_pairs=n_pairs)
    best_snp, best_r = out["best_snp"], out["best_r"]
    best_p = np.full(q, np.nan)
    has = best_snp >= 0
    best_p[has] = t_and_pvalue(best_r[has], df[has])[1]
    res = AtlasqtlResult(assoc=assoc, rs_thres=rs, nb_pairwise=n_pairs, best_snp=best_snp, best_r=best_r, best_pvalue=best_p,
                         n_obs=n_obs, df=df, n_undefined=int(out["n_undefined"]), n=int(prep.n), p=p, q=q,
                         threshold=dict(mode=o["mode"], level=o["level"], r2_cut=cut, n_tests=n_tests),
                         names_x=list(names_x), names_y=list(names_y))
    if o["dense"]:
        res["r"] = out["r_dense"]
    return res


def marginal_screen(Y, X, p_value=None, fdr=None, max_pairs=None, covariates=None, ld_prune=None, transform_y=None, dense=False,
                    device=0):
    """Every predictor of X tested against every trait of Y on its own, on the GPU.

    X and Y are prepared exactly as atlasqtl() prepares them (prepare_on_device: X float64, int8 dosages or a plink.PlinkBed;
    constant and duplicated predictors removed; `covariates`, `ld_prune`, `transform_y` as there), and the screen runs on the
    prepared handle: for every remaining predictor s and trait t the Pearson correlation r over the trait's observed rows,
    t = r sqrt(df / (1 - r^2)) with df = m_t - 2 - d (m_t observed values, d covariates) and the two-sided p-value of Student's
    t.  With covariates and missing values the predictors were residualised over all samples, not over the trait's observed
    ones: the same approximation that the `covariates` argument of atlasqtl() describes.

    Selection: p_value=c keeps the pairs with p <= c; fdr=a keeps the Benjamini-Hochberg set at level a over the M = p q -
    n_undefined defined tests (the GPU selects p <= a, a superset, and the host cuts it); neither means Bonferroni,
    p_value = 0.05 / (p q).  At most one of the two.  The table is ordered by (p-value, -|t|, position snp + p trait);
    max_pairs cuts the ordered complete table.

    Returns an AtlasqtlResult with
      assoc: dict(snp, trait [indices into names_x / names_y], r, t, df, pvalue, qvalue [Benjamini-Hochberg over M tests;
        exact wherever it is <= the threshold used, an upper bound elsewhere], snp_name, trait_name, n_pairs [the size of the
        complete table]);
      rs_thres: per fitted predictor, its number of selected traits -- the marginal hotspot sizes, with the name and the
        meaning of the fit's; nb_pairwise: their sum;
      best_snp, best_r, best_pvalue: per trait, the predictor of largest r^2 (the lowest index on a tie; -1 / NaN where no pair
        of the trait is defined);
      n_obs, df: per trait; n_undefined: pairs without a defined r; threshold: dict(mode, level, r2_cut [per trait], n_tests);
      names_x, names_y, n, p, q, and rmvd_cst_x, rmvd_coll_x, rmvd_cov_x, rmvd_ld_x as prepare_data_ gives them;
      r: with dense=True, the p x q matrix of correlations (NaN where undefined); refused above 2^27 entries."""
    screen_options(p_value, fdr, max_pairs, dense)             # before the first device call
    dat = prepare_data_(Y, X, 0.1, 1, None, 0, None, None, device=device, covariates=covariates, ld_prune=ld_prune,
                        transform_y=transform_y)
    prep = dat["X"]
    try:
        res = screen_handle(prep, dat["names_x"], dat["names_y"], p_value, fdr, max_pairs, dense)
    finally:
        prep.close()
    for key in ("rmvd_cst_x", "rmvd_coll_x", "rmvd_cov_x", "rmvd_ld_x"):
        res[key] = dat[key]
    res["n_covariates"] = dat["n_covariates"]
    return res
