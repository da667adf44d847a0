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

Permutation nulls (permutations=; aq_prep_marginal_perm, csrc/aq_prep_marginal_perm.hip).  The p-values above are per pair:
they do not correct a trait's best predictor for the p correlated predictors it was chosen from, and they do not say how large
a marginal hotspot correlated traits produce by chance.  Permuting the sample rows of Y, all traits together, keeps the LD among
predictors and the correlation among traits and breaks only the link between the two; every permutation is a whole screen on
the GPU, of which each trait's largest r^2, the largest hotspot size and the number of selected pairs come back.  The host
parses the argument (permutation_options) and turns the null statistics into p-values (permutation_summary).
"""
from __future__ import annotations

import numpy as np

from .checks import AtlasqtlError, _is_real, _is_whole
from .prepare import prepare_data_

DENSE_MAX = 1 << 27           # entries of the dense r that dense=True returns (1 GiB of fp64)
INITIAL_CAP = 1 << 16         # rows of the first call's table; a second call with cap = n_pairs follows when they do not suffice
SCREEN_KEYS = ("p_value", "fdr", "max_pairs")


def screen_options(p_value=None, fdr=None, max_pairs=None, dense=False, p=None, q=None, who="marginal_screen"):
    """The threshold arguments of marginal_screen() checked on the host.  At most one of p_value and fdr, each in (0, 1];
    neither means Bonferroni, p_value = 0.05 / (p q), resolved once p and q are known.  max_pairs: None or a whole number
    >= 1.  dense=True is refused above 2^27 entries.  Returns dict(mode "p_value" | "fdr" | "bonferroni", level (None until p
    and q are known, for Bonferroni), max_pairs, dense).  who: the entry whose arguments they are, which the messages name."""
    if p_value is not None and fdr is not None:
        raise AtlasqtlError(f"{who}: at most one of p_value and fdr may be given.")
    for name, v in (("p_value", p_value), ("fdr", fdr)):
        if v is not None and not _is_real(v, 0.0, 1.0, lo_open=True):
            raise AtlasqtlError(f"{who}: {name} must be a number in (0, 1], not {v!r}.")
    if max_pairs is not None and (not _is_whole(max_pairs) or int(max_pairs) < 1):
        raise AtlasqtlError(f"{who}: max_pairs must be None or a whole number >= 1, not {max_pairs!r}.")
    if not isinstance(dense, (bool, np.bool_)):
        raise AtlasqtlError(f"{who}: dense must be True or False, not {dense!r}.")
    known = p is not None and q is not None
    if dense and known and int(p) * int(q) > DENSE_MAX:
        raise AtlasqtlError(f"{who}: dense=True would return {int(p) * int(q)} correlations, at most {DENSE_MAX} "
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


def _check_perm_rows(perms, n):
    """perms as a B x n int32 array whose rows are permutations of 0 ... n - 1 (n None: of 0 ... width - 1), or the error."""
    a = np.asarray(perms)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1 or not np.issubdtype(a.dtype, np.integer):
        raise AtlasqtlError(f"marginal_screen: permutations given as an array must be B x n integers, not {a.dtype} {a.shape}.")
    if n is not None and a.shape[1] != int(n):
        raise AtlasqtlError(f"marginal_screen: the rows of permutations must have one entry per sample ({int(n)}), not {a.shape[1]}.")
    width = a.shape[1]
    bad = np.nonzero(np.any(np.sort(a, axis=1) != np.arange(width)[None, :], axis=1))[0]
    if bad.size:
        raise AtlasqtlError(f"marginal_screen: row {int(bad[0])} of permutations is not a permutation of 0 ... {width - 1}.")
    return np.ascontiguousarray(a, dtype=np.int32)


def permutation_options(permutations, n=None):
    """The `permutations` argument of marginal_screen() checked on the host.  None: no permutations.  A whole number B >= 1:
    B random permutations from seed 0.  A dict {"n": B, "seed": s} (seed optional, a whole number >= 0, default 0).  An integer
    array B x n of explicit permutations, every row a permutation of 0 ... n - 1: permutations restricted within sex or batch,
    or the identity.  Returns None or dict(n B, seed (None for explicit rows), perms (B x n int32; None until n is known)).
    Generated permutations are exactly
        rng = np.random.default_rng(seed); np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int32)"""
    if permutations is None:
        return None
    if isinstance(permutations, (bool, np.bool_, float, np.floating, str)):
        raise AtlasqtlError(f"marginal_screen: permutations must be None, a whole number >= 1, a dict with keys 'n' and 'seed' "
                            f"or an integer array B x n, not {permutations!r}.")
    if _is_whole(permutations) or isinstance(permutations, dict):
        spec = {"n": permutations} if _is_whole(permutations) else dict(permutations)
        if set(spec) - {"n", "seed"} or "n" not in spec:
            raise AtlasqtlError("marginal_screen: permutations given as a dict must have the key 'n' and may have 'seed'.")
        B, seed = spec["n"], spec.get("seed", 0)
        if not _is_whole(B) or int(B) < 1:
            raise AtlasqtlError(f"marginal_screen: the number of permutations must be a whole number >= 1, not {B!r}.")
        if not _is_whole(seed) or int(seed) < 0:
            raise AtlasqtlError(f"marginal_screen: the seed of permutations must be a whole number >= 0, not {seed!r}.")
        B, seed = int(B), int(seed)
        perms = None
        if n is not None:
            rng = np.random.default_rng(seed)
            perms = np.stack([rng.permutation(int(n)) for _ in range(B)]).astype(np.int32)
        return dict(n=B, seed=seed, perms=perms)
    perms = _check_perm_rows(permutations, n)
    return dict(n=int(perms.shape[0]), seed=None, perms=perms)


def permutation_trait_pvalue(max_r2, best_snp, best_r):
    """(1 + #{b: max_r2[b][t] >= best_r[t]^2}) / (B + 1) per trait, from max_r2 (B x q) and the observed best_snp, best_r (q):
    the permutation p-value of the trait's best predictor; NaN where the trait has no defined pair (best_snp[t] < 0)."""
    max_r2 = np.asarray(max_r2, dtype=np.float64)
    best_r = np.asarray(best_r, dtype=np.float64)
    has = np.asarray(best_snp) >= 0
    obs = np.where(has, best_r * best_r, np.inf)
    trait_p = (1.0 + np.sum(max_r2 >= obs[None, :], axis=0)) / (max_r2.shape[0] + 1.0)
    trait_p[~has] = np.nan
    return trait_p


def permutation_summary(max_r2, hs_max, n_sel, best_snp, best_r, rs_thres, nb_pairwise):
    """What the permutation nulls say about a screen, in numpy.  max_r2 (B x q), hs_max (B), n_sel (B): the outputs of
    PreparedData.marginal_permute; best_snp, best_r (q), rs_thres (p), nb_pairwise: of the screen.  Returns dict of
      trait_pvalue[t] = (1 + #{b: max_r2[b][t] >= best_r[t]^2}) / (B + 1): the p-value of the trait's best predictor, corrected
        for the predictors it was chosen from; NaN where the trait has no defined pair (best_snp[t] < 0);
      hotspot_pvalue[s] = (1 + #{b: hs_max[b] >= rs_thres[s]}) / (B + 1): of a hotspot of that size anywhere among the
        predictors (1 for a predictor without a selected trait);
      expected_null_pairs = mean(n_sel); empirical_fdr = min(1, expected_null_pairs / max(1, nb_pairwise))."""
    hs_max = np.asarray(hs_max, dtype=np.int64)
    B = np.shape(max_r2)[0]
    rs = np.asarray(rs_thres, dtype=np.int64)
    hot_p = (1.0 + (B - np.searchsorted(np.sort(hs_max), rs, side="left"))) / (B + 1.0)      # #{b: hs_max[b] >= rs[s]}
    expected = float(np.mean(np.asarray(n_sel, dtype=np.float64)))
    return dict(trait_pvalue=permutation_trait_pvalue(max_r2, best_snp, best_r), hotspot_pvalue=hot_p, expected_null_pairs=expected,
                empirical_fdr=min(1.0, expected / max(1, int(nb_pairwise))))


def association_table_(out, df, n_tests, mode, level, max_pairs, names_x, names_y, p):
    """What the host makes of the rows a scan returned (out: snp, trait, r, best_snp, best_r; df: per trait): t, p-value and
    Benjamini-Hochberg q-value over n_tests tests per row, the rows in table_order, in the mode "fdr" cut to q <= level, and
    `assoc`, the table cut to max_pairs rows with n_pairs the size of the complete one; best_pvalue per trait (NaN where
    best_snp < 0).  Returns (assoc, best_pvalue, snp, pvalue), the last two of the complete table."""
    snp, trait, r = out["snp"], out["trait"], out["r"]
    dfr = df[trait].astype(np.float64)
    t, pv = t_and_pvalue(r, dfr)
    order = table_order(pv, t, snp, trait, p)
    snp, trait, r, t, pv, dfr = snp[order], trait[order], r[order], t[order], pv[order], dfr[order]
    qv = bh_qvalues(pv, n_tests)
    if mode == "fdr":                                         # the device selected p <= alpha, a superset of the BH set
        keep = int(np.sum(qv <= level))                       # q is non-decreasing along the table
        snp, trait, r, t, pv, dfr, qv = (a[:keep] for a in (snp, trait, r, t, pv, dfr, qv))
    n_pairs = int(snp.size)
    m = n_pairs if max_pairs is None else min(n_pairs, max_pairs)
    assoc = dict(snp=snp[:m], trait=trait[:m], r=r[:m], t=t[:m], df=dfr[:m].astype(np.int64), pvalue=pv[:m], qvalue=qv[:m],
                 snp_name=np.asarray(names_x, dtype=object)[snp[:m]], trait_name=np.asarray(names_y, dtype=object)[trait[:m]],
                 n_pairs=n_pairs)
    best_snp, best_r = out["best_snp"], out["best_r"]
    best_p = np.full(best_snp.shape[0], np.nan)
    has = best_snp >= 0
    best_p[has] = t_and_pvalue(best_r[has], df[has])[1]
    return assoc, best_p, snp, pv


def initial_cap_(total):
    """The rows of a scan's first table, when it could return `total` at the most.  INITIAL_CAP is read when called."""
    return int(min(total, INITIAL_CAP))


def complete_table_(scan, cap, count_key):
    """The two-call protocol of every entry that returns a table of selected rows: scan(cap) with the first table's size, and,
    when it counted more rows than that (out[count_key], the full count whatever `cap` is), once more with a table that
    holds them all -- the complete set, whatever order the first call filled its rows in.  Returns the last call's dict."""
    out = scan(cap)
    if out[count_key] > cap:
        out = scan(out[count_key])
    return out


def screen_handle(prep, names_x, names_y, p_value=None, fdr=None, max_pairs=None, dense=False, permutations=None):
    """The screen on a PreparedData as it stands: marginal_screen() without the preparation.  Returns the result dict without
    the rmvd_* fields."""
    from .api import AtlasqtlResult
    p, q = int(prep.p), int(prep.q)
    o = screen_options(p_value, fdr, max_pairs, dense, p, q)
    po = permutation_options(permutations, int(prep.n))
    n_obs = np.sum(~np.isnan(prep.Y), axis=0).astype(np.int64)
    df = n_obs - 2 - int(prep.n_cov)
    cut = r2_cutoff(o["level"], df)
    out = complete_table_(lambda cap: prep.marginal(cut, cap, dense=o["dense"]), initial_cap_(p * q), "n_pairs")
    n_tests = p * q - int(out["n_undefined"])
    assoc, best_p, snp, pv = association_table_(out, df, n_tests, o["mode"], o["level"], o["max_pairs"], names_x, names_y, p)
    n_pairs, best_snp, best_r = assoc["n_pairs"], out["best_snp"], out["best_r"]
    rs = np.asarray(out["rs"], dtype=np.int64)
    if o["mode"] == "fdr":                                    # the Benjamini-Hochberg cut dropped rows the device had counted
        rs = np.bincount(snp, minlength=p).astype(np.int64)
    res = AtlasqtlResult(assoc=assoc, rs_thres=rs, nb_pairwise=n_pairs, best_snp=best_snp, best_r=best_r, best_pvalue=best_p,
                         n_obs=n_obs, df=df, n_undefined=int(out["n_undefined"]), n=int(prep.n), p=p, q=q,
                         threshold=dict(mode=o["mode"], level=o["level"], r2_cut=cut, n_tests=n_tests),
                         names_x=list(names_x), names_y=list(names_y))
    if o["dense"]:
        res["r"] = out["r_dense"]
    if po is not None:
        # the null counts use the cutoff that defined rs_thres: the device's own, or in the fdr mode the one of the largest
        # p-value that the Benjamini-Hochberg cut kept (+inf everywhere: nothing was kept)
        if o["mode"] != "fdr":
            null_cut = cut
        elif n_pairs > 0:
            null_cut = r2_cutoff(float(pv[-1]), df)
        else:
            null_cut = np.full(q, np.inf)
        nul = prep.marginal_permute(null_cut, po["perms"])
        res["permutation"] = dict(n=po["n"], seed=po["seed"], max_r2=nul["max_r2"], hotspot_max=nul["hs_max"], n_selected=nul["n_sel"],
                                  n_undefined=nul["n_undef"], r2_cut=null_cut,
                                  **permutation_summary(nul["max_r2"], nul["hs_max"], nul["n_sel"], best_snp, best_r, rs, n_pairs))
    return res


def on_prepared_(prepare, body, Y, X, device, covariates, ld_prune, transform_y):
    """What marginal_screen() and, through cis.on_cis_windows_, cis_screen(), cis_independent() and cis_finemap() do around
    their work on the handle: prepare (the caller's prepare_data_, passed in so that the name in the caller's module is what
    runs: tests replace cis.prepare_data_, which all three cis entries go through), run body(prep, dat) on the handle, close it
    whatever happens, attach the preparation's rmvd_* fields and n_covariates."""
    dat = prepare(Y, X, 0.1, 1, None, 0, None, None, device=device, covariates=covariates, ld_prune=ld_prune, transform_y=transform_y)
    prep = dat["X"]
    try:
        res = body(prep, dat)
    finally:
        prep.close()
    for key in ("rmvd_cst_x", "rmvd_coll_x", "rmvd_cov_x", "rmvd_ld_x"):
        res[key] = dat[key]
    res["n_covariates"] = dat["n_covariates"]
    return res


def marginal_screen(Y, X, p_value=None, fdr=None, max_pairs=None, covariates=None, ld_prune=None, transform_y=None, dense=False,
                    device=0, permutations=None):
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
      r: with dense=True, the p x q matrix of correlations (NaN where undefined); refused above 2^27 entries.

    permutations (None; a whole number B; {"n": B, "seed": s}; or a B x n integer array of explicit permutations, see
    permutation_options) adds permutation nulls, computed on the GPU from the same handle (aq_prep_marginal_perm): the sample
    rows of the prepared Y are permuted, all traits together and the missing values with them, which keeps the LD among the
    predictors and the correlation among the traits and breaks only the link between the two; every permutation is a whole
    screen, of which only each trait's largest r^2, the largest hotspot size and the number of selected pairs are kept.  The
    result then carries
      permutation: dict(n, seed [None for explicit rows], max_r2 [B x q, -1 where a trait has no defined pair], hotspot_max
        [B], n_selected [B], n_undefined [B], trait_pvalue [q: (1 + #{b: max_r2[b][t] >= best_r[t]^2}) / (B + 1), the p-value
        of the trait's best predictor corrected for the p predictors it was chosen from; NaN where best_snp < 0],
        hotspot_pvalue [p: (1 + #{b: hotspot_max[b] >= rs_thres[s]}) / (B + 1)], expected_null_pairs [mean of n_selected],
        empirical_fdr [min(1, expected_null_pairs / max(1, nb_pairwise))], r2_cut [q: the cutoff of the null counts -- the one
        that defined rs_thres: threshold["r2_cut"], or with fdr= the cutoff of the largest p-value kept, +inf if none was]).
    Without the argument the result has no such key.  With covariates= it is the residualised Y whose rows are permuted (the
    scheme of Freedman and Lane): an approximation, since the residuals are not exchangeable exactly and the predictors were
    residualised on the unpermuted rows; df keeps its covariate count."""
    screen_options(p_value, fdr, max_pairs, dense)             # before the first device call
    permutation_options(permutations)
    def body(prep, dat):
        return screen_handle(prep, dat["names_x"], dat["names_y"], p_value, fdr, max_pairs, dense, permutations)
    return on_prepared_(prepare_data_, body, Y, X, device, covariates, ld_prune, transform_y)
