"""The cis scan: every trait (gene) tested only against the predictors within a window around its own position, the mapping
that FastQTL and tensorQTL compute first, on the GPU from a prepare handle (aq_prep_cis, aq_prep_cis_perm,
csrc/aq_prep_cis.hip).

The GPU does the work of the band -- the correlations of the in-window pairs on the f64 matrix pipe, the selection and each
trait's best cis predictor in registers, and with permutations= each trait's largest in-window r^2 under every permutation of
the sample rows of Y.  The host does O(p + q), O(selected pairs) and O(B q) work, all of it here: the windows from positions
(cis_windows), the user's threshold as a per-trait cutoff on r^2, t, p-value and Benjamini-Hochberg q-value of the rows that
came back, and the permutation p-value of every trait's best predictor with its beta approximation (beta_approximation).

The statistic is the marginal screen's (marginal.py): r over the m_t observed rows of the trait, df_t = m_t - 2 - n_cov, a pair
undefined when the predictor is constant over those rows, Syy_t = 0 or df_t < 1.  A pair outside its trait's window does not
exist: it is neither selected, nor counted as undefined, nor a candidate for the best predictor.

condition_on= turns the scan into the conditional one (aq_prep_cis_cond, csrc/aq_prep_cis_cond.hip): r becomes the partial
correlation given the trait's own conditioning variants, df_t = n - 2 - n_cov - k_eff[t].  The argument is checked by
cis_lists.py; cis_condition.py runs cis_independent()'s forward-backward pass on top of this scan.

interaction= turns the scan into the genotype x environment one (aq_prep_cis_int, csrc/aq_prep_cis_int.hip; tensorQTL's
map_cis(interaction_df=)): r becomes the partial correlation of g o e with the trait given the intercept, the covariates, e
and g, df = n - 4 - n_cov.  The basis of [1, Z, e] the library takes is built on the host, by cis_interaction.py.

What cis_screen(), cis_independent() (cis_condition.py) and cis_finemap() (cis_susie.py) do around their work on the handle has
its one text here, on_cis_windows_: the predictors' coordinates, the preparation, the windows over the kept columns.
"""
from __future__ import annotations

import numpy as np

from .checks import AtlasqtlError, _is_whole
from .cis_interaction import _interaction_vector, interaction_basis, refuse_with_interaction
from .cis_lists import condition_lists, refuse_with_condition
from .marginal import (association_table_, bh_qvalues, complete_table_, initial_cap_, on_prepared_, permutation_options,
                       permutation_trait_pvalue, r2_cutoff, screen_options, t_and_pvalue)
from .plink import PlinkBed
from .prepare import prepare_data_


def cis_windows(snp_chrom, snp_pos, trait_chrom, trait_start, trait_end=None, window=1_000_000):
    """(s_lo, s_hi), int32 each, one entry per trait: the window of trait t is the half-open range s_lo[t] <= s < s_hi[t] of
    predictor indices on the trait's chromosome with trait_start[t] - window <= pos <= trait_end[t] + window (trait_end
    defaults to trait_start).  snp_chrom, snp_pos: one value per predictor, in the predictors' order (the kept columns of a
    prepared matrix).  The predictors of a chromosome must be contiguous and their positions non-decreasing, so that the
    window is one index range; otherwise AtlasqtlError names the first offending column.  A trait on a chromosome without
    predictors gets an empty window (0, 0).  Chromosomes are compared as strings."""
    chrom = np.asarray([str(c) for c in snp_chrom], dtype=object)
    try:
        pos = np.asarray(snp_pos, dtype=np.int64)
        start = np.atleast_1d(np.asarray(trait_start, dtype=np.int64))
        end = start if trait_end is None else np.atleast_1d(np.asarray(trait_end, dtype=np.int64))
    except (TypeError, ValueError) as e:
        raise AtlasqtlError(f"cis_windows: positions must be whole numbers ({e}).") from e
    tchrom = [str(c) for c in np.atleast_1d(np.asarray(trait_chrom, dtype=object))]
    if pos.ndim != 1 or pos.shape != chrom.shape:
        raise AtlasqtlError(f"cis_windows: snp_chrom and snp_pos must hold one value per predictor ({chrom.shape} and {pos.shape}).")
    if start.ndim != 1 or start.shape != end.shape or len(tchrom) != start.size:
        raise AtlasqtlError("cis_windows: trait_chrom, trait_start and trait_end must hold one value per trait.")
    if not _is_whole(window) or int(window) < 0:
        raise AtlasqtlError(f"cis_windows: window must be a whole number >= 0, not {window!r}.")
    if np.any(end < start):
        raise AtlasqtlError(f"cis_windows: trait_end < trait_start for trait {int(np.nonzero(end < start)[0][0])}.")
    window = int(window)
    blocks = {}                                        # chromosome -> (first column, one past its last column)
    p = chrom.size
    j = 0
    while j < p:
        c = chrom[j]
        if c in blocks:
            raise AtlasqtlError(f"cis_windows: the predictors of chromosome {c} are not contiguous: column {j} follows other "
                                "chromosomes. Order the predictors by chromosome and position.")
        k = j + 1
        while k < p and chrom[k] == c:
            if pos[k] < pos[k - 1]:
                raise AtlasqtlError(f"cis_windows: the positions on chromosome {c} decrease at column {k} ({int(pos[k])} after "
                                    f"{int(pos[k - 1])}). Order the predictors by chromosome and position.")
            k += 1
        blocks[c] = (j, k)
        j = k
    q = start.size
    s_lo, s_hi = np.zeros(q, dtype=np.int32), np.zeros(q, dtype=np.int32)
    for t in range(q):
        blk = blocks.get(tchrom[t])
        if blk is None:
            continue
        a, b = blk
        s_lo[t] = a + np.searchsorted(pos[a:b], start[t] - window, side="left")
        s_hi[t] = a + np.searchsorted(pos[a:b], end[t] + window, side="right")
    return s_lo, s_hi


def beta_approximation(max_r2, df, best_pvalue):
    """The beta approximation of the permutation p-value of each trait's best predictor, in the moment-matched form of
    FastQTL's (without its likelihood refinement of the shapes and without its estimate of the degrees of freedom).
    max_r2: B x q, the largest in-window r^2 per permutation (-1: none); df: q; best_pvalue: q, the two-sided Student p-value
    of the observed best predictor.  Per trait: p_b = the two-sided Student p-value of max_r2[b][t] with df_t; m and v their
    mean and (B - 1)-denominator variance; shape1 = m (m (1 - m) / v - 1), shape2 = shape1 (1 / m - 1);
    pvalue = Beta(shape1, shape2).cdf(best_pvalue).  All three NaN where B < 2, v = 0, a shape <= 0, or the trait or a
    permutation of it has no defined pair.  Returns (shape1, shape2, pvalue)."""
    from scipy.stats import beta
    max_r2 = np.asarray(max_r2, dtype=np.float64)
    B, q = max_r2.shape
    df = np.asarray(df, dtype=np.float64)
    best_pvalue = np.asarray(best_pvalue, dtype=np.float64)
    s1, s2, pv = np.full(q, np.nan), np.full(q, np.nan), np.full(q, np.nan)
    if B < 2:
        return s1, s2, pv
    usable = np.all(max_r2 >= 0, axis=0) & (df >= 1) & ~np.isnan(best_pvalue)
    if not usable.any():
        return s1, s2, pv
    pb = t_and_pvalue(np.sqrt(max_r2[:, usable]), np.broadcast_to(df[usable], (B, int(usable.sum()))))[1]
    m, v = pb.mean(axis=0), pb.var(axis=0, ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = m * (m * (1.0 - m) / v - 1.0)
        b = a * (1.0 / m - 1.0)
    ok = (v > 0) & (a > 0) & (b > 0) & np.isfinite(a) & np.isfinite(b)
    idx = np.nonzero(usable)[0][ok]
    s1[idx], s2[idx] = a[ok], b[ok]
    pv[idx] = beta.cdf(best_pvalue[idx], a[ok], b[ok])
    return s1, s2, pv


def cis_permutation_summary(max_r2, best_snp, best_r, best_pvalue, df):
    """What the permutation nulls say about a cis scan, in numpy: dict of
      trait_pvalue[t] = (1 + #{b: max_r2[b][t] >= best_r[t]^2}) / (B + 1), NaN where best_snp[t] < 0;
      beta_shape1, beta_shape2, trait_pvalue_beta: beta_approximation;
      trait_qvalue: Benjamini-Hochberg of trait_pvalue_beta over the traits with a defined pair (NaN elsewhere, and where the
        beta approximation is NaN: those traits are not among the tests)."""
    trait_p = permutation_trait_pvalue(max_r2, best_snp, best_r)
    has = np.asarray(best_snp) >= 0
    s1, s2, pbeta = beta_approximation(max_r2, df, np.where(has, best_pvalue, np.nan))
    qv = np.full(trait_p.shape, np.nan)
    tested = np.nonzero(has & ~np.isnan(pbeta))[0]
    if tested.size:
        order = tested[np.argsort(pbeta[tested], kind="stable")]
        qv[order] = bh_qvalues(pbeta[order], tested.size)
    return dict(trait_pvalue=trait_p, beta_shape1=s1, beta_shape2=s2, trait_pvalue_beta=pbeta, trait_qvalue=qv)


def cis_options(p_value=None, fdr=None, max_pairs=None):
    """The threshold arguments of cis_screen() checked on the host: those of marginal.screen_options, under this function's
    name.  Returns dict(mode, level (None for Bonferroni until the windows are known), max_pairs)."""
    o = screen_options(p_value, fdr, max_pairs, who="cis_screen")
    return dict(mode=o["mode"], level=o["level"], max_pairs=o["max_pairs"])


def cis_handle(prep, names_x, names_y, s_lo, s_hi, p_value=None, fdr=None, max_pairs=None, permutations=None, condition_on=None,
               interaction=None, covariates=None):
    """The cis scan on a PreparedData as it stands, with the windows given as index ranges over its columns: cis_screen()
    without the preparation and without cis_windows.  condition_on: as for cis_screen(), by index into names_x / names_y or by
    name; None takes the unconditional path unchanged.  interaction: as for cis_screen(), with covariates the matrix the data
    were prepared with (None: none); None changes nothing.  Returns the result without the rmvd_* fields."""
    from .api import AtlasqtlResult
    p, q = int(prep.p), int(prep.q)
    o = cis_options(p_value, fdr, max_pairs)
    inter = None
    if interaction is not None:
        refuse_with_interaction(permutations, condition_on, prep.Y)
        inter = interaction_basis(interaction, covariates, int(prep.n), int(prep.n_cov))
    cond = None
    if condition_on is not None:
        cond = condition_lists(condition_on, names_x, names_y)
        refuse_with_condition(permutations, prep.Y)
    po = permutation_options(permutations, int(prep.n))
    s_lo, s_hi = prep._cis_windows_arg(s_lo, s_hi, "cis_screen")
    n_cis = (s_hi.astype(np.int64) - s_lo.astype(np.int64))
    M = int(n_cis.sum())
    level = o["level"] if o["mode"] != "bonferroni" else 0.05 / max(M, 1)
    n_obs = np.sum(~np.isnan(prep.Y), axis=0).astype(np.int64)
    df = n_obs - 2 - int(prep.n_cov)
    if inter is not None:
        def scan(cut, cap):
            return prep.cis_interaction(s_lo, s_hi, inter[0], inter[1], cut, cap)
        df = df - 2                                           # e and g: n - 4 - n_cov
    elif cond is None:
        def scan(cut, cap):
            return prep.cis(s_lo, s_hi, cut, cap)
    else:
        def scan(cut, cap):
            return prep.cis_conditional(s_lo, s_hi, cond, cut, cap)
        # the cutoff on r^2 needs df_t, which needs k_eff: the list's length, unless the device drops a collinear column
        df = df - np.where(n_cis > 0, np.asarray([len(c) for c in cond], dtype=np.int64), 0)
    cut = r2_cutoff(level, df)

    def table(cap):
        nonlocal df, cut
        out = scan(cut, cap)
        if cond is not None and np.any(n_obs - 2 - int(prep.n_cov) - out["k_eff"] != df):   # then once more, with the k_eff reported
            df = n_obs - 2 - int(prep.n_cov) - out["k_eff"]
            cut = r2_cutoff(level, df)
            out = scan(cut, cap)
        return out
    out = complete_table_(table, initial_cap_(M), "n_pairs")   # its second call finds df and cut as the re-cut left them
    n_tests_t = n_cis - out["n_undef"]
    n_tests = int(n_tests_t.sum())
    assoc, best_p, _, _ = association_table_(out, df, n_tests, o["mode"], level, o["max_pairs"], names_x, names_y, p)
    best_snp, best_r = out["best_snp"], out["best_r"]
    res = AtlasqtlResult(assoc=assoc, window=(s_lo, s_hi), n_cis=n_cis, n_tests=n_tests_t, best_snp=best_snp, best_r=best_r,
                         best_pvalue=best_p, n_obs=n_obs, df=df, n_undefined=out["n_undef"], n=int(prep.n), p=p, q=q,
                         threshold=dict(mode=o["mode"], level=level, r2_cut=cut, n_tests=n_tests), plan=out["plan"],
                         names_x=list(names_x), names_y=list(names_y))
    if cond is not None:
        res["condition_on"] = cond
        res["k_eff"] = out["k_eff"]
    if inter is not None:
        res["interaction"] = inter[1]
        res["int_tol"] = out["int_tol"]
        res["best_pvalue_bonferroni"] = np.minimum(1.0, best_p * n_tests_t)
    if po is not None:
        max_r2 = prep.cis_permute(s_lo, s_hi, po["perms"])
        res["permutation"] = dict(n=po["n"], seed=po["seed"], max_r2=max_r2,
                                  **cis_permutation_summary(max_r2, best_snp, best_r, best_p, df))
    return res


def _snp_coordinates(X, snp_chrom, snp_pos, who):
    """snp_chrom and snp_pos as given, or the chrom and pos of a PlinkBed X where they are not."""
    if isinstance(X, PlinkBed):
        snp_chrom = X.chrom if snp_chrom is None else snp_chrom
        snp_pos = X.pos if snp_pos is None else snp_pos
    if snp_chrom is None or snp_pos is None:
        raise AtlasqtlError(f"{who}: snp_chrom and snp_pos are required unless X is a PlinkBed.")
    return snp_chrom, snp_pos


def _per_predictor(X, snp_chrom, snp_pos):
    """snp_chrom and snp_pos as arrays with one value per predictor given."""
    p_given = X.shape[1] if hasattr(X, "shape") else np.asarray(X).shape[1]
    out = []
    for name, values in (("snp_chrom", snp_chrom), ("snp_pos", snp_pos)):
        a = np.asarray(values)
        if a.ndim != 1 or a.shape[0] != int(p_given):
            raise AtlasqtlError(f"cis_screen: {name} must hold one value per predictor given ({int(p_given)}), not {a.shape}.")
        out.append(a)
    return out


def _windows_of_kept(prep, dat, snp_chrom, snp_pos, trait_chrom, trait_start, trait_end, window, who):
    """cis_windows over the columns the preparation kept, once the traits are known to be as many as the prepared ones."""
    kept = ~np.asarray(dat["bool_rmvd_x"], dtype=bool)
    if len(np.atleast_1d(trait_start)) != int(prep.q):
        raise AtlasqtlError(f"{who}: trait_chrom, trait_start and trait_end must hold one value per trait ({int(prep.q)}).")
    return cis_windows(snp_chrom[kept], snp_pos[kept], trait_chrom, trait_start, trait_end, window)


def on_cis_windows_(who, run, Y, X, coordinates, device, covariates, ld_prune, transform_y, window_first=True, covariates_from=None):
    """What cis_screen(), cis_independent() and cis_finemap() do around their work on the handle, after the checks of their own
    arguments.  coordinates: (trait_chrom, trait_start, trait_end, window, snp_chrom, snp_pos) as the entry got them.  Before
    the first device call: `window` (with window_first; cis_independent() leaves it to cis_windows, on the prepared handle),
    then snp_chrom and snp_pos, from a PlinkBed X where they are not given, one value per predictor given.  Then
    marginal.on_prepared_ with this module's prepare_data_, and on the handle run(prep, dat, s_lo, s_hi) with the windows over
    the columns the preparation kept.  covariates_from: a function of no arguments that returns the covariates in the place of
    `covariates`, called once the coordinates have passed: cis_finemap()'s genotype PCs are device work."""
    trait_chrom, trait_start, trait_end, window, snp_chrom, snp_pos = coordinates
    if window_first and (not _is_whole(window) or int(window) < 0):
        raise AtlasqtlError(f"{who}: window must be a whole number >= 0, not {window!r}.")
    snp_chrom, snp_pos = _per_predictor(X, *_snp_coordinates(X, snp_chrom, snp_pos, who))
    if covariates_from is not None:
        covariates = covariates_from()

    def body(prep, dat):
        return run(prep, dat, *_windows_of_kept(prep, dat, snp_chrom, snp_pos, trait_chrom, trait_start, trait_end, window, who))
    return on_prepared_(prepare_data_, body, Y, X, device, covariates, ld_prune, transform_y)


def cis_screen(Y, X, trait_chrom, trait_start, trait_end=None, window=1_000_000, snp_chrom=None, snp_pos=None, p_value=None,
               fdr=None, max_pairs=None, permutations=None, covariates=None, ld_prune=None, transform_y=None, device=0,
               condition_on=None, interaction=None):
    """Every trait of Y tested against the predictors of X within `window` base pairs of it, on the GPU: cis-QTL mapping.

    X and Y are prepared exactly as marginal_screen() prepares them.  trait_chrom, trait_start, trait_end (default:
    trait_start): one value per trait; the window of trait t is the kept predictors on its chromosome with trait_start -
    window <= pos <= trait_end + window (cis_windows, which needs the predictors ordered by chromosome and position).
    snp_chrom, snp_pos: one value per predictor GIVEN, cut to the kept columns as names_x is; they default to the chrom and
    pos of a plink.PlinkBed.  For every pair inside a window: the Pearson correlation r over the trait's observed rows,
    t = r sqrt(df / (1 - r^2)) with df = m_t - 2 - d and the two-sided p-value of Student's t, as in marginal_screen().  A pair
    outside its trait's window does not exist.

    Selection as in marginal_screen(), with M = the number of in-window pairs in the place of p q: p_value=c keeps p <= c;
    fdr=a keeps the Benjamini-Hochberg set at level a over the M - (undefined in-window pairs) tests; neither means
    Bonferroni, p_value = 0.05 / M.  The table is ordered by (p-value, -|t|, position snp + p trait); max_pairs cuts it.

    Returns an AtlasqtlResult with
      assoc: the columns of marginal_screen()'s;
      per trait: window (s_lo, s_hi: index ranges into names_x), n_cis (predictors in the window), n_tests (defined pairs
        among them), n_undefined, best_snp, best_r, best_pvalue (the in-window predictor of largest r^2, the lowest index on
        a tie; -1 / NaN / NaN where the window is empty or holds no defined pair), n_obs, df;
      threshold: dict(mode, level, r2_cut, n_tests); plan: the dict of aq_cis_plan, whose window_pairs / staged_pairs is the
        fill of the band; names_x, names_y, n, p, q, n_covariates and rmvd_cst_x, rmvd_coll_x, rmvd_cov_x, rmvd_ld_x.

    permutations (as in marginal_screen(): None, B, {"n": B, "seed": s} or a B x n array) adds the permutation null of every
    trait's best cis predictor, computed on the GPU over the same windows (aq_prep_cis_perm): the result then carries
      permutation: dict(n, seed, max_r2 [B x q: the largest in-window r^2 per permutation, -1 where none is defined],
        trait_pvalue [(1 + #{b: max_r2[b][t] >= best_r[t]^2}) / (B + 1); NaN where best_snp < 0],
        beta_shape1, beta_shape2, trait_pvalue_beta [the beta approximation of that p-value in the moment-matched form of
        FastQTL's, without its likelihood refinement and its estimate of the degrees of freedom: with p_b the two-sided
        Student p-value of max_r2[b][t] at df_t, m and v the mean and the (B - 1)-denominator variance of the p_b,
        shape1 = m (m (1 - m) / v - 1), shape2 = shape1 (1 / m - 1), trait_pvalue_beta = Beta(shape1, shape2).cdf(best_pvalue);
        NaN where B < 2, v = 0 or a shape <= 0],
        trait_qvalue [Benjamini-Hochberg of trait_pvalue_beta over the traits with a defined pair: the eGenes are
        trait_qvalue <= level]).
    With covariates= the residualised Y is permuted, as marginal_screen() describes.

    condition_on (None; a dict trait -> variants; or a list of q lists; traits and variants by index into names_y / names_x,
    the kept columns, or by name) makes the scan conditional: trait t is tested after its own at most 4 variants, inside its
    window or not, have been regressed out of it and of every predictor (aq_prep_cis_cond).  r is then the partial
    correlation, df = n - 2 - d - k_eff, and a pair is also undefined when the predictor is collinear with the list (each
    listed variant itself is) or the list explains the whole trait.  The result then also carries condition_on (the q index
    lists) and k_eff (per trait, the listed variants not collinear with the earlier ones; 0 where the window is empty).
    Complete Y only, and not together with permutations=: both are refused before anything is computed.  A window of
    [0, p) for every trait is the conditional trans scan.  Without the argument the call is the unconditional scan above.

    interaction (None, or one vector e of n values: cell-type fraction, sex, age, treatment; one term per call, as in
    tensorQTL's map_cis(interaction_df=)) makes the scan the genotype x environment one (aq_prep_cis_int): every in-window pair
    is tested for the coefficient of g o e in y ~ 1 + covariates + e + g + g o e, g the prepared predictor.  r in assoc is then
    the partial correlation of g o e with the trait given the other four, t = r sqrt(df / (1 - r^2)) that coefficient's OLS t,
    and df = n - 4 - d.  A pair is undefined when g is collinear with [1, covariates, e] (a variant that equals e), when g o e
    is collinear with [1, covariates, e, g] (a variant that is zero outside one level of a binary e), or when these explain
    the whole trait.  The result then also carries interaction (e centred), int_tol (per kept predictor, the share of g o e
    that [1, covariates, e, g] leave; NaN where the predictor is undefined) and best_pvalue_bonferroni = min(1, best_pvalue
    n_tests), the correction of each trait's best interaction over its window.  e must be finite, not constant, and outside
    span[1, covariates].  Complete Y only, and not together with permutations= or condition_on=: all refused before anything
    is computed.  A window of [0, p) for every trait is the genome-wide interaction scan.  Without the argument the call is
    the scan above, unchanged."""
    cis_options(p_value, fdr, max_pairs)                       # before the first device call
    permutation_options(permutations)
    if condition_on is not None:
        refuse_with_condition(permutations, None if isinstance(Y, str) else Y)
    if interaction is not None:
        Yh = None if isinstance(Y, str) else Y
        refuse_with_interaction(permutations, condition_on, Yh)
        if Yh is not None and np.ndim(Yh) == 2 and (covariates is None or np.ndim(covariates) == 2):
            interaction_basis(interaction, covariates, np.shape(Yh)[0], 0 if covariates is None else np.shape(covariates)[1])
        else:
            _interaction_vector(interaction)

    def run(prep, dat, s_lo, s_hi):
        return cis_handle(prep, dat["names_x"], dat["names_y"], s_lo, s_hi, p_value, fdr, max_pairs, permutations, condition_on,
                          interaction, covariates if interaction is not None else None)
    return on_cis_windows_("cis_screen", run, Y, X, (trait_chrom, trait_start, trait_end, window, snp_chrom, snp_pos), device,
                           covariates, ld_prune, transform_y)
