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
correlation given the trait's own conditioning variants, df_t = n - 2 - n_cov - k_eff[t].  cis_independent() runs the
forward-backward conditional pass of QTLtools and tensorQTL's map_independent on top of it: the loop itself is
independent_signals_, which takes the scan as a callable.

interaction= turns the scan into the genotype x environment one (aq_prep_cis_int, csrc/aq_prep_cis_int.hip; tensorQTL's
map_cis(interaction_df=)): r becomes the partial correlation of g o e with the trait given the intercept, the covariates, e
and g, df = n - 4 - n_cov.  The basis of [1, Z, e] the library takes is built here, on the host (interaction_basis).

cis_finemap() is the step after them: per trait SuSiE over its window, fitted by IBSS on the GPU for all traits in lockstep
(aq_prep_cis_finemap, csrc/aq_prep_cis_finemap.hip), which returns the alphas above a per-trait threshold as rows.  The host
part is here: the credible sets from the rows (credible_sets_), their purity through aq_prep_set_purity, the PIPs.
"""
from __future__ import annotations

import numpy as np

from .checks import AtlasqtlError, _is_real, _is_whole
from .marginal import (INITIAL_CAP, association_table_, bh_qvalues, on_prepared_, permutation_options, permutation_trait_pvalue,
                       r2_cutoff, screen_options, t_and_pvalue)
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
    try:
        o = screen_options(p_value, fdr, max_pairs)
    except AtlasqtlError as e:
        raise AtlasqtlError(str(e).replace("marginal_screen:", "cis_screen:")) from None
    return dict(mode=o["mode"], level=o["level"], max_pairs=o["max_pairs"])


def condition_lists(condition_on, names_x, names_y):
    """The condition_on argument of cis_screen() checked on the host: q lists of indices into names_x.  condition_on: a dict
    trait -> variants (a trait is an index into names_y or a name in it; traits not named get an empty list), or a list of q
    lists.  A variant is an index into names_x or a name in it; a single variant may stand without a list.  At most 4
    distinct variants per trait."""
    names_x, names_y = list(names_x), list(names_y)
    q = len(names_y)
    by_name = {}                                       # "trait" / "variant" -> name -> first index, built when a name is met

    def lookup(v, names, what):
        if isinstance(v, (str, np.str_)):
            if what not in by_name:
                by_name[what] = {str(nm): i for i, nm in reversed(list(enumerate(names)))}
            if str(v) not in by_name[what]:
                raise AtlasqtlError(f"cis_screen: condition_on names the {what} {v!r}, which is not among the {what}s kept.")
            return by_name[what][str(v)]
        if not _is_whole(v) or isinstance(v, (bool, np.bool_)):
            raise AtlasqtlError(f"cis_screen: condition_on must name a {what} by its name or its index, not {v!r}.")
        if not 0 <= int(v) < len(names):
            raise AtlasqtlError(f"cis_screen: condition_on has the {what} index {int(v)} outside [0, {len(names)}).")
        return int(v)

    if isinstance(condition_on, dict):
        items = [[] for _ in range(q)]
        for key, vs in condition_on.items():
            t = lookup(key, names_y, "trait")
            if items[t]:
                raise AtlasqtlError(f"cis_screen: condition_on names trait {t} twice.")
            items[t] = vs
    else:
        try:
            items = list(condition_on)
        except TypeError:
            items = None
        if items is None or len(items) != q or isinstance(condition_on, str):
            raise AtlasqtlError(f"cis_screen: condition_on must be a dict trait -> variants or a list of one list per trait ({q}).")
    out = []
    for t, vs in enumerate(items):
        if isinstance(vs, (str, np.str_)) or np.ndim(vs) == 0:
            vs = [vs]
        lst = [lookup(v, names_x, "variant") for v in vs]
        if len(lst) > 4:
            raise AtlasqtlError(f"cis_screen: trait {t} conditions on {len(lst)} variants; at most 4 are supported.")
        if len(set(lst)) != len(lst):
            raise AtlasqtlError(f"cis_screen: condition_on names a variant of trait {t} more than once.")
        out.append(lst)
    return out


def _refuse_with_condition(permutations, Y):
    if permutations is not None:
        raise AtlasqtlError("cis_screen: condition_on= together with permutations= is not supported: permutation nulls are "
                            "computed for the unconditional scan only. Run the two separately, or cis_independent().")
    if Y is not None and np.isnan(np.asarray(Y, dtype=np.float64)).any():
        raise AtlasqtlError("cis_screen: condition_on= needs complete Y; Y has missing values.")


COV_TOL = 1e-10                                        # AQ_COV_TOL of csrc/aq_cov_kernels.h: the rule of aq_cov_basis


def _interaction_vector(e, n=None):
    """The interaction variable as one finite, non-constant float64 vector (of n values, where n is given)."""
    try:
        ev = np.asarray(e, dtype=np.float64)
    except (TypeError, ValueError):
        ev = None
    if ev is None or ev.ndim != 1 or ev.size < 1 or (n is not None and ev.shape[0] != int(n)):
        want = "one value per sample" if n is None else f"one value per sample ({int(n)})"
        raise AtlasqtlError(f"cis_screen: interaction must be one numeric vector with {want}, not "
                            f"{'that' if ev is None else ev.shape}. One interaction term per call.")
    if not np.all(np.isfinite(ev)):
        raise AtlasqtlError("cis_screen: interaction must be finite without missing value.")
    if ev.max() == ev.min():
        raise AtlasqtlError("cis_screen: interaction is constant: it cannot be told from the intercept.")
    return ev


def interaction_basis(e, covariates, n, n_cov):
    """(B, m) for the interaction scan, on the host: m = e centred (n values) and B, nb x n with nb = n_cov + 2, the orthonormal
    rows spanning [1, Z, e] in this order, by Gram-Schmidt with one re-orthogonalisation and long-double dot products.  A
    column is dropped when what is left of it after the columns before it has a squared norm <= 1e-10 times its own (the
    rule of aq_cov_basis).  Refused with AtlasqtlError, before anything is computed on a device: an e of the wrong length, a
    non-finite e, a constant e, an e inside span[1, Z], and covariates whose rank (the columns not dropped) is not n_cov, the
    number the handle was prepared with."""
    n, n_cov = int(n), int(n_cov)
    ev = _interaction_vector(e, n)
    if covariates is None:
        Z = np.zeros((n, 0))
    else:
        try:
            Z = np.asarray(covariates, dtype=np.float64)
        except (TypeError, ValueError):
            Z = None
        if Z is None or Z.ndim != 2 or Z.shape[0] != n or not np.all(np.isfinite(Z)):
            raise AtlasqtlError(f"cis_screen: covariates must be a finite numeric matrix with one row per sample ({n}).")
    LD = np.longdouble
    rows = [np.full(n, 1.0 / np.sqrt(n))]

    def remainder(col):
        v = np.array(col, dtype=np.float64)
        own = float(np.dot(v.astype(LD), v.astype(LD)))
        for _ in range(2):
            for b in rows:
                v = v - b * float(np.dot(b.astype(LD), v.astype(LD)))
        rem = float(np.dot(v.astype(LD), v.astype(LD)))
        return v, rem, own

    for l in range(Z.shape[1]):
        v, rem, own = remainder(Z[:, l])
        if rem > COV_TOL * own:
            rows.append(v / np.sqrt(rem))
    rank = len(rows) - 1
    if rank != n_cov:
        raise AtlasqtlError(f"cis_screen: the covariates given with interaction= have rank {rank}, but the data were prepared with "
                            f"{n_cov} covariates. Pass the covariates the data were prepared with.")
    m = ev - ev.mean()
    v, rem, own = remainder(m)
    if not rem > COV_TOL * own:
        raise AtlasqtlError("cis_screen: interaction lies in the span of the intercept and the covariates: its effect cannot be "
                            "told from theirs.")
    rows.append(v / np.sqrt(rem))
    return np.ascontiguousarray(np.stack(rows, axis=0)), m


def _refuse_with_interaction(permutations, condition_on, Y):
    if permutations is not None:
        raise AtlasqtlError("cis_screen: interaction= together with permutations= is not supported: permutation nulls are "
                            "computed for the plain scan only. best_pvalue_bonferroni corrects each trait's best interaction.")
    if condition_on is not None:
        raise AtlasqtlError("cis_screen: interaction= together with condition_on= is not supported. Run the two separately.")
    if Y is not None and np.isnan(np.asarray(Y, dtype=np.float64)).any():
        raise AtlasqtlError("cis_screen: interaction= needs complete Y; Y has missing values.")


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
        _refuse_with_interaction(permutations, condition_on, prep.Y)
        inter = interaction_basis(interaction, covariates, int(prep.n), int(prep.n_cov))
    cond = None
    if condition_on is not None:
        cond = condition_lists(condition_on, names_x, names_y)
        _refuse_with_condition(permutations, prep.Y)
    po = permutation_options(permutations, int(prep.n))
    s_lo, s_hi = prep._cis_windows_arg(s_lo, s_hi, "cis_screen")
    n_cis = (s_hi.astype(np.int64) - s_lo.astype(np.int64))
    M = int(n_cis.sum())
    level = o["level"] if o["mode"] != "bonferroni" else 0.05 / max(M, 1)
    n_obs = np.sum(~np.isnan(prep.Y), axis=0).astype(np.int64)
    df = n_obs - 2 - int(prep.n_cov)
    cap = int(min(M, INITIAL_CAP))
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
    out = scan(cut, cap)
    if cond is not None and np.any(n_obs - 2 - int(prep.n_cov) - out["k_eff"] != df):   # then once more, with the k_eff reported
        df = n_obs - 2 - int(prep.n_cov) - out["k_eff"]
        cut = r2_cutoff(level, df)
        out = scan(cut, cap)
    if out["n_pairs"] > cap:                                  # the complete set, whatever order the first call filled its rows in
        out = scan(cut, out["n_pairs"])
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
        _refuse_with_condition(permutations, None if isinstance(Y, str) else Y)
    if interaction is not None:
        Yh = None if isinstance(Y, str) else Y
        _refuse_with_interaction(permutations, condition_on, Yh)
        if Yh is not None and np.ndim(Yh) == 2 and (covariates is None or np.ndim(covariates) == 2):
            interaction_basis(interaction, covariates, np.shape(Yh)[0], 0 if covariates is None else np.shape(covariates)[1])
        else:
            _interaction_vector(interaction)
    if not _is_whole(window) or int(window) < 0:
        raise AtlasqtlError(f"cis_screen: window must be a whole number >= 0, not {window!r}.")
    snp_chrom, snp_pos = _per_predictor(X, *_snp_coordinates(X, snp_chrom, snp_pos, "cis_screen"))

    def body(prep, dat):
        s_lo, s_hi = _windows_of_kept(prep, dat, snp_chrom, snp_pos, trait_chrom, trait_start, trait_end, window, "cis_screen")
        return cis_handle(prep, dat["names_x"], dat["names_y"], s_lo, s_hi, p_value, fdr, max_pairs, permutations, condition_on,
                          interaction, covariates if interaction is not None else None)
    return on_prepared_(prepare_data_, body, Y, X, device, covariates, ld_prune, transform_y)


MAX_SIGNALS = 5                                        # one more than the variants a trait can be conditioned on


def _check_max_signals(max_signals):
    if not _is_whole(max_signals) or not 1 <= int(max_signals) <= MAX_SIGNALS:
        raise AtlasqtlError(f"cis_independent: max_signals must be a whole number from 1 to {MAX_SIGNALS}, not {max_signals!r}.")


def independent_signals_(scan, best_snp, best_pvalue, threshold, max_signals=MAX_SIGNALS, best_r=None, df=None):
    """The forward-backward conditional pass of QTLtools (and tensorQTL's map_independent) over all traits together, on the
    host: the scans themselves are `scan`, so the loop runs against the GPU or against numpy alike.

    scan(cond, active) -> dict(best_snp, best_pvalue[, best_r, df]), q entries each: the conditional scan in which trait t is
    conditioned on the variants cond[t]; only the entries of the traits with active[t] are read (the others may be scanned
    with an empty window, so that they cost nothing), best_snp < 0 meaning that no pair is defined.
    best_snp, best_pvalue[, best_r, df]: the unconditional scan's.  threshold: per trait, the nominal p-value a signal must
    reach; NaN for a trait that is no eGene.  max_signals: 1 ... 5.

    Signal 1 of a trait with a threshold is its best_snp.  Forward rounds j = 1 ... max_signals - 1: one scan covers all
    traits still active, each conditioned on its own j signals; a trait whose conditional best has p <= threshold gains that
    variant and stays active, the others leave; the rounds stop when no trait gains one.  Backward rounds i = 0, 1, ... for the
    traits with m >= 2 signals: conditioned on the forward set without signal i -- the forward sets stay fixed throughout --
    the best variant replaces signal i's lead if its p <= threshold, otherwise the signal is dropped.  A trait with one signal
    keeps it as it is.
    Returns dict(forward: per trait the forward variants; signals: per trait a list of dict(rank [1-based position in the
    forward set], snp, forward_snp, pvalue, r, df [NaN / -1 where the scan does not give them]); n_signals)."""
    _check_max_signals(max_signals)
    best_snp = np.asarray(best_snp)
    best_pvalue = np.asarray(best_pvalue, dtype=np.float64)
    threshold = np.asarray(threshold, dtype=np.float64)
    q = best_snp.shape[0]

    def row(out, t):
        r = out.get("best_r")
        d = out.get("df")
        return dict(snp=int(out["best_snp"][t]), pvalue=float(out["best_pvalue"][t]), r=float(r[t]) if r is not None else np.nan,
                    df=int(d[t]) if d is not None else -1)

    active = ~np.isnan(threshold) & (best_snp >= 0)
    forward = [[int(best_snp[t])] if active[t] else [] for t in range(q)]
    for _ in range(1, int(max_signals)):
        if not active.any():
            break
        out = scan([list(forward[t]) if active[t] else [] for t in range(q)], active.copy())
        for t in np.nonzero(active)[0]:
            if out["best_snp"][t] >= 0 and out["best_pvalue"][t] <= threshold[t]:
                forward[t].append(int(out["best_snp"][t]))
            else:
                active[t] = False
    primary = dict(best_snp=best_snp, best_pvalue=best_pvalue, best_r=best_r, df=df)
    signals = [[dict(rank=1, forward_snp=f[0], **row(primary, t))] if len(f) == 1 else [] for t, f in enumerate(forward)]
    for i in range(max((len(f) for f in forward), default=0)):
        active = np.asarray([len(f) >= 2 and len(f) > i for f in forward], dtype=bool)
        if not active.any():
            break
        out = scan([f[:i] + f[i + 1:] if active[t] else [] for t, f in enumerate(forward)], active.copy())
        for t in np.nonzero(active)[0]:
            if out["best_snp"][t] >= 0 and out["best_pvalue"][t] <= threshold[t]:
                signals[t].append(dict(rank=i + 1, forward_snp=forward[t][i], **row(out, t)))
    return dict(forward=forward, signals=signals, n_signals=np.asarray([len(s) for s in signals], dtype=np.int64))


def cis_independent_handle(prep, names_x, names_y, s_lo, s_hi, fdr=0.05, permutations=1000, max_signals=MAX_SIGNALS):
    """cis_independent() on a PreparedData as it stands, with the windows given as index ranges over its columns.  Returns
    the result without the rmvd_* fields."""
    from scipy.stats import beta
    from .api import AtlasqtlResult
    if not _is_real(fdr, 0.0, 1.0, lo_open=True):
        raise AtlasqtlError(f"cis_independent: fdr must be a number in (0, 1], not {fdr!r}.")
    if permutations is None:
        raise AtlasqtlError("cis_independent: permutations are required: they decide the eGenes and each gene's threshold.")
    _check_max_signals(max_signals)
    if np.isnan(prep.Y).any():
        raise AtlasqtlError("cis_independent: the conditional scans need complete Y; Y has missing values.")
    primary = cis_handle(prep, names_x, names_y, s_lo, s_hi, permutations=permutations)
    s_lo, s_hi = primary["window"]
    q = int(prep.q)
    perm = primary["permutation"]
    pbeta = perm["trait_pvalue_beta"]
    with np.errstate(invalid="ignore"):
        egene = perm["trait_qvalue"] <= float(fdr)
    threshold = np.full(q, np.nan)
    if egene.any():
        ok = ~np.isnan(perm["beta_shape1"])
        threshold[ok] = beta.ppf(float(np.max(pbeta[egene])), perm["beta_shape1"][ok], perm["beta_shape2"][ok])
    base_df = primary["df"]
    no_cut = np.full(q, np.inf)

    def scan(cond, active):
        out = prep.cis_conditional(np.where(active, s_lo, 0), np.where(active, s_hi, 0), cond, no_cut, 0)
        d = base_df - out["k_eff"]
        pv = np.full(q, np.nan)
        has = out["best_snp"] >= 0
        pv[has] = t_and_pvalue(out["best_r"][has], d[has])[1]
        return dict(best_snp=out["best_snp"], best_pvalue=pv, best_r=out["best_r"], df=d)

    loop = independent_signals_(scan, primary["best_snp"], primary["best_pvalue"], np.where(egene, threshold, np.nan), max_signals,
                                best_r=primary["best_r"], df=base_df)
    rows = [(t, s) for t in range(q) for s in loop["signals"][t]]
    snp = np.asarray([s["snp"] for _, s in rows], dtype=np.int32)
    trait = np.asarray([t for t, _ in rows], dtype=np.int32)
    r = np.asarray([s["r"] for _, s in rows], dtype=np.float64)
    dfs = np.asarray([s["df"] for _, s in rows], dtype=np.int64)
    signals = dict(trait=trait, rank=np.asarray([s["rank"] for _, s in rows], dtype=np.int32), snp=snp,
                   forward_snp=np.asarray([s["forward_snp"] for _, s in rows], dtype=np.int32), r=r,
                   t=t_and_pvalue(r, dfs)[0] if rows else np.zeros(0), df=dfs,
                   pvalue=np.asarray([s["pvalue"] for _, s in rows], dtype=np.float64),
                   snp_name=np.asarray(names_x, dtype=object)[snp], trait_name=np.asarray(names_y, dtype=object)[trait])
    return AtlasqtlResult(signals=signals, n_signals=loop["n_signals"], forward=loop["forward"], threshold=threshold, egene=egene,
                          fdr=float(fdr), max_signals=int(max_signals), primary=primary, n=int(prep.n), p=int(prep.p), q=q,
                          names_x=list(names_x), names_y=list(names_y))


def cis_independent(Y, X, trait_chrom, trait_start, trait_end=None, window=1_000_000, snp_chrom=None, snp_pos=None, fdr=0.05,
                    permutations=1000, max_signals=MAX_SIGNALS, covariates=None, ld_prune=None, transform_y=None, device=0):
    """The independent cis signals of every eGene, by the forward-backward conditional pass of QTLtools (tensorQTL's
    map_independent), on one prepared handle on the GPU.  Arguments as for cis_screen(); complete Y only.

    (a) The unconditional scan with permutations (cis_screen(permutations=...)).  The eGenes are the traits with
        trait_qvalue <= fdr; p* is the largest trait_pvalue_beta among them; each trait's nominal threshold is
        Beta(beta_shape1_t, beta_shape2_t).ppf(p*).  Signal 1 of an eGene is its best_snp.
    (b), (c) independent_signals_ with the conditional scan (cis_screen(condition_on=...)): every round is ONE scan over all
        genes still active, each conditioned on its own variants, the others with an empty window; a conditional best is
        compared at its reduced df = n - 2 - d - k_eff.
    Returns an AtlasqtlResult with
      signals: one row per signal kept, ordered by (trait, rank): trait, rank (1-based position in the forward set), snp (the
        lead after the backward pass), forward_snp (the variant the forward pass found), r, t, df, pvalue (conditional on the
        trait's other forward variants; unconditional for a trait with one signal), snp_name, trait_name;
      n_signals: per trait; forward: per trait the forward variants; threshold: per trait (NaN where the beta approximation
      is NaN, or there is no eGene); egene; primary: the result of (a); names_x, names_y, n, p, q, n_covariates, rmvd_*."""
    snp_chrom, snp_pos = _snp_coordinates(X, snp_chrom, snp_pos, "cis_independent")
    _check_max_signals(max_signals)
    if permutations is None:
        raise AtlasqtlError("cis_independent: permutations are required: they decide the eGenes and each gene's threshold.")
    permutation_options(permutations)
    snp_chrom, snp_pos = _per_predictor(X, snp_chrom, snp_pos)

    def body(prep, dat):
        s_lo, s_hi = _windows_of_kept(prep, dat, snp_chrom, snp_pos, trait_chrom, trait_start, trait_end, window, "cis_independent")
        return cis_independent_handle(prep, dat["names_x"], dat["names_y"], s_lo, s_hi, fdr, permutations, max_signals)
    return on_prepared_(prepare_data_, body, Y, X, device, covariates, ld_prune, transform_y)


PURITY_MAX = 100                                       # members of a set that aq_prep_set_purity looks at (csrc/aq_finemap_plan.h)


def row_threshold(alpha_min, coverage, n_weighted):
    """thr_t of aq_prep_cis_finemap: rows with alpha below min(alpha_min, 0.1 (1 - coverage) / P_t) are not returned, P_t the
    predictors of the trait's window with prior weight.  An effect then loses less than 0.1 (1 - coverage) of its mass, all
    of it in the tail of the ordered alphas, so the credible set built from the rows is the one built from the full vector."""
    P = np.maximum(np.asarray(n_weighted, dtype=np.float64), 1.0)
    return np.minimum(float(alpha_min), 0.1 * (1.0 - float(coverage)) / P)


def credible_sets_(rows, V, coverage=0.95):
    """The credible sets of a fine-mapping, pure host logic.  rows: dict(snp, trait, effect, alpha[, mu]) -- for every (trait,
    effect) all predictors whose alpha matters (cis_finemap's rows, or a full vector); V: q x L, the prior variances.
    Per (trait, effect) with V > 0: the alphas in descending order (ties to the lower predictor index), and the smallest prefix
    whose mass reaches `coverage`: 1 + the number of partial sums below it, susieR's rule.  An effect with V = 0 gives none.
    Of the sets of one trait that hold the same predictors only the one of the lowest effect stays, as in susieR.
    Returns a list of dict(trait, effect, snp [in the order of the prefix], alpha, mu [NaN without rows['mu']], mass),
    ordered by (trait, effect)."""
    snp, trait, effect = (np.asarray(rows[k], dtype=np.int64) for k in ("snp", "trait", "effect"))
    alpha = np.asarray(rows["alpha"], dtype=np.float64)
    mu = np.asarray(rows["mu"], dtype=np.float64) if rows.get("mu") is not None else np.full(alpha.shape, np.nan)
    V = np.asarray(V, dtype=np.float64)
    order = np.lexsort((snp, -alpha, effect, trait))         # by trait, effect, alpha descending, predictor ascending
    snp, trait, effect, alpha, mu = snp[order], trait[order], effect[order], alpha[order], mu[order]
    key = trait * (V.shape[1] if V.ndim == 2 else 1) + effect
    starts = np.nonzero(np.r_[True, key[1:] != key[:-1]])[0] if key.size else np.zeros(0, dtype=np.int64)
    ends = np.r_[starts[1:], key.size]
    sets, seen = [], set()
    for a, b in zip(starts, ends):
        t, l = int(trait[a]), int(effect[a])
        if not V[t, l] > 0:
            continue
        csum = np.cumsum(alpha[a:b])
        k = min(int(np.sum(csum < coverage)) + 1, b - a)
        members = (t, tuple(sorted(int(s) for s in snp[a:a + k])))
        if members in seen:
            continue
        seen.add(members)
        sets.append(dict(trait=t, effect=l, snp=snp[a:a + k].astype(np.int32), alpha=alpha[a:a + k], mu=mu[a:a + k],
                         mass=float(csum[k - 1])))
    return sets


def finemap_options(L=10, coverage=0.95, min_abs_corr=0.5, tol=1e-3, max_iter=100, scaled_prior_variance=0.2, alpha_min=1e-4,
                    max_rows=None):
    """The arguments of cis_finemap() checked on the host, before the first device call."""
    if not _is_whole(L) or not 1 <= int(L) <= 16:
        raise AtlasqtlError(f"cis_finemap: L must be a whole number from 1 to 16, not {L!r}.")
    if not _is_real(coverage, 0.0, 1.0, lo_open=True) or float(coverage) >= 1.0:
        raise AtlasqtlError(f"cis_finemap: coverage must be a number in (0, 1), not {coverage!r}.")
    if not _is_real(min_abs_corr, 0.0, 1.0):
        raise AtlasqtlError(f"cis_finemap: min_abs_corr must be a number in [0, 1], not {min_abs_corr!r}.")
    if not _is_real(tol, 0.0, np.inf) or not np.isfinite(float(tol)):
        raise AtlasqtlError(f"cis_finemap: tol must be a finite number >= 0, not {tol!r}.")
    if not _is_whole(max_iter) or int(max_iter) < 1:
        raise AtlasqtlError(f"cis_finemap: max_iter must be a whole number >= 1, not {max_iter!r}.")
    if not _is_real(scaled_prior_variance, 0.0, np.inf, lo_open=True) or not np.isfinite(float(scaled_prior_variance)):
        raise AtlasqtlError(f"cis_finemap: scaled_prior_variance must be a finite number > 0, not {scaled_prior_variance!r}.")
    if not _is_real(alpha_min, 0.0, 1.0):
        raise AtlasqtlError(f"cis_finemap: alpha_min must be a number in [0, 1], not {alpha_min!r}.")
    if max_rows is not None and (not _is_whole(max_rows) or int(max_rows) < 1):
        raise AtlasqtlError(f"cis_finemap: max_rows must be None or a whole number >= 1, not {max_rows!r}.")
    return dict(L=int(L), coverage=float(coverage), min_abs_corr=float(min_abs_corr), tol=float(tol), max_iter=int(max_iter),
                scaled_prior_variance=float(scaled_prior_variance), alpha_min=float(alpha_min),
                max_rows=None if max_rows is None else int(max_rows))


def _traits_arg(traits, names_y):
    """traits= of cis_finemap() as q booleans: None (all), q booleans, or a list of indices into names_y / names in it."""
    q = len(names_y)
    if traits is None:
        return None
    a = np.asarray(traits)
    if a.dtype == bool:
        if a.shape != (q,):
            raise AtlasqtlError(f"cis_finemap: a boolean traits= must hold one flag per trait ({q}), not {a.shape}.")
        return a.copy()
    by_name = {str(nm): i for i, nm in reversed(list(enumerate(names_y)))}
    out = np.zeros(q, dtype=bool)
    for v in np.atleast_1d(np.asarray(traits, dtype=object)):
        if isinstance(v, (str, np.str_)):
            if str(v) not in by_name:
                raise AtlasqtlError(f"cis_finemap: traits= names the trait {v!r}, which is not among the traits.")
            out[by_name[str(v)]] = True
        elif _is_whole(v) and not isinstance(v, (bool, np.bool_)) and 0 <= int(v) < q:
            out[int(v)] = True
        else:
            raise AtlasqtlError(f"cis_finemap: traits= must name a trait by its name or its index in [0, {q}), not {v!r}.")
    return out


def cis_finemap_handle(prep, names_x, names_y, s_lo, s_hi, L=10, coverage=0.95, min_abs_corr=0.5, tol=1e-3, max_iter=100,
                       scaled_prior_variance=0.2, traits=None, alpha_min=1e-4, max_rows=None, dense=False):
    """cis_finemap() on a PreparedData as it stands, with the windows given as index ranges over its columns.  Returns the
    result without the rmvd_* fields."""
    from .api import AtlasqtlResult
    o = finemap_options(L, coverage, min_abs_corr, tol, max_iter, scaled_prior_variance, alpha_min, max_rows)
    active = _traits_arg(traits, names_y)
    s_lo, s_hi = prep._cis_windows_arg(s_lo, s_hi, "cis_finemap")
    p, q = int(prep.p), int(prep.q)
    kw = dict(L=o["L"], tol=o["tol"], max_iter=o["max_iter"], scaled_prior_variance=o["scaled_prior_variance"], coverage=o["coverage"],
              alpha_min=o["alpha_min"], active=active, dense=dense)
    n_win = int((s_hi.astype(np.int64) - s_lo.astype(np.int64)).sum())
    cap = int(min(o["L"] * n_win, INITIAL_CAP)) if o["max_rows"] is None else o["max_rows"]
    out = prep.cis_finemap(s_lo, s_hi, cap=cap, **kw)
    if out["n_rows"] > cap and o["max_rows"] is None:          # the complete set, whatever order the first call filled its rows in
        out = prep.cis_finemap(s_lo, s_hi, cap=out["n_rows"], **kw)
    if out["n_rows"] > cap and o["max_rows"] is not None:
        raise AtlasqtlError(f"cis_finemap: {out['n_rows']} rows exceed max_rows = {cap}; the credible sets need all of them. Raise "
                            "max_rows or alpha_min, or fit fewer traits.")
    names_x, names_y = np.asarray(names_x, dtype=object), np.asarray(names_y, dtype=object)
    # pip = 1 - prod_l (1 - alpha_ls) over the rows of (snp, trait)
    pos = out["snp"].astype(np.int64) + p * out["trait"].astype(np.int64)
    upos, inv = np.unique(pos, return_inverse=True)
    log1m = np.zeros(upos.size)
    with np.errstate(divide="ignore"):                         # alpha = 1: pip = 1
        np.add.at(log1m, inv, np.log1p(-out["alpha"]))
    pip = -np.expm1(log1m)
    pip_table = dict(snp=(upos % p).astype(np.int32), trait=(upos // p).astype(np.int32), pip=pip)
    pip_table["snp_name"], pip_table["trait_name"] = names_x[pip_table["snp"]], names_y[pip_table["trait"]]
    pip_of = dict(zip(upos.tolist(), pip.tolist()))
    sets = credible_sets_(out, out["V"], o["coverage"])
    pure = []
    if sets:
        top = [cs["snp"][:PURITY_MAX] for cs in sets]          # in descending alpha: the top members of a larger set
        pmin, pmean = prep.set_purity(top)
        for cs, a, b in zip(sets, pmin, pmean):
            cs["purity_min"], cs["purity_mean"] = float(a), float(b)
            if a >= o["min_abs_corr"]:
                pure.append(cs)
    cols = dict(trait=[], cs=[], snp=[], alpha=[], pip=[], beta=[], cs_size=[], purity_min=[], purity_mean=[], lbf=[])
    for cs in pure:
        k = cs["snp"].size
        cols["trait"] += [cs["trait"]] * k
        cols["cs"] += [cs["effect"]] * k
        cols["snp"] += [int(s) for s in cs["snp"]]
        cols["alpha"] += list(cs["alpha"])
        cols["pip"] += [pip_of[int(s) + p * cs["trait"]] for s in cs["snp"]]
        cols["beta"] += list(cs["alpha"] * cs["mu"])
        cols["cs_size"] += [k] * k
        cols["purity_min"] += [cs["purity_min"]] * k
        cols["purity_mean"] += [cs["purity_mean"]] * k
        cols["lbf"] += [float(out["lbf"][cs["trait"], cs["effect"]])] * k
    table = {key: np.asarray(v, dtype=np.int32 if key in ("trait", "cs", "snp", "cs_size") else np.float64) for key, v in cols.items()}
    table["snp_name"], table["trait_name"] = names_x[table["snp"]], names_y[table["trait"]]
    n_cs = np.zeros(q, dtype=np.int64)
    for cs in pure:
        n_cs[cs["trait"]] += 1
    res = AtlasqtlResult(cs=table, pip=pip_table, n_impure=len(sets) - len(pure), sigma2=out["sigma2"], prior_variance=out["V"],
                         elbo=out["elbo"], n_iter=out["n_iter"], converged=out["converged"].astype(bool), n_cs=n_cs, lbf=out["lbf"],
                         n_undefined=out["n_undef"], window=(s_lo, s_hi), traits=active, plan=out["plan"], coverage=o["coverage"],
                         min_abs_corr=o["min_abs_corr"], L=o["L"], n=int(prep.n), p=p, q=q, names_x=list(names_x), names_y=list(names_y))
    if dense:
        res["alpha"], res["mu"] = out["alpha_dense"], out["mu_dense"]
    return res


def cis_finemap(Y, X, trait_chrom, trait_start, trait_end=None, window=1_000_000, snp_chrom=None, snp_pos=None, L=10, coverage=0.95,
                min_abs_corr=0.5, tol=1e-3, max_iter=100, scaled_prior_variance=0.2, traits=None, alpha_min=1e-4, max_rows=None,
                covariates=None, ld_prune=None, transform_y=None, genotype_pcs=None, dense=False, device=0):
    """Statistical fine-mapping of every trait's cis window by SuSiE (the sum of single effects; tensorQTL's susie.map) on one
    prepared handle on the GPU: the credible sets of variants that carry the trait's independent signals.

    X, Y, the windows and covariates=, ld_prune=, transform_y= as for cis_screen(); genotype_pcs= as for atlasqtl(), appended to
    the covariates; complete Y only.  The model is susieR's susie(standardize = FALSE, intercept = FALSE) on the prepared
    matrices, with L single effects, the prior variances of the effects estimated by EM from scaled_prior_variance y'y / (n - 1)
    and the residual variance estimated; IBSS stops for a trait when its ELBO gains less than tol (tol = 0: after max_iter
    iterations), all traits stepping together on the GPU (aq_prep_cis_finemap).  traits: the traits to fit -- the eGenes of a
    cis_screen(), for example -- as q booleans or a list of indices or names; None fits all.

    Credible sets (credible_sets_): per trait and effect with prior variance > 0, the smallest set of variants, taken in
    descending alpha, whose alphas sum to `coverage`; duplicates of one trait are dropped; a set whose smallest |correlation|
    between two of its variants (of the 100 of largest alpha, for a larger set) is below min_abs_corr is left out.  The GPU
    returns the alphas >= min(alpha_min, 0.1 (1 - coverage) / P_t), P_t the variants of the window: the sets are those of the
    full vectors.  max_rows sizes their table up front, and more rows than that are an error; without it the fit is run again
    with a table of the size the first run counted, when 65 536 rows do not hold them.

    Returns an AtlasqtlResult with
      cs: one row per member of a credible set, ordered by (trait, cs, alpha descending): trait, cs (the effect), snp, alpha,
        pip, beta = alpha mu, cs_size, purity_min, purity_mean, lbf (of the effect), snp_name, trait_name;
      n_impure: the sets left out for their purity; n_cs: per trait, the sets kept;
      pip: snp, trait, pip = 1 - prod_l (1 - alpha_ls) over the effects with prior variance > 0, from the rows returned: a lower
        bound, within L times the row threshold of the full value; variants without a row are not listed;
      sigma2, prior_variance [q x L], lbf [q x L], elbo [max_iter x q], n_iter, converged, n_undefined (variants of the window
        without variance, which get no weight), window, plan (the dict of aq_finemap_plan); alpha, mu [q x L x p] with dense=True;
      names_x, names_y, n, p, q, n_covariates, rmvd_*.
    A trait that is not fitted (traits=), or whose window is empty, has NaN in sigma2, prior_variance, lbf and n_iter = 0."""
    finemap_options(L, coverage, min_abs_corr, tol, max_iter, scaled_prior_variance, alpha_min, max_rows)   # before the first device call
    if not _is_whole(window) or int(window) < 0:
        raise AtlasqtlError(f"cis_finemap: window must be a whole number >= 0, not {window!r}.")
    snp_chrom, snp_pos = _per_predictor(X, *_snp_coordinates(X, snp_chrom, snp_pos, "cis_finemap"))
    if genotype_pcs is not None:
        from .prepare import covariates_with_genotype_pcs
        covariates = covariates_with_genotype_pcs(Y, X, covariates, genotype_pcs, device)[0]

    def body(prep, dat):
        s_lo, s_hi = _windows_of_kept(prep, dat, snp_chrom, snp_pos, trait_chrom, trait_start, trait_end, window, "cis_finemap")
        return cis_finemap_handle(prep, dat["names_x"], dat["names_y"], s_lo, s_hi, L, coverage, min_abs_corr, tol, max_iter,
                                  scaled_prior_variance, traits, alpha_min, max_rows, dense)
    return on_prepared_(prepare_data_, body, Y, X, device, covariates, ld_prune, transform_y)
