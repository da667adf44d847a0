"""cis_finemap(): the step after the cis scans, per trait SuSiE over its window, fitted by IBSS on the GPU for all traits in
lockstep (aq_prep_cis_finemap, csrc/aq_prep_cis_finemap.hip), which returns the alphas above a per-trait threshold
(row_threshold) as rows.  The host part is here: the arguments (finemap_options, _traits_arg), the credible sets from the rows
(credible_sets_), their purity through aq_prep_set_purity, the PIPs and the two tables.  (The module is not named after its
entry, so that atlasqtl_amd.cis_finemap is the function and nothing else.)
"""
from __future__ import annotations

import numpy as np

from .checks import AtlasqtlError, _is_real, _is_whole, name_or_index_
from .cis import on_cis_windows_
from .marginal import complete_table_, initial_cap_
from .prepare import covariates_with_genotype_pcs

PURITY_MAX = 100                                    # members of a set that aq_prep_set_purity looks at (csrc/aq_finemap_plan.h)


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
    not_one = "cis_finemap: traits= must name a trait by its name or its index in [0, {n}), not {v!r}."
    trait = name_or_index_(list(names_y), "cis_finemap: traits= names the trait {v!r}, which is not among the traits.", not_one, not_one)
    out = np.zeros(q, dtype=bool)
    for v in np.atleast_1d(np.asarray(traits, dtype=object)):
        out[trait(v)] = True
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
    if o["max_rows"] is None:
        out = complete_table_(lambda cap: prep.cis_finemap(s_lo, s_hi, cap=cap, **kw), initial_cap_(o["L"] * n_win), "n_rows")
    else:
        out = prep.cis_finemap(s_lo, s_hi, cap=o["max_rows"], **kw)
        if out["n_rows"] > o["max_rows"]:
            raise AtlasqtlError(f"cis_finemap: {out['n_rows']} rows exceed max_rows = {o['max_rows']}; the credible sets need all of "
                                "them. Raise max_rows or alpha_min, or fit fewer traits.")
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

    def run(prep, dat, s_lo, s_hi):
        return cis_finemap_handle(prep, dat["names_x"], dat["names_y"], s_lo, s_hi, L, coverage, min_abs_corr, tol, max_iter,
                                  scaled_prior_variance, traits, alpha_min, max_rows, dense)
    with_pcs = None if genotype_pcs is None else (lambda: covariates_with_genotype_pcs(Y, X, covariates, genotype_pcs, device)[0])
    return on_cis_windows_("cis_finemap", run, Y, X, (trait_chrom, trait_start, trait_end, window, snp_chrom, snp_pos), device,
                           covariates, ld_prune, transform_y, covariates_from=with_pcs)
