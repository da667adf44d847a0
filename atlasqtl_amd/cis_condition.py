"""cis_independent(): the independent cis signals of every eGene, by the forward-backward conditional pass of QTLtools and
tensorQTL's map_independent on top of the conditional cis scan (cis.cis_handle with permutations for the eGenes and their
thresholds, PreparedData.cis_conditional for every round).  The loop itself is independent_signals_, pure host logic that
takes the scan as a callable; cis_independent_handle gives it the GPU's and makes the table of signals.
"""
from __future__ import annotations

import numpy as np

from .checks import AtlasqtlError, _is_real, _is_whole, refuse_
from .cis import cis_handle, on_cis_windows_
from .marginal import permutation_options, t_and_pvalue

MAX_SIGNALS = 5                                        # one more than the variants a trait can be conditioned on


def _check_max_signals(max_signals):
    if not _is_whole(max_signals) or not 1 <= int(max_signals) <= MAX_SIGNALS:
        raise AtlasqtlError(f"cis_independent: max_signals must be a whole number from 1 to {MAX_SIGNALS}, not {max_signals!r}.")


def _require_permutations(permutations):
    if permutations is None:
        raise AtlasqtlError("cis_independent: permutations are required: they decide the eGenes and each gene's threshold.")


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
    _require_permutations(permutations)
    _check_max_signals(max_signals)
    refuse_("cis_independent", complete_y=(prep.Y, "the conditional scans need complete Y; Y has missing values."))
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
    _check_max_signals(max_signals)
    _require_permutations(permutations)
    permutation_options(permutations)

    def run(prep, dat, s_lo, s_hi):
        return cis_independent_handle(prep, dat["names_x"], dat["names_y"], s_lo, s_hi, fdr, permutations, max_signals)
    return on_cis_windows_("cis_independent", run, Y, X, (trait_chrom, trait_start, trait_end, window, snp_chrom, snp_pos), device,
                           covariates, ld_prune, transform_y, window_first=False)
