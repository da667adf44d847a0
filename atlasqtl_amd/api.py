"""User-level entry point: ``atlasqtl()`` with the reference's argument surface
(R/atlasqtl.R:179-184) and return fields (R/atlasqtl.R:293-316,
R/atlasqtl_global_local_core.R:426-428).  Pre-processing and hyper-parameter /
initialisation handling run on the host (checks.py, prepare.py, hyper_init.py); the
variational loop runs on the GPU through core.atlasqtl_global_local_core_.
"""
from __future__ import annotations

import sys
import warnings

import numpy as np

from . import prediction
from .core import atlasqtl_global_local_core_
from .postproc import hotspot_sizes, six_numbers_host_, sparse_output_options, value_summary
from .hyper_init import prepare_list_hyper_, prepare_list_init_
from .marginal import screen_arg, screen_handle
from .checks import check_annealing_, check_positive_, check_vector_, check_verbose_
from .prepare import covariates_with_genotype_pcs, prepare_data_, transform_y_options


class AtlasqtlResult(dict):
    """The reference returns an S3 list of class "atlasqtl"; this is a dict with attribute access."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def add_collinear_back_(beta_vb, gam_vb, theta_vb, initial_colnames_X, rmvd_coll_x, names_x):
    """R/utils.R:671-733: re-insert the rows of predictors removed as duplicates, copying the
    estimates of the column each one duplicated, in the pre-removal column order."""
    pos = {nm: i for i, nm in enumerate(names_x)}
    rows = [pos[nm] if nm in pos else pos[rmvd_coll_x[nm]] for nm in initial_colnames_X]
    return beta_vb[rows, :], gam_vb[rows, :], theta_vb[rows]


def add_collinear_back_pairs_(assoc, rs_thres, theta_vb, initial_colnames_X, rmvd_coll_x, names_x, max_pairs=None):
    """add_collinear_back_ for the sparse result (PPI mode): every removed duplicate column gets the rows of the column it
    duplicated.  `assoc` is the complete table of the fitted (de-duplicated) matrix; the returned table is the one of the
    dense add_collinear_back_ output: snp in its row numbering (initial_colnames_X order), rows ordered by (-ppi, position
    in the expanded matrix), fdr = cumsum(1 - ppi) / (1:N) along it (copies share their PPI, so a threshold on the PPI
    keeps or drops them together and the expanded table is again a prefix of the expanded matrix's order); max_pairs cuts
    it afterwards.  rs_thres and theta_vb are expanded like the dense vectors.  Returns (assoc, rs_thres, theta_vb)."""
    if len(assoc["snp"]) != assoc["n_pairs"]:
        raise ValueError("add_collinear_back_pairs_ needs the complete table (max_pairs cuts the expanded table)")
    pos = {nm: i for i, nm in enumerate(names_x)}
    rows = np.array([pos[nm] if nm in pos else pos[rmvd_coll_x[nm]] for nm in initial_colnames_X], dtype=np.int64)
    p_new = rows.size
    by_kept = np.argsort(rows, kind="stable")                       # expanded rows grouped by the fitted row they copy
    first = np.searchsorted(rows[by_kept], assoc["snp"], side="left")
    reps = np.searchsorted(rows[by_kept], assoc["snp"], side="right") - first
    src = np.repeat(np.arange(len(assoc["snp"])), reps)             # table row each expanded row comes from
    within = np.arange(src.size) - np.repeat(np.cumsum(reps) - reps, reps)
    snp = by_kept[first[src] + within].astype(np.int32)
    trait, ppi = assoc["trait"][src], assoc["ppi"][src]
    order = np.lexsort((snp.astype(np.int64) + p_new * trait.astype(np.int64), -ppi))
    m = order.size if max_pairs is None else min(order.size, int(max_pairs))
    out = dict(snp=snp[order][:m], trait=trait[order][:m], ppi=ppi[order][:m], beta=assoc["beta"][src][order][:m],
               fdr=(np.cumsum(1 - ppi[order]) / np.arange(1, order.size + 1))[:m], n_pairs=int(order.size))
    return out, np.asarray(rs_thres)[rows], np.asarray(theta_vb)[rows]


def warn_tied_traits_(n_obs, n_tied, names_y):
    """One warning that names the responses (the first ten) more than half of whose observed values are tied."""
    bad = np.where(2 * np.asarray(n_tied, dtype=np.int64) > np.asarray(n_obs, dtype=np.int64))[0]
    if bad.size:
        shown = ", ".join(str(names_y[k]) for k in bad[:10]) + (", ..." if bad.size > 10 else "")
        warnings.warn(f"transform_y: more than half of the observed values are tied in {bad.size} response(s) ({shown}); ranks do not "
                      "make such a response normal.")


def atlasqtl(Y, X, p0, anneal=(1, 2, 10), tol=0.1, maxit=1000, user_seed=None, verbose=1, list_hyper=None,
             list_init=None, save_hyper=False, save_init=False, full_output=False, thinned_elbo_eval=True,
             checkpoint_path=None, trace_path=None, add_collinear_back=False, device=0, device_init=False,
             sparse_output=None, covariates=None, ld_prune=None, genotype_pcs=None, transform_y=None, marginal_screen=None,
             predict=None, fitted=False, keep_predictor=False):
    """R/atlasqtl.R:179-322.

    X: a float64 matrix, int8 dosages, or a plink.PlinkBed (a PLINK 1 .bed / .bim / .fam fileset, unpacked on the GPU): the
    predictors are then named by the .bim's variant IDs and the result carries `genotype_counts` (4 x p int32: homozygous
    A1, heterozygous, homozygous A2, missing, per variant given, over the samples used).

    sparse_output = {"thres": 0.5, "fdr_adjust": False, "max_pairs": None} (missing keys take these values): instead of
    the p x q gam_vb / beta_vb, return what summary.atlasqtl reads off them (R/summarise_output.R:99-106) -- `assoc`, the
    table of pairs with gam_vb > thres (or assign_bFDR(gam_vb) < thres) with snp / trait indices and names, ppi, beta and
    fdr; `rs_thres` and `nb_pairwise` -- so that the matrices never leave the GPU.  With "summary": True also
    `value_summary`, the quartiles and means of all p q PPIs and effect sizes that summary() prints (computed on the GPU,
    core.VbRun.value_summary).  None: the dense result.

    covariates: an n x d matrix (age, sex, genotype PCs, batch factors ...; 1 <= d <= 96, finite, rows as in Y) that is
    regressed, with an intercept, out of every predictor and every response on the GPU before the fit (prepare_on_device);
    the fit is the fit to those residuals.  The result then carries `n_covariates`, `rmvd_cov_x` (names of the predictors
    that the covariates explain entirely, or None; they are among `rmvd_cst_x`) and `cov_r2_x` (per predictor given, the
    share of its variance that the covariates explain).  For a response with missing values the predictors are adjusted
    over all samples, not over its observed ones, and the model is not told about the d + 1 degrees of freedom removed.

    ld_prune = {"r2": 0.8, "window": 500, "window_bp": None, "groups": None, "positions": None} (missing keys take these
    values): prune the predictors for linkage disequilibrium on the GPU before the fit, on the standardised columns the fit
    sees (after constant and duplicate removal, with covariates on the residuals).  Going through the predictors in order, one
    is removed when a kept predictor at most `window` columns before it, in the same group (one label per predictor given; a
    PlinkBed's chromosomes by default) and, with window_bp, at most that many base pairs away (`positions`; a PlinkBed's by
    default) has a squared correlation above r2 with it.  The result then carries `rmvd_ld_x` (removed name -> the kept
    predictor that tags it, or None) and `ld_r2_x` (per predictor given, its r^2 with that predictor, NaN otherwise);
    `names_x` is the pruned list, and a list_hyper / list_init of the original p is cut accordingly.  Not with
    add_collinear_back=True.

    genotype_pcs = k or {"k": k, "ld_prune": None}: take the k leading genotype principal components of X on the GPU
    (genotype_pcs(): the n x n relationship matrix of the standardised, unresidualised predictors, its eigenvectors on the
    host) and append them to `covariates`.  1 <= k <= min(n - 2, 96 - d) with d user covariates; n <= 10240 -- or, with
    {"k": k, "solver": "subspace"} and optionally "oversample", "tol", "max_iter", "seed" (genotype_pcs()), by subspace
    iteration on the GPU without the n x n matrix, for every n a fit takes.  The option's own
    "ld_prune" (the dict ld_prune= takes) thins only the matrix the PCs are taken from, the usual prune-then-PCA; the fit's
    predictors are governed by ld_prune= alone.  X is prepared twice.  The result then carries `genotype_pcs` (n x k),
    `pc_eigenvalues`, `pc_var_explained`, `pc_solver`, `pc_iterations`, `pc_converged`, and `n_covariates` counts d + k.

    transform_y = "int" or {"method": "int", "offset": 0.375}: the rank-based inverse normal transform of every response on the
    GPU before anything else is done to Y (rank_normalize(): Phi^-1((r - offset) / (m + 1 - 2 offset)) over the m observed values
    of the response, ties given their average rank, missing values left missing) -- what expression, protein and metabolite
    levels go through before a QTL analysis; with covariates the transformed response is residualised.  The genotype PCs
    never see Y.  The result then carries `transform_y` (the options used), `y_n_obs` and `y_n_tied` (per response, its observed
    values and those among them that share their value with another one).  A response more than half of whose observed
    values are tied is not made normal by ranks: one warning names such responses (the first ten).

    marginal_screen = True or {"p_value": ..., "fdr": ..., "max_pairs": ...} (at most one of the first two; True or neither:
    Bonferroni, 0.05 / (p q)): before the fit, test every predictor against every response on its own on the GPU
    (marginal_screen()), on the very handle the fit is about to use, so X is prepared once.  The result then carries
    `marginal`: the result of marginal_screen() -- its `assoc` table, `rs_thres` (the marginal hotspot sizes, to hold the
    fit's against), `best_snp` ... -- without the rmvd_* fields, which this result has itself.

    predict = X_new (float64 or int8 dosages, n_new rows, the columns of X in its original numbering, finite): apply the fitted
    model to new genotypes on the GPU before the run's state is released, so also with sparse_output.  The removed columns
    (constant, duplicate, LD-pruned) are dropped and the others standardised by the fit's own means and standard deviations.  The
    result then carries `predicted` (n_new x q): the genetic component of the responses on the scale of the prepared Y
    (centred, and transformed if transform_y= was used).  Not with covariates= or genotype_pcs=; not a PlinkBed.
    fitted=True: the result carries `X_beta_vb` (n x q), the same product for the samples of the fit, on the prepared X.
    keep_predictor=True: the result carries `predictor` = {"kept_x", "x_center", "x_scale", "p_given"} -- the kept columns
    in the original numbering and their standardisation -- with which predict(res, X_new) applies a dense result later.
    Without these three arguments the result has none of these keys."""
    X_new = None
    if predict is not None:
        prediction.refuse_with_covariates("predict=", covariates, genotype_pcs)
        X_new = prediction.check_x_new(predict, (X.shape if hasattr(X, "shape") else np.shape(X))[1], "predict")
    if keep_predictor:
        prediction.refuse_with_covariates("keep_predictor=True", covariates, genotype_pcs)
    if ld_prune is not None and add_collinear_back:
        raise ValueError("add_collinear_back=True cannot be combined with ld_prune: a predictor removed for LD is not a copy of "
                         "the predictor that tags it, and the add-back maps assume copies (they would hand it the tag's "
                         "estimates).  Read the tags off rmvd_ld_x, or fit without pruning.")
    sparse = None if sparse_output is None else sparse_output_options(sparse_output)
    if sparse is not None and add_collinear_back and sparse["fdr_adjust"]:
        raise ValueError("add_collinear_back=True cannot be combined with sparse_output in FDR mode: the re-inserted copies "
                         "would take part in the FDR ranking, which changes the selected set and cannot be derived from the "
                         "table.  Use the PPI mode (fdr_adjust=False) or the dense output.")
    if sparse is not None and add_collinear_back and sparse["summary"]:
        raise ValueError('add_collinear_back=True cannot be combined with sparse_output={"summary": True}: the re-inserted '
                         "copies would enter the quartiles of gam_vb and beta_vb, which the six numbers of the fitted matrix "
                         "cannot reproduce.  Use the dense output.")
    check_verbose_(verbose)
    check_annealing_(anneal)
    yt_opts = transform_y_options(transform_y)                              # before the first device call
    screen = screen_arg(marginal_screen)
    pcs = None
    if genotype_pcs is not None:
        covariates, pcs = covariates_with_genotype_pcs(Y, X, covariates, genotype_pcs, device)
    if yt_opts is None:
        dat = prepare_data_(Y, X, tol, maxit, user_seed, verbose, checkpoint_path, trace_path, covariates=covariates,
                            ld_prune=ld_prune)
    else:
        dat = prepare_data_(Y, X, tol, maxit, user_seed, verbose, checkpoint_path, trace_path, covariates=covariates,
                            ld_prune=ld_prune, transform_y=yt_opts)
        warn_tied_traits_(dat["y_n_obs"], dat["y_n_tied"], dat["names_y"])
    bool_rmvd_x = dat["bool_rmvd_x"]
    Xs, Yc = dat["X"], dat["Y"]
    n, p = Xs.shape
    q = Yc.shape[1]
    shr_fac_inv = q                                                         # :218
    if list_hyper is None or list_init is None:
        check_vector_(p0, "p0", size=2)
        check_positive_(p0, "p0")
    elif p0 is not None:
        warnings.warn("Provided argument p0 not used, as both list_hyper and list_init were provided.")
    list_hyper = prepare_list_hyper_(list_hyper, Yc, p, p0, bool_rmvd_x)
    list_init = prepare_list_init_(list_init, Yc, p, p0, bool_rmvd_x, shr_fac_inv, user_seed, device_init=device_init)
    if verbose != 0:
        print("**************************************************** \n"
              f"Number of samples: {n}\nNumber of (non-redundant) candidate predictors: {p}\n"
              f"Number of responses: {q}\n**************************************************** \n")
    marginal = None if screen is None else screen_handle(Xs, dat["names_x"], dat["names_y"], **screen)
    df = 1                                                                  # :272  (hs <- TRUE, debug <- TRUE :267-268)
    new_args = {}                                                           # only what was asked for reaches the core
    predictor = None
    if X_new is not None or keep_predictor:
        predictor = prediction.predictor_of(bool_rmvd_x, *Xs.x_moments(len(bool_rmvd_x)))
    if X_new is not None:
        new_args["predict"] = {"X": X_new[:, predictor["kept_x"]], "center": predictor["x_center"], "scale": predictor["x_scale"],
                               "checked": True}
    if fitted:
        new_args["fitted"] = True
    res = atlasqtl_global_local_core_(Yc, Xs, shr_fac_inv, None if anneal is None else tuple(anneal), df, tol,
                                      maxit, verbose, list_hyper, list_init, checkpoint_path, trace_path,
                                      full_output, thinned_elbo_eval, debug=True, device=device,
                                      # the collinear copies are added to the complete table; max_pairs cuts afterwards
                                      sparse_output=None if sparse is None else
                                      {**sparse, "max_pairs": None if add_collinear_back else sparse["max_pairs"]}, **new_args)
    res = AtlasqtlResult(res)
    if keep_predictor:
        res["predictor"] = predictor
    res["p0"] = p0
    res["rmvd_cst_x"] = dat["rmvd_cst_x"]
    res["rmvd_coll_x"] = dat["rmvd_coll_x"]
    res["names_x"], res["names_y"] = dat["names_x"], dat["names_y"]
    if marginal is not None:
        res["marginal"] = marginal
    if dat["genotype_counts"] is not None:                # X = PlinkBed: 4 x p (hom A1, het, hom A2, missing), before removals
        res["genotype_counts"] = dat["genotype_counts"]
    if covariates is not None:
        res["n_covariates"], res["rmvd_cov_x"], res["cov_r2_x"] = dat["n_covariates"], dat["rmvd_cov_x"], dat["cov_r2_x"]
    if pcs is not None:
        res["genotype_pcs"], res["pc_eigenvalues"], res["pc_var_explained"] = pcs["pcs"], pcs["eigenvalues"], pcs["var_explained"]
        res["pc_solver"], res["pc_iterations"], res["pc_converged"] = pcs["solver"], pcs["iterations"], pcs["converged"]
    if ld_prune is not None:
        res["rmvd_ld_x"], res["ld_r2_x"] = dat["rmvd_ld_x"], dat["ld_r2_x"]
    if yt_opts is not None:
        res["transform_y"], res["y_n_obs"], res["y_n_tied"] = dict(yt_opts), dat["y_n_obs"], dat["y_n_tied"]
    names_snp = dat["names_x"]
    if sparse is not None:
        if sparse["summary"]:
            res["sparse_output"] = dict(sparse)
        if add_collinear_back:
            if dat["rmvd_coll_x"]:
                res["assoc"], res["rs_thres"], res["theta_vb"] = add_collinear_back_pairs_(
                    res["assoc"], res["rs_thres"], res["theta_vb"], dat["initial_colnames_X"], dat["rmvd_coll_x"],
                    dat["names_x"], sparse["max_pairs"])
                res["nb_pairwise"] = res["assoc"]["n_pairs"]
                names_snp = dat["initial_colnames_X"]
                res["names_x_all"] = list(names_snp)              # the rows of rs_thres / theta_vb, for summary()
            elif sparse["max_pairs"] is not None:
                res["assoc"] = {k: (v if k == "n_pairs" else v[:int(sparse["max_pairs"])]) for k, v in res["assoc"].items()}
        res["assoc"]["snp_name"] = np.asarray(names_snp, dtype=object)[res["assoc"]["snp"]]
        res["assoc"]["trait_name"] = np.asarray(dat["names_y"], dtype=object)[res["assoc"]["trait"]]
    elif add_collinear_back and dat["rmvd_coll_x"]:
        res["beta_vb"], res["gam_vb"], res["theta_vb"] = add_collinear_back_(
            res["beta_vb"], res["gam_vb"], res["theta_vb"], dat["initial_colnames_X"], dat["rmvd_coll_x"],
            dat["names_x"])
        res["names_x_all"] = list(dat["initial_colnames_X"])      # the rows of gam_vb / theta_vb, for summary()
    if save_hyper:
        res["list_hyper"] = list_hyper
    if save_init:
        res["list_init"] = list_init
    return res


# ---- S3 methods of the reference: print.atlasqtl and summary.atlasqtl (R/summarise_output.R) ----
def _rchar(x):
    """as.character of a number as paste0 writes it: 15 significant digits, integers without a decimal point."""
    if isinstance(x, (bool, np.bool_)):
        return "TRUE" if x else "FALSE"
    if isinstance(x, (int, np.integer)):
        return str(int(x))
    return f"{float(x):.15g}"


def _rformat(x, digits):
    """format(x, digits = d) of one number: d significant digits, but never fewer than the integer part has."""
    x = float(x)
    if np.isfinite(x) and abs(x) >= 10 ** digits:
        return f"{x:.0f}"
    return f"{x:.{digits}g}"


_SIX = (("min", "Min."), ("q1", "1st Qu."), ("median", "Median"), ("mean", "Mean"), ("q3", "3rd Qu."), ("max", "Max."))


def _print_six(six, file):
    """print(summary(x)): R's labels over the six numbers, four significant digits (summary.default's default)."""
    vals = [("NaN" if lab == "Mean" else "NA") if six is None else _rformat(six[k], 4) for k, lab in _SIX]
    width = [max(len(lab), len(v)) + 1 for (_, lab), v in zip(_SIX, vals)]
    print("".join(lab.rjust(w) for (_, lab), w in zip(_SIX, width)) + " ", file=file)
    print("".join(v.rjust(w) for v, w in zip(vals, width)) + " ", file=file)


def _only_six(d):
    return {k: d[k] for k, _ in _SIX}


def print_atlasqtl(x, file=None):
    """print.atlasqtl, R/summarise_output.R:14-59: basic information about the run."""
    file = sys.stdout if file is None else file
    if x["converged"]:
        file.write("****************************************************** \n"
                   f"Successful convergence after {_rchar(x['it'])} iterations, using a\n"
                   f"tolerance of {_rchar(x['tol'])} on the absolute changes in the ELBO.\n"
                   "****************************************************** \n\n")
        anneal = x.get("anneal")
        if anneal is not None:
            anneal_type = {1: "Geometric", 2: "Harmonic", 3: "Linear"}[int(anneal[0])]
            default = tuple(float(a) for a in anneal) == (1.0, 2.0, 10.0)
            file.write(f"{anneal_type} annealing on the inverse temperature was\n"
                       f"applied for the first {_rchar(anneal[2])} iterations, with initial\n"
                       f"temperature of {_rchar(anneal[1])}" + (" (default).\n\n" if default else ".\n\n"))
        p0 = x.get("p0")
        file.write(f"Number of samples: {_rchar(x['n'])};\n"
                   f"Number of (non-redundant) candidate predictors: {_rchar(x['p'])};\n"
                   f"Number of responses: {_rchar(x['q'])};\n"
                   "Prior expectation for the number of predictors\n"
                   f"associated with each response: {'NA' if p0 is None else _rchar(p0[0])} (sd: "
                   f"{'NA' if p0 is None else _rformat(np.sqrt(p0[1]), 2)}).\n\n")
        file.write("The posterior quantities inferred by ATLASQTL can\n"
                   "be accessed as list elements from the `atlasqtl` S3\n"
                   "object, and a summary can obtained using the\n"
                   "`summary` function.\n\n")
    else:
        file.write("************************************************ \n"
                   f"Unsuccessful convergence after {_rchar(x['maxit'])} iterations. \n"
                   "Difference between last two consecutive values\n"
                   f"of the ELBO: {_rformat(x['diff_lb'], 3)}.\n\n"
                   "Try increasing:\n"
                   "- the maximum number of iterations (maxit) or\n"
                   "- the convergence threshold (tol). \n"
                   "************************************************ \n\n")


def summary(object, thres=0.5, fdr_adjust=False, full_summary=True, file=None, device=0):
    """summary.atlasqtl, R/summarise_output.R:83-137: prints the posterior summary for variable selection to `file`
    (default sys.stdout) and returns what it printed: gam_vb, beta_vb, theta_vb (Min., 1st Qu., Median, Mean, 3rd Qu., Max. as
    dicts; with full_summary only), nb_pairwise, n_active, hotspot_sizes (the six numbers of the active predictors' sizes,
    None when there is none), top (up to six (name, size) by decreasing size) and rs_thres.

    A dense result (gam_vb, beta_vb present) is summarised here, the p q quartiles by value_summary on the GPU `device`.
    A sparse result must come from sparse_output={..., "summary": True} and the same (thres, fdr_adjust): its matrices
    never left the GPU, the numbers were taken there."""
    file = sys.stdout if file is None else file
    thres, fdr_adjust = float(thres), bool(fdr_adjust)
    dense = "gam_vb" in object and "beta_vb" in object
    if not dense:
        if "value_summary" not in object:
            raise ValueError('summary() of a sparse result needs the quartiles taken on the GPU: run atlasqtl with '
                             'sparse_output={..., "summary": True}')
        used = object["sparse_output"]
        if (float(used["thres"]), bool(used["fdr_adjust"])) != (thres, fdr_adjust):
            raise ValueError(f"summary(thres={thres}, fdr_adjust={fdr_adjust}) of a sparse result computed with thres="
                             f"{used['thres']}, fdr_adjust={used['fdr_adjust']}: the p x q matrices are gone, only the run's "
                             "own threshold can be summarised")
    out = {}
    file.write("****************************************************** \n"
               "* ATLASQTL: posterior summary for variable selection *\n"
               "****************************************************** \n\n")
    if full_summary:
        if dense:
            out["gam_vb"] = _only_six(value_summary(object["gam_vb"], device))
            out["beta_vb"] = _only_six(value_summary(object["beta_vb"], device))
        else:
            out["gam_vb"] = _only_six(object["value_summary"]["gam_vb"])
            out["beta_vb"] = _only_six(object["value_summary"]["beta_vb"])
        out["theta_vb"] = _only_six(six_numbers_host_(object["theta_vb"]))
        file.write("Posterior probabilities pairwise association, pr(gamma_st = 1 | y)\n")
        _print_six(out["gam_vb"], file)
        file.write("\nPosterior mean of pairwise regression coefficients, E(beta_st | y)\n")
        _print_six(out["beta_vb"], file)
        file.write("\nPosterior mean of hotspot propensities, E(theta_s | y)\n ")
        _print_six(out["theta_vb"], file)
        file.write("\n\n")
    if dense:
        rs_thres, nb_pairwise = hotspot_sizes(object["gam_vb"], thres, fdr_adjust, device)
    else:
        rs_thres, nb_pairwise = np.asarray(object["rs_thres"], dtype=np.int64), int(object["nb_pairwise"])
    if fdr_adjust:
        file.write(f"Using a {_rchar(100 * thres)}% FDR control:\n-----------------------\n")
    else:
        file.write(f"Using a PPI threshold of {_rchar(thres)}:\n------------------------------\n")
    active = rs_thres > 0
    n_active = int(active.sum())
    file.write(f"\nNb of pairwise (predictor-response) associations: {nb_pairwise} \n")
    file.write("\nNb of predictors associated with at least one response \n"
               f"(active predictors): {n_active} \n")
    file.write("\nHotspot sizes (nb of responses associated with each \nactive predictor):\n")
    sizes = _only_six(six_numbers_host_(rs_thres[active])) if n_active else None
    _print_six(sizes, file)
    names = object.get("names_x_all", object.get("names_x"))
    if names is None or len(names) != rs_thres.size:
        names = [str(j + 1) for j in range(rs_thres.size)]
    order = np.argsort(-rs_thres, kind="stable")[:min(n_active, 6)]     # sort(decreasing = TRUE) keeps ties in predictor order
    top = [(names[j], int(rs_thres[j])) for j in order]
    if top:
        label = [f"{nm} (size {sz})" for nm, sz in top]
        file.write("\nTop hotspots: \n" + ", ".join(label[:3]) + (", " if len(top) > 3 else ". ") + "\n")
        if len(top) > 3:
            file.write(", ".join(label[3:]))
    out.update(nb_pairwise=int(nb_pairwise), n_active=n_active, hotspot_sizes=sizes, top=top, rs_thres=rs_thres)
    return out
