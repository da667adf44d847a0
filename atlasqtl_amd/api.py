"""User-level entry point: ``atlasqtl()`` with the reference's argument surface
(R/atlasqtl.R:179-184) and return fields (R/atlasqtl.R:293-316,
R/atlasqtl_global_local_core.R:426-428).  Pre-processing and hyper-parameter /
initialisation handling run on the host (prepare.py, hyper_init.py); the
variational loop runs on the GPU through core.atlasqtl_global_local_core_.
"""
from __future__ import annotations

import warnings

import numpy as np

from .core import atlasqtl_global_local_core_, sparse_output_options
from .hyper_init import prepare_list_hyper_, prepare_list_init_
from .prepare import check_annealing_, check_positive_, check_vector_, check_verbose_, prepare_data_


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


def atlasqtl(Y, X, p0, anneal=(1, 2, 10), tol=0.1, maxit=1000, user_seed=None, verbose=1, list_hyper=None,
             list_init=None, save_hyper=False, save_init=False, full_output=False, thinned_elbo_eval=True,
             checkpoint_path=None, trace_path=None, add_collinear_back=False, device=0, device_init=False,
             sparse_output=None):
    """R/atlasqtl.R:179-322.

    sparse_output = {"thres": 0.5, "fdr_adjust": False, "max_pairs": None} (missing keys take these values): instead of
    the p x q gam_vb / beta_vb, return what summary.atlasqtl reads off them (R/summarise_output.R:99-106) -- `assoc`, the
    table of pairs with gam_vb > thres (or assign_bFDR(gam_vb) < thres) with snp / trait indices and names, ppi, beta and
    fdr; `rs_thres` and `nb_pairwise` -- so that the matrices never leave the GPU.  None: the dense result."""
    sparse = None if sparse_output is None else sparse_output_options(sparse_output)
    if sparse is not None and add_collinear_back and sparse["fdr_adjust"]:
        raise ValueError("add_collinear_back=True cannot be combined with sparse_output in FDR mode: the re-inserted copies "
                         "would take part in the FDR ranking, which changes the selected set and cannot be derived from the "
                         "table.  Use the PPI mode (fdr_adjust=False) or the dense output.")
    check_verbose_(verbose)
    check_annealing_(anneal)
    dat = prepare_data_(Y, X, tol, maxit, user_seed, verbose, checkpoint_path, trace_path)
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
    df = 1                                                                  # :272  (hs <- TRUE, debug <- TRUE :267-268)
    res = atlasqtl_global_local_core_(Yc, Xs, shr_fac_inv, None if anneal is None else tuple(anneal), df, tol,
                                      maxit, verbose, list_hyper, list_init, checkpoint_path, trace_path,
                                      full_output, thinned_elbo_eval, debug=True, device=device,
                                      # the collinear copies are added to the complete table; max_pairs cuts afterwards
                                      sparse_output=None if sparse is None else
                                      {**sparse, "max_pairs": None if add_collinear_back else sparse["max_pairs"]})
    res = AtlasqtlResult(res)
    res["p0"] = p0
    res["rmvd_cst_x"] = dat["rmvd_cst_x"]
    res["rmvd_coll_x"] = dat["rmvd_coll_x"]
    res["names_x"], res["names_y"] = dat["names_x"], dat["names_y"]
    names_snp = dat["names_x"]
    if sparse is not None:
        if add_collinear_back:
            if dat["rmvd_coll_x"]:
                res["assoc"], res["rs_thres"], res["theta_vb"] = add_collinear_back_pairs_(
                    res["assoc"], res["rs_thres"], res["theta_vb"], dat["initial_colnames_X"], dat["rmvd_coll_x"],
                    dat["names_x"], sparse["max_pairs"])
                res["nb_pairwise"] = res["assoc"]["n_pairs"]
                names_snp = dat["initial_colnames_X"]
            elif sparse["max_pairs"] is not None:
                res["assoc"] = {k: (v if k == "n_pairs" else v[:int(sparse["max_pairs"])]) for k, v in res["assoc"].items()}
        res["assoc"]["snp_name"] = np.asarray(names_snp, dtype=object)[res["assoc"]["snp"]]
        res["assoc"]["trait_name"] = np.asarray(dat["names_y"], dtype=object)[res["assoc"]["trait"]]
    elif add_collinear_back and dat["rmvd_coll_x"]:
        res["beta_vb"], res["gam_vb"], res["theta_vb"] = add_collinear_back_(
            res["beta_vb"], res["gam_vb"], res["theta_vb"], dat["initial_colnames_X"], dat["rmvd_coll_x"],
            dat["names_x"])
    if save_hyper:
        res["list_hyper"] = list_hyper
    if save_init:
        res["list_init"] = list_init
    return res
