"""The preparation of the data, mirroring the reference's R/prepare_atlasqtl.R:8-87 (``prepare_data_``) and
R/utils.R:276-343 (``rm_constant_``, ``rm_collinear_``).  The argument checks (checks.py) run on the host; the O(n p) work
itself -- scale(X), the removal of constant and duplicated columns, the centring of Y -- runs on the GPU and X
stays there: one call of aq_prepare_data_opt, the five aq_prepare_data* entries in one, whose pipeline is csrc/aq_prepare.hip;
the .bed decode, the covariates, the transform of Y and LD pruning are the csrc/aq_prep_*.hip units.  Covariates, which the
reference does not take, are regressed out of X and Y there as well, and the compact matrix can be pruned for linkage
disequilibrium there before the fit (aq_prep_ld_prune).  The rank-based inverse normal transform of the traits (transform_y=,
rank_normalize) runs there too, before everything else that is done to Y (aq_prepare_data_opt, aq_rank_int).  Here: the
parsers of the options, rank_normalize, prepare_on_device and prepare_data_; the PreparedData they return is prepared.py, the
genotype GRM / principal components taken from one (genotype_grm, genotype_pcs) stay here, below their rule: their names are
what callers import from this module.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings

import numpy as np

from . import _lib
from .checks import AtlasqtlError, _is_real, _is_whole, check_matrix_, check_natural_, check_positive_, check_vector_
from .plink import PlinkBed
from .prepared import PreparedData, raise_for_code


def _covariates_arg(covariates, n):
    """The covariates as aq_prepare_data_cov takes them: (AqPrepCov, the n x d Fortran array it points into), or (None, None)."""
    if covariates is None:
        return None, None
    try:
        Z = np.asfortranarray(covariates, dtype=np.float64)
    except (TypeError, ValueError):
        Z = None
    if Z is None or Z.ndim != 2 or Z.shape[1] < 1 or not np.all(np.isfinite(Z)):
        raise AtlasqtlError("covariates must be a non-empty a numeric matrix, finite without missing value.")
    if Z.shape[0] != n:
        raise AtlasqtlError(f"covariates and Y must have the same number of samples ({Z.shape[0]} and {n} rows).")
    cov = _lib.AqPrepCov()
    cov.d, cov.Z = Z.shape[1], _lib.as_dp(Z)
    return cov, Z


GRM_MAX_N = 10240             # AQ_GRM_MAX_N of csrc/aq_grm_plan.h
N_MAX = 82944                 # AQ_N_MAX of csrc/aq_plan_const.h: the samples a fit takes
PCS_MAX_L = 128               # AQ_PCS_MAX_L of csrc/aq_pcs_plan.h: vectors per block of aq_prep_grm_apply
PC_SOLVERS = ("eigh", "subspace")
PC_SOLVER_DEFAULTS = {"solver": "eigh", "oversample": None, "tol": 1e-8, "max_iter": 300, "seed": 0}
COV_MAX_D = 96                # AQ_COV_MAX_D: covariates that aq_prepare_data_cov takes
LD_PRUNE_DEFAULTS = {"r2": 0.8, "window": 500, "window_bp": None, "groups": None, "positions": None}
LD_MAX_WINDOW = 4096          # AQ_LD_MAX_WINDOW of csrc/aq_ld_kernels.h
TRANSFORM_Y_DEFAULTS = {"method": "int", "offset": 0.375}


def transform_y_options(transform_y):
    """The `transform_y` argument of atlasqtl() / prepare_on_device checked on the host: None (no transform), "int", or a dict
    with the keys 'method' ("int", the rank-based inverse normal transform) and, optionally, 'offset' (c in [0, 1/2]: 3/8 Blom,
    the default; 0 van der Waerden; 1/2 rankit).  Returns None or {"method": "int", "offset": c}."""
    if transform_y is None:
        return None
    if isinstance(transform_y, str):
        transform_y = {"method": transform_y}
    if not isinstance(transform_y, dict) or "method" not in transform_y or set(transform_y) - set(TRANSFORM_Y_DEFAULTS):
        raise AtlasqtlError("transform_y must be None, 'int' or a dict with the key 'method' and, optionally, 'offset'.")
    o = {**TRANSFORM_Y_DEFAULTS, **transform_y}
    if not isinstance(o["method"], str) or o["method"] != "int":
        raise AtlasqtlError(f"transform_y: method must be 'int' (the rank-based inverse normal transform), not {o['method']!r}.")
    o["offset"] = _check_int_offset(o["offset"], "transform_y")
    return o


def _check_int_offset(c, what):
    if not _is_real(c, 0.0, 0.5):
        raise AtlasqtlError(f"{what}: offset must be a number in [0, 1/2], not {c!r}.")
    return float(c)


def _ytrans_arg(transform_y):
    """The transform as aq_prepare_data_opt takes it: (AqPrepYtrans, the options), or (None, None)."""
    o = transform_y_options(transform_y)
    if o is None:
        return None, None
    yt = _lib.AqPrepYtrans()
    yt.method, yt.offset = 1, o["offset"]
    return yt, o


def rank_normalize(Y, offset=0.375, device=0):
    """The rank-based inverse normal transform of every column of Y (n x q, NaN = missing and stays NaN) on the GPU
    (aq_rank_int): Phi^-1((r - offset) / (m + 1 - 2 offset)) with r the 1-based rank among the m observed values of the column,
    ties given their average rank.  Returns dict(Y n x q, n_obs (q), n_tied (q): the observed values of a column that share
    their value with another one).  A column with fewer than two distinct observed values raises AtlasqtlError."""
    c = _check_int_offset(offset, "rank_normalize")
    try:
        Ya = np.asfortranarray(Y, dtype=np.float64)
    except (TypeError, ValueError):
        Ya = None
    if Ya is None or Ya.ndim != 2 or Ya.shape[0] < 2 or Ya.shape[1] < 1:
        raise AtlasqtlError("rank_normalize: Y must be a numeric matrix with at least 2 rows and 1 column.")
    n, q = Ya.shape
    if n > N_MAX:
        raise AtlasqtlError(f"rank_normalize: n = {n} samples given, at most {N_MAX} are supported.")
    out = np.empty((n, q), order="F")
    n_obs = np.zeros(q, dtype=np.int32); n_tied = np.zeros(q, dtype=np.int32)
    raise_for_code(_lib.lib().aq_rank_int(_lib.as_dp(Ya), n, q, c, _lib.as_dp(out), _lib.as_ip(n_obs), _lib.as_ip(n_tied), int(device)),
                   "aq_rank_int")
    return dict(Y=out, n_obs=n_obs, n_tied=n_tied)


def ld_prune_options(ld_prune):
    """The `ld_prune` argument of atlasqtl() / prepare_on_device with its defaults filled in and checked on the host:
    r2 in (0, 1], window a whole number in [1, 4096], window_bp None or a whole number >= 1, groups None or one label per
    predictor given, positions None or one whole number per predictor given."""
    if not isinstance(ld_prune, dict) or set(ld_prune) - set(LD_PRUNE_DEFAULTS):
        raise AtlasqtlError("ld_prune must be None or a dict with keys among 'r2', 'window', 'window_bp', 'groups', 'positions'.")
    o = {**LD_PRUNE_DEFAULTS, **ld_prune}
    r2 = o["r2"]
    if not _is_real(r2, 0.0, 1.0, lo_open=True):
        raise AtlasqtlError(f"ld_prune: r2 must be a number in (0, 1], not {r2!r}.")
    if not _is_whole(o["window"]) or not (1 <= int(o["window"]) <= LD_MAX_WINDOW):
        raise AtlasqtlError(f"ld_prune: window must be a whole number in [1, {LD_MAX_WINDOW}], not {o['window']!r}.")
    if o["window_bp"] is not None and (not _is_whole(o["window_bp"]) or int(o["window_bp"]) < 1):
        raise AtlasqtlError(f"ld_prune: window_bp must be None or a whole number >= 1, not {o['window_bp']!r}.")
    if o["groups"] is not None:
        g = np.asarray(o["groups"])
        if g.ndim != 1 or g.size == 0:
            raise AtlasqtlError("ld_prune: groups must be None or a one-dimensional array with one label per predictor.")
    if o["positions"] is not None:
        try:
            pos = np.asarray(o["positions"])
            ok = pos.ndim == 1 and pos.size > 0 and (np.issubdtype(pos.dtype, np.integer) or
                                                      (np.issubdtype(pos.dtype, np.floating) and bool(np.all(np.isfinite(pos)))
                                                       and bool(np.all(pos == np.round(pos)))))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise AtlasqtlError("ld_prune: positions must be None or a one-dimensional array of whole numbers, one per predictor.")
    o["r2"], o["window"] = float(r2), int(o["window"])
    o["window_bp"] = None if o["window_bp"] is None else int(o["window_bp"])
    return o


def _ld_arg(ld_prune, X):
    """The pruning as aq_prep_ld_prune takes it: (AqPrepLd, the arrays it points into), or (None, None).  For a PlinkBed the
    groups default to its chromosomes and, with window_bp, the positions to its base-pair positions.  All checks are here,
    before the first device call."""
    if ld_prune is None:
        return None, None
    o = ld_prune_options(ld_prune)
    p = X.p if isinstance(X, PlinkBed) else (np.shape(X)[1] if np.ndim(X) == 2 else -1)
    groups, positions = o["groups"], o["positions"]
    if isinstance(X, PlinkBed):
        if groups is None:
            groups = X.chrom
        if positions is None and o["window_bp"] is not None:
            positions = X.pos
    if o["window_bp"] is not None and positions is None:
        raise AtlasqtlError("ld_prune: window_bp needs positions (one per predictor given).")
    ld = _lib.AqPrepLd()
    ld.window, ld.r2, ld.window_bp = o["window"], o["r2"], 0 if o["window_bp"] is None else o["window_bp"]
    ld.group, ld.pos = None, None
    keep = []
    for name, arr in (("groups", groups), ("positions", positions)):
        if arr is not None and np.asarray(arr).shape != (p,):
            raise AtlasqtlError(f"ld_prune: {name} must hold one entry per predictor given ({p}), not {np.asarray(arr).shape}.")
    if groups is not None:
        codes = np.ascontiguousarray(np.unique(np.asarray(groups), return_inverse=True)[1].reshape(-1), dtype=np.int32)
        ld.group = _lib.as_ip(codes)
        keep.append(codes)
    if positions is not None:
        pos = np.ascontiguousarray(positions, dtype=np.int64)
        ld.pos = pos.ctypes.data_as(C.POINTER(C.c_int64))
        keep.append(pos)
    return ld, keep


def _ld_prune_handle(ret, ld):
    """aq_prep_ld_prune on the PreparedData of a prepare_on_device return value; fills its ld_* fields."""
    prep = ret[0]
    L = _lib.lib()
    p = len(ret[1])
    try:
        raise_for_code(L.aq_prep_ld_prune(prep.handle, C.byref(ld)), "aq_prep_ld_prune")
    except Exception:
        prep.close()
        raise
    pk = C.c_int32(0)
    rm = np.zeros(p, dtype=np.uint8); of = np.zeros(p, dtype=np.int32); r2 = np.zeros(p)
    _lib.check(L.aq_prep_ld_info(prep.handle, C.byref(pk), rm.ctypes.data_as(C.POINTER(C.c_uint8)), _lib.as_ip(of), _lib.as_dp(r2)),
               "aq_prep_ld_info")
    prep.p, prep.shape = int(pk.value), (prep.n, int(pk.value))
    prep.ld_removed, prep.ld_of, prep.ld_r2 = rm.astype(bool), of, r2
    return ret


def prepare_on_device(Y, X, device=0, covariates=None, ld_prune=None, transform_y=None):
    """scale(X), constant / duplicate-column removal and the centring of Y on the GPU (R/prepare_atlasqtl.R:57-83).
    X: float64 (n x p), int8 dosages (1 byte per genotype: the fp64 matrix is then never formed on the host), or a
    plink.PlinkBed (2 bits per genotype: the packed blocks of the .bed are uploaded and unpacked on the GPU; the returned
    PreparedData then carries genotype_counts).
    covariates: n x d (1 <= d <= 96, finite, rows as in Y), regressed with an intercept out of every column of X (over all
    rows) and of Y (over the column's observed rows) before the above; a column of X that they explain (1 - R^2 <= 1e-10) is
    reported constant and flagged in PreparedData.cov_absorbed.
    ld_prune: None, or a dict (ld_prune_options: r2 0.8, window 500, window_bp, groups, positions).  After the above, column j of
    the compact matrix is removed when a kept column i < j with j - i <= window, the same group and, with window_bp, a
    position within window_bp of its own has r(i, j)^2 > r2; the first one wins.  The PreparedData then holds the pruned matrix
    and ld_removed / ld_of / ld_r2 per column given.  A PlinkBed's chromosomes are the default groups, its base-pair positions
    the default positions.
    transform_y: None, "int" or {"method": "int", "offset": 0.375} (transform_y_options): the rank-based inverse normal transform
    of every column of Y over its observed rows, before the regression on the covariates or the centring (rank_normalize); the
    PreparedData then carries y_n_obs and y_n_tied.  X is prepared as without it.
    Returns (PreparedData, bool_cst_x [p], bool_coll_x [p, original numbering], dup_of [p])."""
    Y = np.asfortranarray(Y, dtype=np.float64)
    n, q = Y.shape
    cov, Z = _covariates_arg(covariates, n)
    ld, ld_arrays = _ld_arg(ld_prune, X)                       # checked here, before the first device call
    yt = _ytrans_arg(transform_y)[0]
    ret = _prepare_unpruned(Y, X, device, cov, yt)
    return ret if ld is None else _ld_prune_handle(ret, ld)


def _prepare_unpruned(Y, X, device, cov, yt=None):
    """prepare_on_device before any pruning: Y float64 in Fortran order, cov from _covariates_arg, yt from _ytrans_arg."""
    n, q = Y.shape
    if isinstance(X, PlinkBed):
        return _prepare_bed_on_device(Y, X, device, cov, yt)
    pin = _lib.AqPrepInput()
    if np.asarray(X).dtype == np.int8:
        Xa = np.asfortranarray(X)
        pin.X, pin.X_i8 = None, Xa.ctypes.data_as(C.POINTER(C.c_int8))
    else:
        Xa = np.asfortranarray(X, dtype=np.float64)
        pin.X, pin.X_i8 = _lib.as_dp(Xa), None
    if Xa.shape[0] != n:
        raise AtlasqtlError("X and Y must have the same number of samples.")
    p = Xa.shape[1]
    pin.n, pin.p, pin.q, pin.Y, pin.device = n, p, q, _lib.as_dp(Y), int(device)
    return _prepare_opt(pin, False, cov, yt, n, p, q, device)


def _prepare_opt(pin, bed, cov, yt, n, p, q, device):
    """aq_prepare_data_opt on the one input given (pin: an AqPrepBedInput if bed, else an AqPrepInput; cov, yt: None where
    absent) and the return value of prepare_on_device from its handle.  An error names the entry that the arguments name."""
    h = C.c_void_p()
    rc = _lib.lib().aq_prepare_data_opt(None if bed else C.byref(pin), C.byref(pin) if bed else None, None if cov is None else C.byref(cov),
                                        None if yt is None else C.byref(yt), C.byref(h))
    what = "aq_prepare_data_opt" if yt is not None else "aq_prepare_data" + ("_bed" if bed else "") + ("" if cov is None else "_cov")
    return _prepared_from_handle(rc, h, what, n, p, q, device, bed=bed, cov=cov is not None, ytrans=yt is not None)


def _prepared_from_handle(rc, h, what, n, p, q, device, bed=False, cov=False, ytrans=False):
    """The return value of prepare_on_device from the handle aq_prepare_data / aq_prepare_data_bed made (or their error)."""
    raise_for_code(rc, what)
    pk = C.c_int32(0)
    cst = np.zeros(p, dtype=np.uint8); coll = np.zeros(p, dtype=np.uint8); dup = np.zeros(p, dtype=np.int32)
    _lib.check(_lib.lib().aq_prep_info(h, C.byref(pk), cst.ctypes.data_as(C.POINTER(C.c_uint8)),
                                       coll.ctypes.data_as(C.POINTER(C.c_uint8)), _lib.as_ip(dup), None, None), "aq_prep_info")
    Yc = np.empty((n, q), order="F")
    _lib.check(_lib.lib().aq_prep_get(h, None, _lib.as_dp(Yc)), "aq_prep_get")
    counts = None
    if bed:
        counts = np.zeros((4, p), dtype=np.int32, order="F")
        _lib.check(_lib.lib().aq_prep_genotype_counts(h, _lib.as_ip(counts)), "aq_prep_genotype_counts")
    n_cov, absorbed, r2 = 0, None, None
    if cov:
        d = C.c_int32(0)
        absorbed = np.zeros(p, dtype=np.uint8); r2 = np.zeros(p)
        _lib.check(_lib.lib().aq_prep_cov_info(h, C.byref(d), absorbed.ctypes.data_as(C.POINTER(C.c_uint8)), _lib.as_dp(r2)),
                   "aq_prep_cov_info")
        n_cov, absorbed = int(d.value), absorbed.astype(bool)
    y_n_obs = y_n_tied = None
    if ytrans:
        y_n_obs = np.zeros(q, dtype=np.int32); y_n_tied = np.zeros(q, dtype=np.int32)
        _lib.check(_lib.lib().aq_prep_ytrans_info(h, None, None, _lib.as_ip(y_n_obs), _lib.as_ip(y_n_tied)), "aq_prep_ytrans_info")
    return (PreparedData(h, n, int(pk.value), q, Yc, int(device), genotype_counts=counts, n_cov=n_cov, cov_absorbed=absorbed,
                         cov_r2=r2, y_n_obs=y_n_obs, y_n_tied=y_n_tied), cst.astype(bool), coll.astype(bool), dup)


def _prepare_bed_on_device(Y, bed, device, cov=None, yt=None):
    """prepare_on_device for a plink.PlinkBed: the packed blocks go to the library as they are (the .bed input of
    aq_prepare_data_opt)."""
    n, q = Y.shape
    if bed.n != n:
        raise AtlasqtlError("X and Y must have the same number of samples.")
    blocks = bed.packed()                                  # p x stride uint8; a view of the memory map where it can be
    pin = _lib.AqPrepBedInput()
    pin.n_file, pin.n, pin.p, pin.q = bed.n_file, n, bed.p, q
    pin.bed = C.cast(blocks.ctypes.data, C.POINTER(C.c_uint8))
    pin.sample_idx = None if bed.sample_index is None else _lib.as_ip(bed.sample_index)
    pin.Y, pin.device = _lib.as_dp(Y), int(device)
    pin.count_a2, pin.missing = int(bed.count == "A2"), int(bed.missing == "mean")
    return _prepare_opt(pin, True, cov, yt, n, bed.p, q, device)       # `blocks` lives until the call has returned


def prepare_data_(Y, X, tol, maxit, user_seed, verbose, checkpoint_path, trace_path,
                  names_x=None, names_y=None, device=0, covariates=None, ld_prune=None, transform_y=None):
    """R/prepare_atlasqtl.R:8-87.  Returns dict(Y, X, bool_rmvd_x, initial_colnames_X,
    rmvd_cst_x, rmvd_coll_x, names_x, names_y, genotype_counts, n_covariates, rmvd_cov_x, cov_r2_x); X is a PreparedData (the
    standardised matrix lives on the GPU), Y the centred responses on the host.  With covariates (prepare_on_device) both are
    residuals; rmvd_cov_x names the predictors that the covariates absorb (they are in rmvd_cst_x too) and cov_r2_x holds, per
    predictor given, the share of its variance that they explain.  X may be float64, int8 dosages or a plink.PlinkBed, whose variant IDs are
    the default names_x and whose per-variant genotype counts are returned as genotype_counts (None otherwise).
    With ld_prune (prepare_on_device) bool_rmvd_x and names_x account for the predictors removed for LD as well; rmvd_ld_x maps
    each of them to the kept predictor that tags it and ld_r2_x holds, per predictor given, its r^2 with that one (NaN: kept or
    removed for another reason).  Both are None without pruning.
    With transform_y (prepare_on_device) Y is rank-normalised before all that; transform_y holds the options used and y_n_obs /
    y_n_tied the observed and the tied values per trait.  All three are None without it."""
    is_bed = isinstance(X, PlinkBed)
    check_vector_(user_seed, "user_seed", size=1, null_ok=True)
    check_vector_(tol, "tol", size=1)
    check_positive_(tol, "tol", eps=np.finfo(np.float64).eps)
    check_vector_(maxit, "maxit", size=1)
    check_natural_(maxit, "maxit")
    if not is_bed and not (isinstance(X, np.ndarray) and X.dtype == np.int8 and X.ndim == 2 and X.size > 0):
        X = check_matrix_(X, "X")
    if checkpoint_path is not None and not os.path.isdir(checkpoint_path):
        raise AtlasqtlError("The directory specified in checkpoint_path does not exist. Please make sure to "
                            "provide a valid path.")
    if trace_path is not None and not os.path.isdir(trace_path):
        raise AtlasqtlError("The directory specified in trace_path does not exist. Please make sure to "
                            "provide a valid path.")
    n, p = X.shape
    Y = check_matrix_(Y, "Y", na_ok=True)
    q = Y.shape[1]
    if Y.shape[0] != n:
        raise AtlasqtlError("X and Y must have the same number of samples.")
    if np.sum(~np.isnan(Y)) / (n * q) < 0.05:
        raise AtlasqtlError("Too few non-NA values in matrix Y. Exit.")
    ind_low = (np.sum(~np.isnan(Y), axis=0) / n) < 0.025
    if ind_low.any():
        raise AtlasqtlError(f"Column(s) {list(np.where(ind_low)[0] + 1)} of matrix Y have more than 97.5% "
                            "missing values, and should be removed. Exit.")
    if names_x is None:
        names_x = list(X.snp_names) if is_bed else [f"Cov_x_{j + 1}" for j in range(p)]
    if names_y is None:
        names_y = [f"Resp_{k + 1}" for k in range(q)]

    # scale(X), rm_constant_, rm_collinear_, centring of Y: on the device (csrc/aq_prepare.hip and its aq_prep_*.hip units); X stays there
    yt_opts = transform_y_options(transform_y)
    prep, bool_cst_x, bool_coll_full, dup_of = prepare_on_device(Y, X, device, covariates, ld_prune, transform_y=yt_opts)
    rmvd_cst_x = [names_x[j] for j in np.where(bool_cst_x)[0]] if bool_cst_x.any() else None
    names_after_cst = [nm for nm, b in zip(names_x, bool_cst_x) if not b]
    bool_rmvd_x = bool_cst_x | bool_coll_full
    rmvd_ld_x = None
    if prep.ld_removed is not None:
        bool_rmvd_x = bool_rmvd_x | prep.ld_removed
        rmvd_ld_x = {names_x[j]: names_x[prep.ld_of[j]] for j in np.where(prep.ld_removed)[0]} or None   # removed name -> tag name
    rmvd_coll_x = {names_x[j]: names_x[dup_of[j]] for j in np.where(bool_coll_full)[0]} or None   # removed name -> kept name
    return dict(Y=prep.Y, X=prep, bool_rmvd_x=bool_rmvd_x, initial_colnames_X=names_after_cst,
                rmvd_cst_x=rmvd_cst_x, rmvd_coll_x=rmvd_coll_x, genotype_counts=prep.genotype_counts,
                n_covariates=prep.n_cov, cov_r2_x=prep.cov_r2, rmvd_ld_x=rmvd_ld_x, ld_r2_x=prep.ld_r2,
                transform_y=yt_opts, y_n_obs=prep.y_n_obs, y_n_tied=prep.y_n_tied,
                rmvd_cov_x=[names_x[j] for j in np.where(prep.cov_absorbed)[0]] if prep.n_cov and prep.cov_absorbed.any() else None,
                names_x=[nm for nm, b in zip(names_x, bool_rmvd_x) if not b], names_y=list(names_y))


# ---- genotype principal components: the GRM on the device (aq_prep_grm), its leading eigenvectors on the host ----
def pc_sign_(V):
    """Each column of V with the sign that makes its entry of largest magnitude positive; on a tie the first such entry
    decides.  Equal inputs therefore give equal bits."""
    V = np.array(V, dtype=np.float64, order="F", ndmin=2)
    for c in range(V.shape[1]):
        if V[np.argmax(np.abs(V[:, c])), c] < 0:                 # argmax returns the first of equal magnitudes
            V[:, c] = -V[:, c]
    return V


def pcs_from_grm_(K, k, trace=None):
    """The k leading eigenpairs of the symmetric matrix K (numpy.linalg.eigh: n^3 on the host, against the n^2 p of the GRM on
    the device with p >> n): dict(pcs n x k with unit-norm columns signed by pc_sign_, eigenvalues descending, var_explained =
    eigenvalue / trace)."""
    w, V = np.linalg.eigh(K)
    top = np.arange(w.size - 1, w.size - 1 - int(k), -1)
    lam = w[top]
    tr = float(np.trace(K)) if trace is None else float(trace)
    return dict(pcs=pc_sign_(V[:, top]), eigenvalues=lam, var_explained=lam / tr)


def _n_of(X):
    if isinstance(X, PlinkBed):
        return X.n
    if np.ndim(X) != 2 or np.shape(X)[0] < 1:
        raise AtlasqtlError("X must be a non-empty a numeric matrix, finite without missing value.")
    return int(np.shape(X)[0])


def _check_grm_n(n, what, pcs=False):
    if n > GRM_MAX_N:
        hint = ' genotype_pcs with solver="subspace" takes the leading components without that matrix.' if pcs else ""
        raise AtlasqtlError(f"{what}: n = {n} samples given, at most {GRM_MAX_N} are supported (the n x n relationship matrix "
                            f"is decomposed on the host).{hint}")


def pc_solver_options(k, n, what, solver="eigh", oversample=None, tol=1e-8, max_iter=300, seed=0):
    """The solver arguments of genotype_pcs() checked on the host; returns them as a dict with `oversample` resolved: 16 unless
    given, then clipped so that the block width L = k + oversample stays <= min(128, n - 1).  solver="eigh" is refused above
    10240 samples, solver="subspace" above the 82944 a fit takes."""
    if not isinstance(solver, str) or solver not in PC_SOLVERS:
        raise AtlasqtlError(f"{what}: solver must be 'eigh' or 'subspace', not {solver!r}.")
    if oversample is not None and (not _is_whole(oversample) or int(oversample) < 0):
        raise AtlasqtlError(f"{what}: oversample must be None or a whole number >= 0, not {oversample!r}.")
    if not _is_whole(max_iter) or int(max_iter) < 1:
        raise AtlasqtlError(f"{what}: max_iter must be a whole number >= 1, not {max_iter!r}.")
    if not _is_whole(seed) or int(seed) < 0:
        raise AtlasqtlError(f"{what}: seed must be a whole number >= 0, not {seed!r}.")
    if not _is_real(tol, 0.0, np.inf, lo_open=True, hi_open=True):
        raise AtlasqtlError(f"{what}: tol must be a number > 0, not {tol!r}.")
    if _is_whole(k) and oversample is not None and int(k) + int(oversample) > PCS_MAX_L:
        raise AtlasqtlError(f"{what}: k + oversample must be at most {PCS_MAX_L} (the block of vectors of solver='subspace'), "
                            f"not {int(k)} + {int(oversample)}.")
    if solver == "eigh":
        _check_grm_n(n, what, pcs=True)
    elif n > N_MAX:
        raise AtlasqtlError(f"{what}: n = {n} samples given, at most {N_MAX} are supported.")
    over = 16 if oversample is None else int(oversample)
    if _is_whole(k):
        over = max(0, min(over, min(PCS_MAX_L, n - 1) - int(k)))
    return dict(solver=solver, oversample=over, tol=float(tol), max_iter=int(max_iter), seed=int(seed))


def subspace_pcs_(apply, n, k, oversample=16, tol=1e-8, max_iter=300, seed=0, trace=None):
    """The k leading eigenpairs of a symmetric positive semi-definite operator given only as `apply`: Q (n x L) -> K Q, by
    subspace iteration with a Rayleigh-Ritz step on a block of L = k + oversample vectors.
      Q_0 = the Q factor of numpy.random.default_rng(seed).standard_normal((n, L)); every iteration forms Z = apply(Q),
      B = sym(Q' Z) and its eigenpairs (w descending, W), the Ritz vectors V = Q W and the residuals ||Z W - V diag(w)||_2 per
      column divided by w_1; it stops when the largest of the first k residuals is <= tol, else Q = the Q factor of Z.
    The n x L QR and the L x L eigh run on the host.  Returns dict(pcs n x k signed by pc_sign_, eigenvalues (k, descending),
    var_explained = eigenvalue / trace (NaN without `trace`), iterations, converged, residuals (k)).
    The error of Ritz vector i is at most 2 residual_i lambda_1 / gap_i (Davis-Kahan), gap_i the distance of lambda_i to the
    nearest other eigenvalue, and the iteration contracts component i by lambda_(L+1) / lambda_i per step: a few steps for
    components of population structure, which stand clear of the bulk.  Components INSIDE the noise bulk have tiny gaps, and
    plain subspace iteration then needs hundreds of steps (146 ... 242 at n = 300 for k = 5 with two structural components); a
    block Krylov method would be the tool, and is not built.  `max_iter` bounds the work: when it is reached a warning is
    given, converged is False, and what is returned is still an orthonormal Ritz basis with its residuals -- never an
    exception.  Equal inputs give equal bits."""
    n, k, L = int(n), int(k), int(k) + int(oversample)
    Q = np.linalg.qr(np.random.default_rng(int(seed)).standard_normal((n, L)))[0]
    converged, it = False, 0
    for it in range(1, int(max_iter) + 1):
        Z = np.asarray(apply(Q), dtype=np.float64)
        B = Q.T @ Z
        w, W = np.linalg.eigh(0.5 * (B + B.T))
        w, W = w[::-1], W[:, ::-1]
        V = Q @ W
        res = np.linalg.norm(Z @ W - V * w, axis=0) / w[0]
        if float(np.max(res[:k])) <= tol:
            converged = True
            break
        Q = np.linalg.qr(Z)[0]
    if not converged:
        warnings.warn(f"subspace iteration for {k} genotype principal components has not converged after {it} iterations: the "
                      f"largest residual is {float(np.max(res[:k])):.3e}, tol = {tol:.3e}.  Components inside the noise bulk "
                      "converge slowly; raise max_iter or oversample, or ask for fewer components.")
    lam = np.array(w[:k])
    tr = float("nan") if trace is None else float(trace)
    return dict(pcs=pc_sign_(V[:, :k]), eigenvalues=lam, var_explained=lam / tr, iterations=it, converged=converged,
                residuals=np.array(res[:k]))


def _check_pc_count(k, n, d, what):
    if not _is_whole(k):
        raise AtlasqtlError(f"{what}: k must be a whole number, not {k!r}.")
    kmax = min(n - 2, COV_MAX_D - d)
    if not (1 <= int(k) <= kmax):
        raise AtlasqtlError(f"{what}: k must lie in [1, {kmax}] = [1, min(n - 2, {COV_MAX_D} - d)] with n = {n} samples and "
                            f"d = {d} covariates, not {k!r}.")
    return int(k)


def genotype_pcs_options(genotype_pcs, n, d=0):
    """The `genotype_pcs` argument of atlasqtl() checked on the host: a whole number k or a dict with the key 'k' and,
    optionally, 'ld_prune' (None, or the dict ld_prune= takes) and the solver arguments of genotype_pcs() ('solver',
    'oversample', 'tol', 'max_iter', 'seed'), with 1 <= k <= min(n - 2, 96 - d) for n samples and d user covariates, and
    n <= 10240 unless solver is 'subspace'.  Returns {"k": k, "ld_prune": dict or None} and the solver keys that were given."""
    form = ("genotype_pcs must be None, a whole number k or a dict with the key 'k' and, optionally, 'ld_prune', 'solver', "
            "'oversample', 'tol', 'max_iter', 'seed'.")
    given = {}
    if isinstance(genotype_pcs, dict):
        if "k" not in genotype_pcs or set(genotype_pcs) - {"k", "ld_prune"} - set(PC_SOLVER_DEFAULTS):
            raise AtlasqtlError(form)
        o = {"k": genotype_pcs["k"], "ld_prune": genotype_pcs.get("ld_prune")}
        given = {key: genotype_pcs[key] for key in PC_SOLVER_DEFAULTS if key in genotype_pcs}
    elif _is_whole(genotype_pcs):
        o = {"k": genotype_pcs, "ld_prune": None}
    else:
        raise AtlasqtlError(form)
    pc_solver_options(o["k"], n, "genotype_pcs", **given)
    o["k"] = _check_pc_count(o["k"], n, d, "genotype_pcs")
    if o["ld_prune"] is not None:
        try:
            ld_prune_options(o["ld_prune"])
        except AtlasqtlError as e:
            raise AtlasqtlError(f"genotype_pcs: {e}") from None
    o.update(given)
    return o


def _grm_of(X, device, covariates, ld_prune):
    """(K, trace K, p1) of X as prepare_on_device prepares it, with a one-column dummy Y (all observed, so it passes the
    missingness guards; all zero, so it is zero after centring or regression on any covariates).  The handle is closed."""
    n = _n_of(X)
    _check_grm_n(n, "genotype_grm")
    prep = prepare_on_device(np.zeros((n, 1), order="F"), X, device, covariates, ld_prune)[0]
    try:
        K, tr = prep.grm(return_trace=True)
        return K, tr, prep.p
    finally:
        prep.close()


def genotype_grm(X, device=0, covariates=None, ld_prune=None):
    """The n x n genetic relationship matrix K = Xs Xs' / p1 of X (float64, int8 dosages or a plink.PlinkBed) over the p1
    standardised columns that prepare_on_device keeps -- after constant and duplicate removal, with `covariates` on the
    residuals, with `ld_prune` on the pruned set -- formed on the GPU (aq_prep_grm).  Exactly symmetric; n <= 10240."""
    return _grm_of(X, device, covariates, ld_prune)[0]


def genotype_pcs(X, k, device=0, covariates=None, ld_prune=None, solver="eigh", oversample=None, tol=1e-8, max_iter=300, seed=0):
    """The k leading principal components of the genotypes X: eigenvectors of genotype_grm(X, ...).  Returns dict(pcs n x k,
    unit norm, each signed so that its entry of largest magnitude is positive; eigenvalues (k, descending); var_explained =
    eigenvalue / trace K; p_used = p1, the predictors K was formed over; solver; iterations; converged; residuals (k)).  Every
    column of Xs is centred, so the PCs are orthogonal to the intercept.  1 <= k <= n - 2 - d with d covariates: the residuals
    on them and the intercept span at most n - 1 - d dimensions, and a PC beyond that would be an eigenvector of rounding noise.
    solver="eigh" (the default): K is formed on the GPU and decomposed on the host, n <= 10240; iterations is 0, converged True
    and residuals None.
    solver="subspace": K is never formed.  subspace_pcs_ iterates a block of k + oversample vectors (oversample 16 unless
    given, the block at most min(128, n - 1) wide) whose product with K runs on the GPU (aq_prep_grm_apply); n up to 82944.
    It stops when the residuals of the k components are <= tol or after max_iter iterations (then with a warning and
    converged False, see subspace_pcs_ on components inside the noise bulk); seed fixes the starting block."""
    n = _n_of(X)
    if not _is_whole(k):
        raise AtlasqtlError(f"genotype_pcs: k must be a whole number, not {k!r}.")
    so = pc_solver_options(k, n, "genotype_pcs", solver, oversample, tol, max_iter, seed)
    Z = _covariates_arg(covariates, n)[1]
    d = 0 if Z is None else Z.shape[1]
    if not (1 <= int(k) <= n - 2 - d):
        raise AtlasqtlError(f"genotype_pcs: k must lie in [1, {n - 2 - d}] = [1, n - 2 - d] with n = {n} samples and d = {d} "
                            f"covariates regressed out of the genotypes, not {k!r}.")
    if so["solver"] == "eigh":
        K, tr, p1 = _grm_of(X, device, covariates, ld_prune)
        return dict(pcs_from_grm_(K, int(k), tr), p_used=int(p1), solver="eigh", iterations=0, converged=True, residuals=None)
    prep = prepare_on_device(np.zeros((n, 1), order="F"), X, device, covariates, ld_prune)[0]
    try:
        trace = []

        def apply(Q):                                            # the first application also returns the trace of K
            if trace:
                return prep.grm_apply(Q)
            Z, tr = prep.grm_apply(Q, return_trace=True)
            trace.append(tr)
            return Z

        out = subspace_pcs_(apply, n, int(k), so["oversample"], so["tol"], so["max_iter"], so["seed"])
        return dict(out, var_explained=out["eigenvalues"] / trace[0], p_used=int(prep.p), solver="subspace")
    finally:
        prep.close()


def covariates_with_genotype_pcs(Y, X, covariates, genotype_pcs_arg, device=0):
    """atlasqtl(genotype_pcs=): the PCs of the unresidualised standardised genotypes (pruned by the option's own ld_prune, if
    any) appended to the user's covariates.  Every check runs before the first device call.  Returns ([Z, PCs], the dict of
    genotype_pcs())."""
    n = _n_of(X)
    if np.ndim(Y) != 2 or np.shape(Y)[0] != n:
        raise AtlasqtlError("X and Y must have the same number of samples.")
    Z = _covariates_arg(covariates, n)[1]
    o = genotype_pcs_options(genotype_pcs_arg, n, 0 if Z is None else Z.shape[1])
    _ld_arg(o["ld_prune"], X)                                    # lengths of groups / positions against X
    pcs = genotype_pcs(X, o["k"], device, ld_prune=o["ld_prune"], **{key: o[key] for key in PC_SOLVER_DEFAULTS if key in o})
    return (pcs["pcs"] if Z is None else np.hstack([Z, pcs["pcs"]])), pcs
