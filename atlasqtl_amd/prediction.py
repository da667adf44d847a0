"""Prediction: the fitted model applied to genotypes, Yhat = Xt beta_vb with Xt the new rows standardised by the fit's own
column means and standard deviations -- the genetic component of the responses on the scale of the prepared Y (centred;
transformed if transform_y= was used), for the samples of the fit (the X_beta_vb that the reference's man page lists and its
code never returns) or for new ones.  The product runs on the f64 matrix pipe (csrc/aq_predict.hip): from the state of a run
that is still on the GPU (core.VbRun.predict / fitted, atlasqtl(..., predict=, fitted=)), which is the only way for a
sparse_output= run whose p x q matrices never leave the device, or from a dense result that kept its standardisation
(atlasqtl(..., keep_predictor=True), then predict(res, X_new)).  The argument checks run on the host, before any device call.

Not supported: a plink.PlinkBed as X_new (decode it to int8 dosages first), and posterior predictive variances.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .checks import AtlasqtlError

# most rows of one library call (aq_vb_predict, aq_predict: AQ_N_MAX); longer matrices are looped over in batches of this many
PREDICT_MAX_ROWS = _lib.AQ_N_MAX

PLAN_KEYS = tuple(f[0] for f in _lib.AqPredictPlan._fields_)


def plan_query(n_new, p, q, ncu=256):
    """The launch plan of one prediction call (aq_predict_plan_query: no device; AQ_PREDICT_SPLITS is read as the entries
    read it)."""
    pl = _lib.AqPredictPlan()
    rc = _lib.lib().aq_predict_plan_query(int(n_new), int(p), int(q), int(ncu), C.byref(pl))
    if rc == 1:
        raise AtlasqtlError(_lib.lib().aq_last_error().decode("utf-8", "replace"))
    _lib.check(rc, "aq_predict_plan_query")
    return {k: getattr(pl, k) for k in PLAN_KEYS}


def check_x_new(X_new, n_cols, what="X_new"):
    """X_new as the library takes it: a non-empty matrix of int8 dosages (kept as int8) or of anything that converts to
    float64, with n_cols columns, finite.  Returns the array; raises AtlasqtlError with the reason."""
    from .plink import PlinkBed
    if isinstance(X_new, PlinkBed):
        raise AtlasqtlError(f"{what}: a PlinkBed is not supported for prediction; pass its dosages as an int8 or float64 matrix.")
    try:
        a = np.asarray(X_new)
        if a.dtype != np.int8:
            a = np.asarray(X_new, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise AtlasqtlError(f"{what} must be a numeric matrix (float64 or int8 dosages).") from e
    if a.ndim != 2 or a.size == 0:
        raise AtlasqtlError(f"{what} must be a non-empty numeric matrix (rows: samples, columns: the predictors given to the fit).")
    if a.shape[1] != int(n_cols):
        raise AtlasqtlError(f"{what} has {a.shape[1]} columns, but the fit was given {int(n_cols)} predictors: the columns must be "
                            "those of the X of the fit, in its original numbering.")
    if a.dtype != np.int8 and not np.isfinite(a).all():
        raise AtlasqtlError(f"{what} must be finite, without missing values (NaN): impute them first, as for the X of the fit.")
    return a


def refuse_with_covariates(what, covariates, genotype_pcs):
    """predict= / keep_predictor= cannot follow a fit on residuals."""
    if covariates is not None or genotype_pcs is not None:
        raise AtlasqtlError(f"{what} cannot be combined with covariates= or genotype_pcs=: the fit is then a fit to the residuals of "
                            "the predictors on the covariates, and new samples would need every predictor's covariate "
                            "coefficients, which are not kept.  Use fitted=True for the samples of the fit.")


def _standardisation(center, scale, p):
    if (center is None) != (scale is None):
        raise AtlasqtlError("center and scale must both be given or both be None.")
    if center is None:
        return None, None
    c = np.ascontiguousarray(center, dtype=np.float64)
    s = np.ascontiguousarray(scale, dtype=np.float64)
    if c.shape != (p,) or s.shape != (p,):
        raise AtlasqtlError(f"center and scale must hold one value per predictor ({p}).")
    return c, s


def apply_in_batches(call, X, q, center=None, scale=None):
    """Yhat (n_new x q) from call(Xb, Xb_i8, n_rows, center, scale, out) -> status, over row batches of at most
    PREDICT_MAX_ROWS rows of X (int8 or float64, checked by check_x_new)."""
    p = X.shape[1]
    c, s = _standardisation(center, scale, p)
    nul = C.cast(None, _lib.dp)
    out = np.empty((X.shape[0], int(q)), order="F")
    step = int(PREDICT_MAX_ROWS)
    for r0 in range(0, X.shape[0], step):
        Xb = np.asfortranarray(X[r0:r0 + step])
        ob = out if Xb.shape[0] == X.shape[0] else np.empty((Xb.shape[0], int(q)), order="F")
        xd, x8 = (nul, Xb.ctypes.data_as(C.POINTER(C.c_int8))) if Xb.dtype == np.int8 else (_lib.as_dp(Xb), None)
        call(xd, x8, Xb.shape[0], nul if c is None else _lib.as_dp(c), nul if s is None else _lib.as_dp(s), _lib.as_dp(ob))
        if ob is not out:
            out[r0:r0 + step] = ob
    return out


def predictor_of(bool_rmvd_x, x_mean, x_sd):
    """What a result needs to be applied to new genotypes: the kept columns (original numbering) and their standardisation."""
    kept = np.flatnonzero(~np.asarray(bool_rmvd_x, dtype=bool))
    return dict(kept_x=kept, x_center=np.ascontiguousarray(np.asarray(x_mean)[kept]), x_scale=np.ascontiguousarray(np.asarray(x_sd)[kept]),
                p_given=int(len(bool_rmvd_x)))


def predict(res, X_new, device=0):
    """Apply a dense result of atlasqtl(..., keep_predictor=True) to new genotypes on the GPU `device` (aq_predict):
    X_new is float64 or int8 with the columns that the fit was given, in its original numbering; the removed columns
    (constant, duplicate, LD-pruned) are dropped here and the rest standardised by the fit's own means and standard deviations.
    Returns n_new x q, the genetic component of the responses on the scale of the prepared Y."""
    if "beta_vb" not in res:
        raise AtlasqtlError("predict: a sparse result holds no beta_vb (its p x q matrices never left the GPU); pass predict=X_new to "
                            "the run itself, which predicts before the state is released.")
    if "predictor" not in res:
        raise AtlasqtlError("predict: the result does not carry its standardisation; run atlasqtl(..., keep_predictor=True).")
    pr = res["predictor"]
    beta = np.asfortranarray(res["beta_vb"], dtype=np.float64)
    if "names_x_all" in res or beta.shape[0] != len(pr["kept_x"]):
        raise AtlasqtlError("predict: the result went through add_collinear_back=True; the re-inserted copies of duplicated "
                            "predictors would count twice.  Fit without add_collinear_back.")
    X = check_x_new(X_new, pr["p_given"])
    Xk = X[:, pr["kept_x"]]
    p, q = beta.shape
    L = _lib.lib()

    def call(xd, x8, n_rows, c, s, out):
        _lib.check(L.aq_predict(_lib.as_dp(beta), p, q, xd, x8, n_rows, c, s, out, int(device)), "aq_predict")

    return apply_in_batches(call, Xk, q, pr["x_center"], pr["x_scale"])
