"""Host-side pre-processing, mirroring the reference's R checks and data preparation.

Follows R/prepare_atlasqtl.R:8-124 (``prepare_data_``, ``check_verbose_``,
``check_annealing_``) and R/utils.R:10-100, 276-343 (``check_*_``,
``rm_constant_``, ``rm_collinear_``).  Error messages keep the reference's
wording so tests read like the reference's own.  The argument checks run on the host;
the O(n p) work itself -- scale(X), the removal of constant and duplicated columns,
the centring of Y -- runs on the GPU (aq_prepare_data) and X stays there: one call of aq_prepare_data_opt, the
five aq_prepare_data* entries in one, whose pipeline is csrc/aq_prepare.hip; the .bed decode, the covariates, the transform of
Y, LD pruning and the relationship matrix are the csrc/aq_prep_*.hip units.  Covariates, which the reference
does not take, are regressed out of X and Y there as well (aq_prepare_data_cov), and the compact matrix can be pruned for
linkage disequilibrium there before the fit (aq_prep_ld_prune).  The genetic relationship matrix of the prepared matrix is
formed there too (aq_prep_grm); its leading eigenvectors, the genotype principal components, are taken here on the host --
or, with solver="subspace", by subspace iteration whose operator K Q = Xs (Xs' Q) / p1 runs there (aq_prep_grm_apply) without
K ever being formed, for any n the fit takes.  The rank-based inverse normal transform of the traits (transform_y=, rank_normalize)
runs there as well, before everything else that is done to Y (aq_prepare_data_opt, aq_rank_int).
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib

_EPS75 = np.finfo(np.float64).eps ** 0.75


class AtlasqtlError(ValueError):
    """Raised where the reference calls ``stop()``."""


def check_natural_(x, name, eps=_EPS75):                      # R/utils.R:10-15
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    if np.any((x < eps) | (np.abs(x - np.round(x)) > eps)):
        raise AtlasqtlError(f"{name} must be natural.")


def check_positive_(x, name, eps=_EPS75):                     # R/utils.R:17-24
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    if np.any(x < eps):
        msg = f"{name} must be positive, greater than {eps:.3g}."
        if x.size > 1:
            msg = "All entries of " + msg
        raise AtlasqtlError(msg)


def check_zero_one_(x, name):                                 # R/utils.R:26-32
    x = np.asarray(x)
    if np.any(x < 0) or np.any(x > 1):
        msg = f"{name} must lie between 0 and 1."
        if x.size > 1:
            msg = "All entries of " + msg
        raise AtlasqtlError(msg)


def check_vector_(x, name, size=None, null_ok=False, na_ok=False):
    """check_structure_(x, "vector", ...) of R/utils.R:34-100 for numeric vectors."""
    if x is None:
        if null_ok:
            return None
        raise AtlasqtlError(f"{name} must be a non-empty a numeric vector.")
    a = np.atleast_1d(np.asarray(x, dtype=np.float64))
    ok = a.ndim == 1 and a.size > 0
    if size is not None:
        sizes = size if isinstance(size, (tuple, list)) else (size,)
        ok = ok and a.size in sizes
    if not na_ok:
        ok = ok and not np.any(np.isnan(a))
    ok = ok and bool(np.all(np.isfinite(a[~np.isnan(a)])))
    if not ok:
        raise AtlasqtlError(f"{name} must be a non-empty a numeric vector"
                            + (f" of length {size}" if size is not None else "")
                            + ", finite" + ("" if na_ok else " without missing value")
                            + (" or must be NULL" if null_ok else "") + ".")
    return a


def check_matrix_(x, name, shape=None, na_ok=False):
    """check_structure_(x, "matrix", ...) of R/utils.R:34-100."""
    a = np.asarray(x, dtype=np.float64)
    ok = a.ndim == 2 and a.size > 0
    if shape is not None:
        ok = ok and tuple(a.shape) == tuple(shape)
    if not na_ok:
        ok = ok and not np.any(np.isnan(a))
    ok = ok and bool(np.all(np.isfinite(a[~np.isnan(a)])))
    if not ok:
        raise AtlasqtlError(f"{name} must be a non-empty a numeric matrix"
                            + (f" of dimension {shape[0]} x {shape[1]}" if shape is not None else "")
                            + ", finite" + ("" if na_ok else " without missing value") + ".")
    return a


def check_verbose_(verbose):                                  # R/prepare_atlasqtl.R:90-95
    if verbose not in (0, 1, 2):
        raise AtlasqtlError("The verbose argument must be set to 0, 1 or 2.")


def check_annealing_(anneal):                                 # R/prepare_atlasqtl.R:100-124
    if anneal is None:
        return
    a = check_vector_(anneal, "anneal", size=3)
    check_natural_(a[[0, 2]], "anneal[c(1, 3)]")
    check_positive_(a[1], "anneal[2]")
    if a[0] not in (1, 2, 3):
        raise AtlasqtlError("The annealing spacing scheme must be set to 1 for geometric 2 for harmonic or 3 "
                            "for linear spacing.")
    if a[1] < 1.5:
        raise AtlasqtlError("Initial annealing temperature very small. May not be large enough for a "
                            "successful exploration. Please increase it or select no annealing.")
    if a[2] > 1000:
        raise AtlasqtlError("Temperature grid size very large. This may be unnecessarily computationally "
                            "demanding. Please decrease it.")


class PreparedData:
    """The standardised compact X (n x p) and the centred Y resident on the GPU (aq_prepare_data).  VbRun takes it in place
    of the X array; `Y` is the host copy of the centred responses (n x q, small) that the hyper-parameter rules need."""

    def __init__(self, handle, n, p, q, Y, device, genotype_counts=None, n_cov=0, cov_absorbed=None, cov_r2=None, y_n_obs=None,
                 y_n_tied=None):
        self.handle, self.n, self.p, self.q, self.Y, self.device = handle, n, p, q, Y, device
        self.shape = (n, p)
        # LD pruning (prepare_on_device(ld_prune=)), per column given: removed for LD (bool), the index of the kept column that
        # tags it (-1: none) and its r^2 with that column (NaN: not removed for LD).  None without pruning.
        self.ld_removed = self.ld_of = self.ld_r2 = None
        self.genotype_counts = genotype_counts      # 4 x p_given int32 (hom A1, het, hom A2, missing): PlinkBed input only
        # covariates regressed out of X and Y (0: none); per column given: absorbed by them (bool), and the share of its
        # variance they explain (NaN for a constant column).  None without covariates.
        self.n_cov, self.cov_absorbed, self.cov_r2 = n_cov, cov_absorbed, cov_r2
        # transform_y: per trait, its observed values and those among them that share their value with another one.  None
        # without the transform.
        self.y_n_obs, self.y_n_tied = y_n_obs, y_n_tied

    @property
    def x_ptr(self):
        return _lib.lib().aq_prep_x_device(self.handle)

    @property
    def y_ptr(self):
        return _lib.lib().aq_prep_y_device(self.handle)

    def X_host(self):
        out = np.empty((self.n, self.p), order="F")
        _lib.check(_lib.lib().aq_prep_get(self.handle, _lib.as_dp(out), None), "aq_prep_get")
        return out

    def x_moments(self, p_given):
        """The column means and n - 1 standard deviations that scale(X) used, per column given (aq_prep_info)."""
        mean = np.empty(int(p_given)); sd = np.empty(int(p_given))
        _lib.check(_lib.lib().aq_prep_info(self.handle, None, None, None, None, _lib.as_dp(mean), _lib.as_dp(sd)), "aq_prep_info")
        return mean, sd

    def ld_band(self, window):
        """r(j - 1 - b, j) of the matrix as it stands, p x window (NaN where j - 1 - b < 0): aq_prep_ld_band."""
        out = np.empty((self.p, int(window)), order="F")
        _lib.check(_lib.lib().aq_prep_ld_band(self.handle, int(window), _lib.as_dp(out)), "aq_prep_ld_band")
        return out

    def grm(self, return_trace=False):
        """The genetic relationship matrix Xs Xs' / p of the matrix as it stands, n x n and exactly symmetric: aq_prep_grm.
        return_trace: also the sum of its diagonal, added in index order."""
        import ctypes as C
        out = np.empty((self.n, self.n), order="F")
        tr = C.c_double(0.0)
        _lib.check(_lib.lib().aq_prep_grm(self.handle, _lib.as_dp(out), C.byref(tr)), "aq_prep_grm")
        return (out, float(tr.value)) if return_trace else out

    def grm_apply(self, Q, return_trace=False):
        """Z = Xs (Xs' Q) / p of the matrix as it stands, n x L for Q n x L (1 <= L <= 128), without the n x n matrix:
        aq_prep_grm_apply.  return_trace: also the trace of the relationship matrix, (sum of Xs^2) / p."""
        import ctypes as C
        Q = np.asfortranarray(Q, dtype=np.float64)
        if Q.ndim != 2 or Q.shape[0] != self.n:
            raise AtlasqtlError(f"grm_apply: Q must be n x L with n = {self.n} rows, not {Q.shape}.")
        out = np.empty(Q.shape, order="F")
        tr = C.c_double(0.0)
        _lib.check(_lib.lib().aq_prep_grm_apply(self.handle, _lib.as_dp(Q), Q.shape[1], _lib.as_dp(out),
                                                C.byref(tr) if return_trace else None), "aq_prep_grm_apply")
        return (out, float(tr.value)) if return_trace else out

    def marginal(self, r2_cut, cap, dense=False):
        """The marginal screen of the matrix as it stands against every trait: aq_prep_marginal.  r2_cut: q cutoffs on r^2
        (trait t selects r^2 >= r2_cut[t]; +inf: none); cap: rows of the table (0 only counts).  Returns dict(snp, trait, r:
        the min(n_pairs, cap) rows written, in no particular order; n_pairs: the full count; rs: selected traits per
        predictor (p); best_snp, best_r: per trait, the predictor of largest r^2 (-1 / NaN: none defined); n_undefined;
        r_dense: p x q with dense=True, else None)."""
        import ctypes as C
        cut = np.ascontiguousarray(r2_cut, dtype=np.float64)
        if cut.shape != (self.q,):
            raise AtlasqtlError(f"marginal: r2_cut must hold one cutoff per trait ({self.q}), not {cut.shape}.")
        cap = int(cap)
        rows = max(cap, 0)
        snp = np.empty(rows, dtype=np.int32); trait = np.empty(rows, dtype=np.int32); r = np.empty(rows)
        rs = np.zeros(self.p, dtype=np.int64); best_snp = np.empty(self.q, dtype=np.int32); best_r = np.empty(self.q)
        n_pairs, n_undef = C.c_int64(0), C.c_int64(0)
        r_dense = np.empty((self.p, self.q), order="F") if dense else None
        _lib.check(_lib.lib().aq_prep_marginal(self.handle, _lib.as_dp(cut), cap, _lib.as_ip(snp), _lib.as_ip(trait), _lib.as_dp(r),
                                               C.byref(n_pairs), rs.ctypes.data_as(C.POINTER(C.c_int64)), _lib.as_ip(best_snp),
                                               _lib.as_dp(best_r), C.byref(n_undef), None if r_dense is None else _lib.as_dp(r_dense)),
                   "aq_prep_marginal")
        k = min(int(n_pairs.value), rows)
        return dict(snp=snp[:k], trait=trait[:k], r=r[:k], n_pairs=int(n_pairs.value), rs=rs, best_snp=best_snp, best_r=best_r,
                    n_undefined=int(n_undef.value), r_dense=r_dense)

    def marginal_permute(self, r2_cut, perms):
        """Permutation nulls of the marginal screen: aq_prep_marginal_perm.  r2_cut: q cutoffs on r^2, as for marginal();
        perms: B x n integers, every row a permutation of 0 ... n - 1 (row b permutes the sample rows of Y: Y'[i] = Y[perms[b][i]]).
        Returns dict(max_r2: B x q, the largest defined r^2 of every trait under every permutation (-1.0: none defined);
        hs_max: B, the largest number of selected traits of one predictor; n_sel: B, selected pairs; n_undef: B)."""
        import ctypes as C
        cut = np.ascontiguousarray(r2_cut, dtype=np.float64)
        if cut.shape != (self.q,):
            raise AtlasqtlError(f"marginal_permute: r2_cut must hold one cutoff per trait ({self.q}), not {cut.shape}.")
        perms = np.asarray(perms)
        if perms.ndim != 2 or perms.shape[0] < 1 or perms.shape[1] != self.n or not np.issubdtype(perms.dtype, np.integer):
            raise AtlasqtlError(f"marginal_permute: perms must be a B x n integer array with n = {self.n}, not "
                                f"{perms.dtype} {perms.shape}.")
        if perms.size and (perms.min() < 0 or perms.max() >= self.n):       # before the cast to int32 can wrap a value
            raise AtlasqtlError(f"marginal_permute: every row of perms must be a permutation of 0 ... {self.n - 1}.")
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        B = perms.shape[0]
        max_r2 = np.empty((B, self.q))
        hs, nsel, nundef = (np.zeros(B, dtype=np.int64) for _ in range(3))
        i64 = C.POINTER(C.c_int64)
        _lib.check(_lib.lib().aq_prep_marginal_perm(self.handle, _lib.as_dp(cut), B, _lib.as_ip(perms), _lib.as_dp(max_r2),
                                                    hs.ctypes.data_as(i64), nsel.ctypes.data_as(i64), nundef.ctypes.data_as(i64)),
                   "aq_prep_marginal_perm")
        return dict(max_r2=max_r2, hs_max=hs, n_sel=nsel, n_undef=nundef)

    def _cis_windows_arg(self, s_lo, s_hi, who):
        """The windows as the library takes them: two contiguous int32 vectors of q entries with 0 <= s_lo <= s_hi <= p,
        checked before the cast to int32 can wrap a value (the library checks them again, and names the trait)."""
        lo, hi = np.asarray(s_lo), np.asarray(s_hi)
        for a in (lo, hi):
            if a.shape != (self.q,) or not np.issubdtype(a.dtype, np.integer):
                raise AtlasqtlError(f"{who}: s_lo and s_hi must hold one whole number per trait ({self.q}), not {a.dtype} {a.shape}.")
        if lo.size and (lo.min() < 0 or hi.max() > self.p or np.any(lo > hi)):
            raise AtlasqtlError(f"{who}: every window must satisfy 0 <= s_lo <= s_hi <= p = {self.p}.")
        return np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)

    def cis(self, s_lo, s_hi, r2_cut, cap):
        """The cis scan of the matrix as it stands: aq_prep_cis.  Trait t is tested against the predictors s_lo[t] <= s <
        s_hi[t] only.  r2_cut, cap: as for marginal().  Returns dict(snp, trait, r: the min(n_pairs, cap) rows written, in no
        particular order; n_pairs: the full count; best_snp, best_r: per trait, the in-window predictor of largest r^2 (-1 /
        NaN: none defined); n_undef: per trait, the undefined pairs inside its window; plan: the dict of aq_cis_plan)."""
        import ctypes as C
        lo, hi = self._cis_windows_arg(s_lo, s_hi, "cis")
        cut = np.ascontiguousarray(r2_cut, dtype=np.float64)
        if cut.shape != (self.q,):
            raise AtlasqtlError(f"cis: r2_cut must hold one cutoff per trait ({self.q}), not {cut.shape}.")
        cap = int(cap)
        rows = max(cap, 0)
        snp = np.empty(rows, dtype=np.int32); trait = np.empty(rows, dtype=np.int32); r = np.empty(rows)
        best_snp = np.empty(self.q, dtype=np.int32); best_r = np.empty(self.q); n_undef = np.zeros(self.q, dtype=np.int64)
        n_pairs, plan = C.c_int64(0), _lib.AqCisPlan()
        _lib.check(_lib.lib().aq_prep_cis(self.handle, _lib.as_ip(lo), _lib.as_ip(hi), _lib.as_dp(cut), cap, _lib.as_ip(snp),
                                          _lib.as_ip(trait), _lib.as_dp(r), C.byref(n_pairs), _lib.as_ip(best_snp), _lib.as_dp(best_r),
                                          n_undef.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(plan)), "aq_prep_cis")
        k = min(int(n_pairs.value), rows)
        return dict(snp=snp[:k], trait=trait[:k], r=r[:k], n_pairs=int(n_pairs.value), best_snp=best_snp, best_r=best_r,
                    n_undef=n_undef, plan={name: int(getattr(plan, name)) for name, _ in _lib.AqCisPlan._fields_})

    def cis_permute(self, s_lo, s_hi, perms):
        """Permutation nulls of the cis scan: aq_prep_cis_perm.  perms: B x n integers as for marginal_permute().  Returns
        max_r2, B x q: the largest defined r^2 of every trait over its window under every permutation (-1.0: none)."""
        lo, hi = self._cis_windows_arg(s_lo, s_hi, "cis_permute")
        perms = np.asarray(perms)
        if perms.ndim != 2 or perms.shape[0] < 1 or perms.shape[1] != self.n or not np.issubdtype(perms.dtype, np.integer):
            raise AtlasqtlError(f"cis_permute: perms must be a B x n integer array with n = {self.n}, not {perms.dtype} {perms.shape}.")
        if perms.size and (perms.min() < 0 or perms.max() >= self.n):       # before the cast to int32 can wrap a value
            raise AtlasqtlError(f"cis_permute: every row of perms must be a permutation of 0 ... {self.n - 1}.")
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        B = perms.shape[0]
        max_r2 = np.empty((B, self.q))
        _lib.check(_lib.lib().aq_prep_cis_perm(self.handle, _lib.as_ip(lo), _lib.as_ip(hi), B, _lib.as_ip(perms), _lib.as_dp(max_r2)),
                   "aq_prep_cis_perm")
        return max_r2

    def _cis_cond_arg(self, cond, who):
        """The conditioning lists as the library takes them, (cond_ptr [q + 1 offsets], cond_idx), int32 each: `cond` is q lists
        of at most 4 distinct column indices in [0, p), checked before the cast to int32 can wrap a value."""
        cond = list(cond)
        if len(cond) != self.q:
            raise AtlasqtlError(f"{who}: cond must hold one list per trait ({self.q}), not {len(cond)}.")
        ptr = np.zeros(self.q + 1, dtype=np.int32)
        idx = []
        for t, c in enumerate(cond):
            a = np.atleast_1d(np.asarray(c))
            if a.size == 0:
                a = np.zeros(0, dtype=np.int64)
            if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
                raise AtlasqtlError(f"{who}: the conditioning list of trait {t} must hold whole numbers, not {a.dtype} {a.shape}.")
            if a.size > 4:
                raise AtlasqtlError(f"{who}: trait {t} conditions on {a.size} variants; at most 4 are supported.")
            if a.size and (a.min() < 0 or a.max() >= self.p):
                raise AtlasqtlError(f"{who}: the conditioning list of trait {t} must hold column indices in [0, {self.p}).")
            if np.unique(a).size != a.size:
                raise AtlasqtlError(f"{who}: the conditioning list of trait {t} names a variant more than once.")
            idx += [int(v) for v in a]
            ptr[t + 1] = len(idx)
        return ptr, np.ascontiguousarray(idx + [0], dtype=np.int32)      # one spare entry: never an empty buffer

    def cis_conditional(self, s_lo, s_hi, cond, r2_cut, cap):
        """The conditional cis scan of the matrix as it stands: aq_prep_cis_cond.  s_lo, s_hi, r2_cut, cap: as for cis().
        cond: q lists, trait t is tested after the columns cond[t] (at most 4 distinct indices, in this order, inside the
        trait's window or not) have been regressed out of it and of every predictor.  Complete Y only.  Returns the dict of
        cis() with r the partial correlation, and k_eff: per trait, the columns of its list that were not collinear with the
        earlier ones (df_t = n - 2 - n_cov - k_eff[t]; 0 for a trait with an empty window); plan: the dict of
        aq_ciscond_plan, the fields of its aq_cis_plan alongside."""
        import ctypes as C
        lo, hi = self._cis_windows_arg(s_lo, s_hi, "cis_conditional")
        ptr, idx = self._cis_cond_arg(cond, "cis_conditional")
        cut = np.ascontiguousarray(r2_cut, dtype=np.float64)
        if cut.shape != (self.q,):
            raise AtlasqtlError(f"cis_conditional: r2_cut must hold one cutoff per trait ({self.q}), not {cut.shape}.")
        if np.isnan(self.Y).any():
            raise AtlasqtlError("cis_conditional: Y has missing values; the conditional scan takes complete Y only.")
        cap = int(cap)
        rows = max(cap, 0)
        snp = np.empty(rows, dtype=np.int32); trait = np.empty(rows, dtype=np.int32); r = np.empty(rows)
        best_snp = np.empty(self.q, dtype=np.int32); best_r = np.empty(self.q); n_undef = np.zeros(self.q, dtype=np.int64)
        k_eff = np.zeros(self.q, dtype=np.int32)
        n_pairs, plan = C.c_int64(0), _lib.AqCiscondPlan()
        _lib.check(_lib.lib().aq_prep_cis_cond(self.handle, _lib.as_ip(lo), _lib.as_ip(hi), _lib.as_ip(ptr), _lib.as_ip(idx),
                                               _lib.as_dp(cut), cap, _lib.as_ip(snp), _lib.as_ip(trait), _lib.as_dp(r), C.byref(n_pairs),
                                               _lib.as_ip(best_snp), _lib.as_dp(best_r), n_undef.ctypes.data_as(C.POINTER(C.c_int64)),
                                               _lib.as_ip(k_eff), C.byref(plan)), "aq_prep_cis_cond")
        k = min(int(n_pairs.value), rows)
        pd = {name: int(getattr(plan.cis, name)) for name, _ in _lib.AqCisPlan._fields_}
        pd.update({name: int(getattr(plan, name)) for name, _ in _lib.AqCiscondPlan._fields_ if name != "cis"})
        return dict(snp=snp[:k], trait=trait[:k], r=r[:k], n_pairs=int(n_pairs.value), best_snp=best_snp, best_r=best_r,
                    n_undef=n_undef, k_eff=k_eff, plan=pd)

    def cis_interaction(self, s_lo, s_hi, basis, mult, r2_cut, cap):
        """The interaction cis scan of the matrix as it stands: aq_prep_cis_int.  s_lo, s_hi, r2_cut, cap: as for cis().
        basis: nb x n, orthonormal rows spanning the intercept, the covariates the matrix was prepared with and the interaction
        variable e (cis.interaction_basis); mult: n, e centred.  Complete Y only.  Returns the dict of cis() with r the partial
        correlation of the interaction term g o e given [1, Z, e, g] (df = n - nb - 2), and int_tol: per column, the share of
        g o e that [1, Z, e, g] leave (NaN where the column is undefined for every trait); plan: the dict of aq_cisint_plan,
        the fields of its aq_cis_plan alongside."""
        import ctypes as C
        lo, hi = self._cis_windows_arg(s_lo, s_hi, "cis_interaction")
        cut = np.ascontiguousarray(r2_cut, dtype=np.float64)
        if cut.shape != (self.q,):
            raise AtlasqtlError(f"cis_interaction: r2_cut must hold one cutoff per trait ({self.q}), not {cut.shape}.")
        B = np.ascontiguousarray(basis, dtype=np.float64)
        m = np.ascontiguousarray(mult, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] < 1 or B.shape[1] != self.n or m.shape != (self.n,):
            raise AtlasqtlError(f"cis_interaction: basis must be nb x n and mult must hold n = {self.n} values, not {B.shape} and "
                                f"{m.shape}.")
        if np.isnan(self.Y).any():
            raise AtlasqtlError("cis_interaction: Y has missing values; the interaction scan takes complete Y only.")
        cap = int(cap)
        rows = max(cap, 0)
        snp = np.empty(rows, dtype=np.int32); trait = np.empty(rows, dtype=np.int32); r = np.empty(rows)
        best_snp = np.empty(self.q, dtype=np.int32); best_r = np.empty(self.q); n_undef = np.zeros(self.q, dtype=np.int64)
        int_tol = np.empty(self.p)
        n_pairs, plan = C.c_int64(0), _lib.AqCisintPlan()
        _lib.check(_lib.lib().aq_prep_cis_int(self.handle, _lib.as_ip(lo), _lib.as_ip(hi), _lib.as_dp(B), B.shape[0], _lib.as_dp(m),
                                              _lib.as_dp(cut), cap, _lib.as_ip(snp), _lib.as_ip(trait), _lib.as_dp(r), C.byref(n_pairs),
                                              _lib.as_ip(best_snp), _lib.as_dp(best_r), n_undef.ctypes.data_as(C.POINTER(C.c_int64)),
                                              _lib.as_dp(int_tol), C.byref(plan)), "aq_prep_cis_int")
        k = min(int(n_pairs.value), rows)
        pd = {name: int(getattr(plan.cis, name)) for name, _ in _lib.AqCisPlan._fields_}
        pd.update({name: int(getattr(plan, name)) for name, _ in _lib.AqCisintPlan._fields_ if name != "cis"})
        return dict(snp=snp[:k], trait=trait[:k], r=r[:k], n_pairs=int(n_pairs.value), best_snp=best_snp, best_r=best_r,
                    n_undef=n_undef, int_tol=int_tol, plan=pd)

    def close(self):
        if self.handle is not None:
            _lib.lib().aq_prep_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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
    if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, float, np.integer, np.floating)) or not (0.0 <= float(c) <= 0.5):
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
    L = _lib.lib()
    rc = L.aq_rank_int(_lib.as_dp(Ya), n, q, c, _lib.as_dp(out), _lib.as_ip(n_obs), _lib.as_ip(n_tied), int(device))
    if rc != 0:
        msg = L.aq_last_error().decode("utf-8", "replace")
        if rc == 1:
            raise AtlasqtlError(msg)
        raise _lib.AtlasqtlHipError(f"aq_rank_int: [{rc}] {msg}")
    return dict(Y=out, n_obs=n_obs, n_tied=n_tied)


def _is_whole(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def ld_prune_options(ld_prune):
    """The `ld_prune` argument of atlasqtl() / prepare_on_device with its defaults filled in and checked on the host:
    r2 in (0, 1], window a whole number in [1, 4096], window_bp None or a whole number >= 1, groups None or one label per
    predictor given, positions None or one whole number per predictor given."""
    if not isinstance(ld_prune, dict) or set(ld_prune) - set(LD_PRUNE_DEFAULTS):
        raise AtlasqtlError("ld_prune must be None or a dict with keys among 'r2', 'window', 'window_bp', 'groups', 'positions'.")
    o = {**LD_PRUNE_DEFAULTS, **ld_prune}
    r2 = o["r2"]
    if isinstance(r2, (bool, np.bool_)) or not isinstance(r2, (int, float, np.integer, np.floating)) or not (0.0 < float(r2) <= 1.0):
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
    import ctypes as C
    from .plink import PlinkBed
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
    import ctypes as C
    prep = ret[0]
    L = _lib.lib()
    p = len(ret[1])
    rc = L.aq_prep_ld_prune(prep.handle, C.byref(ld))
    if rc != 0:
        msg = L.aq_last_error().decode("utf-8", "replace")
        prep.close()
        if rc == 1:
            raise AtlasqtlError(msg)
        raise _lib.AtlasqtlHipError(f"aq_prep_ld_prune: [{rc}] {msg}")
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
    import ctypes as C
    from .plink import PlinkBed
    Y = np.asfortranarray(Y, dtype=np.float64)
    n, q = Y.shape
    cov, Z = _covariates_arg(covariates, n)
    ld, ld_arrays = _ld_arg(ld_prune, X)                       # checked here, before the first device call
    yt = _ytrans_arg(transform_y)[0]
    ret = _prepare_unpruned(Y, X, device, cov, yt)
    return ret if ld is None else _ld_prune_handle(ret, ld)


def _prepare_unpruned(Y, X, device, cov, yt=None):
    """prepare_on_device before any pruning: Y float64 in Fortran order, cov from _covariates_arg, yt from _ytrans_arg."""
    import ctypes as C
    from .plink import PlinkBed
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
    import ctypes as C
    h = C.c_void_p()
    rc = _lib.lib().aq_prepare_data_opt(None if bed else C.byref(pin), C.byref(pin) if bed else None, None if cov is None else C.byref(cov),
                                        None if yt is None else C.byref(yt), C.byref(h))
    what = "aq_prepare_data_opt" if yt is not None else "aq_prepare_data" + ("_bed" if bed else "") + ("" if cov is None else "_cov")
    return _prepared_from_handle(rc, h, what, n, p, q, device, bed=bed, cov=cov is not None, ytrans=yt is not None)


def _prepared_from_handle(rc, h, what, n, p, q, device, bed=False, cov=False, ytrans=False):
    """The return value of prepare_on_device from the handle aq_prepare_data / aq_prepare_data_bed made (or their error)."""
    import ctypes as C
    if rc != 0:
        msg = _lib.lib().aq_last_error().decode("utf-8", "replace")
        if rc == 1:
            raise AtlasqtlError(msg)                       # where the reference calls stop()
        raise _lib.AtlasqtlHipError(f"{what}: [{rc}] {msg}")
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
    import ctypes as C
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
    from .plink import PlinkBed
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
    from .plink import PlinkBed
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
    if isinstance(tol, (bool, np.bool_)) or not isinstance(tol, (int, float, np.integer, np.floating)) or not (float(tol) > 0.0) \
            or not np.isfinite(float(tol)):
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
    import warnings
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
