"""PreparedData: the handle of a prepared problem (prepare.py makes it), the standardised compact X and the centred Y
resident on the GPU, and every entry that runs on it as it stands: the copies back, the LD band, the relationship matrix and its
application, the screen family, whose six methods only marshal (marginal.py and cis.py make results of what they return), and
the fine-mapping of the cis windows with the purity of its credible sets (cis_finemap, set_purity; cis.py makes the sets).
What several of them need has one text here: _cutoff_arg, _perms_arg, _cis_windows_arg, _scan_outputs / _scan_dict, _plan_dict,
_refuse_missing_y; and so has the translation of a return code into an exception, raise_for_code.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from . import _lib
from .checks import AtlasqtlError

_i64p = C.POINTER(C.c_int64)


def raise_for_code(rc, what):
    """The one translation of an entry's return code: 0 passes, 1 is the caller's error and raises AtlasqtlError with the
    library's message (where the reference calls stop()), anything else is the library's and raises AtlasqtlHipError."""
    if rc != 0:
        msg = _lib.lib().aq_last_error().decode("utf-8", "replace")
        if rc == 1:
            raise AtlasqtlError(msg)
        raise _lib.AtlasqtlHipError(f"{what}: [{rc}] {msg}")


def _scan_outputs(q, cap):
    """What a scan over q traits writes for a table of `cap` rows (0 only counts): the rows, each trait's best predictor and
    undefined pairs, and the counter of the selected pairs; `table` and `best` are the arguments that name them, in the
    entries' order (snp, trait, r, n_pairs; best_snp, best_r)."""
    o = SimpleNamespace(cap=int(cap), snp=np.empty(max(cap, 0), dtype=np.int32), trait=np.empty(max(cap, 0), dtype=np.int32),
                        r=np.empty(max(cap, 0)), best_snp=np.empty(q, dtype=np.int32), best_r=np.empty(q),
                        n_undef=np.zeros(q, dtype=np.int64), n_pairs=C.c_int64(0))
    o.table = (_lib.as_ip(o.snp), _lib.as_ip(o.trait), _lib.as_dp(o.r), C.byref(o.n_pairs))
    o.best = (_lib.as_ip(o.best_snp), _lib.as_dp(o.best_r))
    return o


def _scan_dict(o, **more):
    """The dict a scan returns from its _scan_outputs after the call: the min(n_pairs, cap) rows written, the full count and
    each trait's best predictor, then `more`."""
    n_pairs = int(o.n_pairs.value)
    k = min(n_pairs, o.snp.shape[0])
    return dict(snp=o.snp[:k], trait=o.trait[:k], r=o.r[:k], n_pairs=n_pairs, best_snp=o.best_snp, best_r=o.best_r, **more)


def _plan_dict(plan):
    """A plan struct as a flat dict of whole numbers, the fields of a nested `cis` member (its aq_cis_plan) alongside; where
    both have a field of one name, the outer one's value stands."""
    out = _plan_dict(plan.cis) if hasattr(plan, "cis") else {}
    out.update({name: int(getattr(plan, name)) for name, _ in plan._fields_ if name != "cis"})
    return out


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
        out = np.empty((self.n, self.n), order="F")
        tr = C.c_double(0.0)
        _lib.check(_lib.lib().aq_prep_grm(self.handle, _lib.as_dp(out), C.byref(tr)), "aq_prep_grm")
        return (out, float(tr.value)) if return_trace else out

    def grm_apply(self, Q, return_trace=False):
        """Z = Xs (Xs' Q) / p of the matrix as it stands, n x L for Q n x L (1 <= L <= 128), without the n x n matrix:
        aq_prep_grm_apply.  return_trace: also the trace of the relationship matrix, (sum of Xs^2) / p."""
        Q = np.asfortranarray(Q, dtype=np.float64)
        if Q.ndim != 2 or Q.shape[0] != self.n:
            raise AtlasqtlError(f"grm_apply: Q must be n x L with n = {self.n} rows, not {Q.shape}.")
        out = np.empty(Q.shape, order="F")
        tr = C.c_double(0.0)
        _lib.check(_lib.lib().aq_prep_grm_apply(self.handle, _lib.as_dp(Q), Q.shape[1], _lib.as_dp(out),
                                                C.byref(tr) if return_trace else None), "aq_prep_grm_apply")
        return (out, float(tr.value)) if return_trace else out

    def _cutoff_arg(self, r2_cut, who):
        """The cutoffs on r^2 as the library takes them: one contiguous float64 per trait."""
        cut = np.ascontiguousarray(r2_cut, dtype=np.float64)
        if cut.shape != (self.q,):
            raise AtlasqtlError(f"{who}: r2_cut must hold one cutoff per trait ({self.q}), not {cut.shape}.")
        return cut

    def _perms_arg(self, perms, who):
        """The permutation rows as the library takes them: B x n contiguous int32 with entries in [0, n), checked before the
        cast to int32 can wrap a value (the library checks that every row is a permutation)."""
        perms = np.asarray(perms)
        if perms.ndim != 2 or perms.shape[0] < 1 or perms.shape[1] != self.n or not np.issubdtype(perms.dtype, np.integer):
            raise AtlasqtlError(f"{who}: perms must be a B x n integer array with n = {self.n}, not {perms.dtype} {perms.shape}.")
        if perms.size and (perms.min() < 0 or perms.max() >= self.n):
            raise AtlasqtlError(f"{who}: every row of perms must be a permutation of 0 ... {self.n - 1}.")
        return np.ascontiguousarray(perms, dtype=np.int32)

    def _refuse_missing_y(self, who, scan):
        if np.isnan(self.Y).any():
            raise AtlasqtlError(f"{who}: Y has missing values; the {scan} scan takes complete Y only.")

    def marginal(self, r2_cut, cap, dense=False):
        """The marginal screen of the matrix as it stands against every trait: aq_prep_marginal.  r2_cut: q cutoffs on r^2
        (trait t selects r^2 >= r2_cut[t]; +inf: none); cap: rows of the table (0 only counts).  Returns dict(snp, trait, r:
        the min(n_pairs, cap) rows written, in no particular order; n_pairs: the full count; rs: selected traits per
        predictor (p); best_snp, best_r: per trait, the predictor of largest r^2 (-1 / NaN: none defined); n_undefined;
        r_dense: p x q with dense=True, else None)."""
        cut = self._cutoff_arg(r2_cut, "marginal")
        o = _scan_outputs(self.q, int(cap))
        rs, n_undef = np.zeros(self.p, dtype=np.int64), C.c_int64(0)
        r_dense = np.empty((self.p, self.q), order="F") if dense else None
        _lib.check(_lib.lib().aq_prep_marginal(self.handle, _lib.as_dp(cut), o.cap, *o.table, rs.ctypes.data_as(_i64p), *o.best,
                                               C.byref(n_undef), None if r_dense is None else _lib.as_dp(r_dense)), "aq_prep_marginal")
        return _scan_dict(o, rs=rs, n_undefined=int(n_undef.value), r_dense=r_dense)

    def marginal_permute(self, r2_cut, perms):
        """Permutation nulls of the marginal screen: aq_prep_marginal_perm.  r2_cut: q cutoffs on r^2, as for marginal();
        perms: B x n integers, every row a permutation of 0 ... n - 1 (row b permutes the sample rows of Y: Y'[i] = Y[perms[b][i]]).
        Returns dict(max_r2: B x q, the largest defined r^2 of every trait under every permutation (-1.0: none defined);
        hs_max: B, the largest number of selected traits of one predictor; n_sel: B, selected pairs; n_undef: B)."""
        cut = self._cutoff_arg(r2_cut, "marginal_permute")
        perms = self._perms_arg(perms, "marginal_permute")
        B = perms.shape[0]
        max_r2 = np.empty((B, self.q))
        hs, nsel, nundef = (np.zeros(B, dtype=np.int64) for _ in range(3))
        _lib.check(_lib.lib().aq_prep_marginal_perm(self.handle, _lib.as_dp(cut), B, _lib.as_ip(perms), _lib.as_dp(max_r2),
                                                    hs.ctypes.data_as(_i64p), nsel.ctypes.data_as(_i64p), nundef.ctypes.data_as(_i64p)),
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
        lo, hi = self._cis_windows_arg(s_lo, s_hi, "cis")
        cut = self._cutoff_arg(r2_cut, "cis")
        o, plan = _scan_outputs(self.q, int(cap)), _lib.AqCisPlan()
        _lib.check(_lib.lib().aq_prep_cis(self.handle, _lib.as_ip(lo), _lib.as_ip(hi), _lib.as_dp(cut), o.cap, *o.table, *o.best,
                                          o.n_undef.ctypes.data_as(_i64p), C.byref(plan)), "aq_prep_cis")
        return _scan_dict(o, n_undef=o.n_undef, plan=_plan_dict(plan))

    def cis_permute(self, s_lo, s_hi, perms):
        """Permutation nulls of the cis scan: aq_prep_cis_perm.  perms: B x n integers as for marginal_permute().  Returns
        max_r2, B x q: the largest defined r^2 of every trait over its window under every permutation (-1.0: none)."""
        lo, hi = self._cis_windows_arg(s_lo, s_hi, "cis_permute")
        perms = self._perms_arg(perms, "cis_permute")
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
        lo, hi = self._cis_windows_arg(s_lo, s_hi, "cis_conditional")
        ptr, idx = self._cis_cond_arg(cond, "cis_conditional")
        cut = self._cutoff_arg(r2_cut, "cis_conditional")
        self._refuse_missing_y("cis_conditional", "conditional")
        o, plan = _scan_outputs(self.q, int(cap)), _lib.AqCiscondPlan()
        k_eff = np.zeros(self.q, dtype=np.int32)
        _lib.check(_lib.lib().aq_prep_cis_cond(self.handle, _lib.as_ip(lo), _lib.as_ip(hi), _lib.as_ip(ptr), _lib.as_ip(idx),
                                               _lib.as_dp(cut), o.cap, *o.table, *o.best, o.n_undef.ctypes.data_as(_i64p),
                                               _lib.as_ip(k_eff), C.byref(plan)), "aq_prep_cis_cond")
        return _scan_dict(o, n_undef=o.n_undef, k_eff=k_eff, plan=_plan_dict(plan))

    def cis_interaction(self, s_lo, s_hi, basis, mult, r2_cut, cap):
        """The interaction cis scan of the matrix as it stands: aq_prep_cis_int.  s_lo, s_hi, r2_cut, cap: as for cis().
        basis: nb x n, orthonormal rows spanning the intercept, the covariates the matrix was prepared with and the interaction
        variable e (cis.interaction_basis); mult: n, e centred.  Complete Y only.  Returns the dict of cis() with r the partial
        correlation of the interaction term g o e given [1, Z, e, g] (df = n - nb - 2), and int_tol: per column, the share of
        g o e that [1, Z, e, g] leave (NaN where the column is undefined for every trait); plan: the dict of aq_cisint_plan,
        the fields of its aq_cis_plan alongside."""
        lo, hi = self._cis_windows_arg(s_lo, s_hi, "cis_interaction")
        cut = self._cutoff_arg(r2_cut, "cis_interaction")
        B = np.ascontiguousarray(basis, dtype=np.float64)
        m = np.ascontiguousarray(mult, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] < 1 or B.shape[1] != self.n or m.shape != (self.n,):
            raise AtlasqtlError(f"cis_interaction: basis must be nb x n and mult must hold n = {self.n} values, not {B.shape} and "
                                f"{m.shape}.")
        self._refuse_missing_y("cis_interaction", "interaction")
        o, plan = _scan_outputs(self.q, int(cap)), _lib.AqCisintPlan()
        int_tol = np.empty(self.p)
        _lib.check(_lib.lib().aq_prep_cis_int(self.handle, _lib.as_ip(lo), _lib.as_ip(hi), _lib.as_dp(B), B.shape[0], _lib.as_dp(m),
                                              _lib.as_dp(cut), o.cap, *o.table, *o.best, o.n_undef.ctypes.data_as(_i64p),
                                              _lib.as_dp(int_tol), C.byref(plan)), "aq_prep_cis_int")
        return _scan_dict(o, n_undef=o.n_undef, int_tol=int_tol, plan=_plan_dict(plan))

    def cis_finemap(self, s_lo, s_hi, L=10, tol=1e-3, max_iter=100, scaled_prior_variance=0.2, coverage=0.95, alpha_min=1e-4,
                    active=None, cap=0, dense=False):
        """Cis fine-mapping of the matrix as it stands: aq_prep_cis_finemap, SuSiE with L single effects per trait over the
        predictors s_lo[t] <= s < s_hi[t], by IBSS on the GPU.  Complete Y only: the library refuses missing values under its
        entry's name (AtlasqtlHipError).  active: q booleans, the traits to fit (None:
        all); nothing is reported for the others (their entries below stay NaN, or 0 for the counts).  cap: rows of the table (0 only counts).
        Returns dict(snp, trait, effect, alpha, mu, mu2: the min(n_rows, cap) rows written, in no particular order -- every
        (predictor, trait, effect) with V > 0 and alpha >= min(alpha_min, 0.1 (1 - coverage) / P_t); n_rows: the full count;
        sigma2 [q]; V, lbf [q x L]; elbo [max_iter x q, NaN where the trait did not run]; n_iter, converged, n_undef [q];
        alpha_dense, mu_dense [q x L x p with dense=True, else None]; plan: the dict of aq_finemap_plan, the fields of its
        aq_cis_plan alongside)."""
        lo, hi = self._cis_windows_arg(s_lo, s_hi, "cis_finemap")
        pm = _lib.AqFinemapParams(int(L), int(max_iter), float(tol), float(scaled_prior_variance), float(coverage), float(alpha_min))
        act = None
        if active is not None:
            act = np.ascontiguousarray(np.asarray(active, dtype=bool), dtype=np.int32)
            if act.shape != (self.q,):
                raise AtlasqtlError(f"cis_finemap: active must hold one flag per trait ({self.q}), not {act.shape}.")
        q, L, cap, iters = self.q, int(L), int(cap), max(int(max_iter), 0)
        Lc = min(max(L, 0), 16)                                   # the library refuses what lies outside; no huge buffer before it does
        snp, trait, effect = (np.empty(max(cap, 0), dtype=np.int32) for _ in range(3))
        alpha, mu, mu2 = (np.empty(max(cap, 0)) for _ in range(3))
        n_rows = C.c_int64(0)
        sigma2, V, lbf = np.full(q, np.nan), np.full((q, Lc), np.nan), np.full((q, Lc), np.nan)
        elbo = np.full((iters, q), np.nan)
        n_iter, conv, n_undef = np.zeros(q, dtype=np.int32), np.zeros(q, dtype=np.int32), np.zeros(q, dtype=np.int64)
        a_dense = np.zeros((q, Lc, self.p)) if dense else None
        m_dense = np.zeros((q, Lc, self.p)) if dense else None
        plan = _lib.AqFinemapPlan()
        raise_for_code(_lib.lib().aq_prep_cis_finemap(
            self.handle, _lib.as_ip(lo), _lib.as_ip(hi), None if act is None else _lib.as_ip(act), C.byref(pm), cap, _lib.as_ip(snp),
            _lib.as_ip(trait), _lib.as_ip(effect), _lib.as_dp(alpha), _lib.as_dp(mu), _lib.as_dp(mu2), C.byref(n_rows), _lib.as_dp(sigma2),
            _lib.as_dp(V), _lib.as_dp(lbf), _lib.as_dp(elbo), _lib.as_ip(n_iter), _lib.as_ip(conv), n_undef.ctypes.data_as(_i64p),
            None if a_dense is None else _lib.as_dp(a_dense), None if m_dense is None else _lib.as_dp(m_dense), C.byref(plan)),
            "aq_prep_cis_finemap")
        k = min(int(n_rows.value), max(cap, 0))
        return dict(snp=snp[:k], trait=trait[:k], effect=effect[:k], alpha=alpha[:k], mu=mu[:k], mu2=mu2[:k], n_rows=int(n_rows.value),
                    sigma2=sigma2, V=V, lbf=lbf, elbo=elbo, n_iter=n_iter, converged=conv, n_undef=n_undef, alpha_dense=a_dense,
                    mu_dense=m_dense, plan=_plan_dict(plan))

    def set_purity(self, sets):
        """(min |r|, mean |r|) over the pairs of columns of each set, of the matrix as it stands: aq_prep_set_purity.  sets: lists
        of 1 ... 100 column indices; a set of one has purity 1."""
        sets = [np.atleast_1d(np.asarray(s, dtype=np.int64)) for s in sets]
        for b, s in enumerate(sets):
            if s.ndim != 1 or not 1 <= s.size <= 100 or s.min() < 0 or s.max() >= self.p:
                raise AtlasqtlError(f"set_purity: set {b} must hold 1 ... 100 column indices in [0, {self.p}).")
        ptr = np.zeros(len(sets) + 1, dtype=np.int32)
        ptr[1:] = np.cumsum([s.size for s in sets])
        idx = np.ascontiguousarray(np.concatenate(sets + [np.zeros(1, dtype=np.int64)]), dtype=np.int32)   # never an empty buffer
        mn, mean = np.empty(len(sets)), np.empty(len(sets))
        raise_for_code(_lib.lib().aq_prep_set_purity(self.handle, _lib.as_ip(ptr), _lib.as_ip(idx), len(sets), _lib.as_dp(mn),
                                                     _lib.as_dp(mean)), "aq_prep_set_purity")
        return mn, mean

    def close(self):
        if self.handle is not None:
            _lib.lib().aq_prep_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
