"""Host-side mirror of the reference's driver interface for the VB hot path.

Same names, argument meaning and error behaviour as the reference's R functions,
with the arithmetic done by libatlasqtl_hip.so on the GPU:

  atlasqtl_global_local_core_(...)             R/atlasqtl_global_local_core.R:8-433
  atlasqtl_global_core_(...)                   R/atlasqtl_global_core.R:8-366

One process drives one GPU.  With a process group (ranks.RankGroup) the trait
axis q is sharded over the ranks: each rank passes its own columns of Y and of
the q-indexed hyper-parameters / initial values; the only exchange per sweep is
one SUM all-reduce (RCCL over xGMI) of aq_vb_reduce_len(p) doubles, plus one of
8 doubles on the sweeps where the ELBO is evaluated.

The in-place operators live in operators.py and the handle-free post-processing in postproc.py; their names stay
importable from here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, prediction
from ._lib import AqVbProblem, AqVbStatus, as_dp, as_ip, check, lib
from .operators import coreDualLoop, coreDualMisLoop  # noqa: F401
from .postproc import (SPARSE_OUTPUT_DEFAULTS, _fetch_pairs, _key_to_double, assign_bFDR, associations,  # noqa: F401
                       fdr_cutoff, hotspot_sizes, merge_pair_tables, order_stats_, quantile_ranks_, radix_select_,
                       six_numbers_, six_numbers_host_, sparse_output_options, value_summary)
from .ranks import RankGroup


def _build_problem(Y, X, prep, n, p, q, q_total, list_hyper, list_init, anneal, tol, maxit, thinned_elbo_eval, debug, device,
                   world, trait_offset, scheme, df, ext_main=None, ext_elbo=None):
    """Fill an aq_vb_problem (include/atlasqtl_hip.h) from the reference's argument lists; returns (problem, objects to keep
    alive while the library reads them)."""
    pr = AqVbProblem()
    pr.n, pr.p, pr.q, pr.q_total = n, p, q, q_total
    keep = []

    def vec(v, m, name):
        a = np.asarray(v, dtype=np.float64)
        a = np.full(m, float(a)) if a.ndim == 0 else np.ascontiguousarray(a)
        if a.shape != (m,):
            raise ValueError(f"{name} must have length {m}, got {a.shape}")
        keep.append(a)
        return as_dp(a)

    def mat(v, shape, name):
        a = np.asfortranarray(v, dtype=np.float64)
        if a.shape != shape:
            raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
        keep.append(a)
        return as_dp(a)

    keep += [X, Y]
    if prep is None:
        pr.X, pr.Y = as_dp(X), as_dp(Y)
    else:
        pr.X = C.cast(prep.x_ptr, _lib.dp)
        if Y is prep.Y or (Y.shape == prep.Y.shape and np.array_equal(Y, prep.Y, equal_nan=True)):
            pr.Y, pr.xy_on_device = C.cast(prep.y_ptr, _lib.dp), 3     # the centred Y that is already on the GPU
        else:
            pr.Y, pr.xy_on_device = as_dp(Y), 1                        # another Y (e.g. one trait shard of it) from the host
    pr.A2_inv = float(list_hyper["A2_inv"]); pr.m0 = float(list_hyper["m0"])
    pr.nu = float(list_hyper["nu"]); pr.rho = float(list_hyper["rho"]); pr.t02 = float(list_hyper["t02"])
    pr.eta = vec(list_hyper["eta"], q, "eta"); pr.kappa = vec(list_hyper["kappa"], q, "kappa")
    pr.n0 = vec(list_hyper["n0"], q, "n0")
    g0, m0_ = list_init["gam_vb"], list_init["mu_beta_vb"]
    if g0 is None and m0_ is None:
        # the p x q initial values are drawn on the device (hyper_init.auto_set_init_(..., device_init=True))
        pr.init_generate = 1
        pr.init_seed = int(list_init["device_seed"]) & 0xFFFFFFFFFFFFFFFF
        pr.init_gam_mean = float(list_init["device_gam_mean"])
        pr.init_gam_sd = float(list_init["device_gam_sd"])
        pr.init_on_device = 0
    elif hasattr(g0, "data_ptr"):
        # torch CUDA tensors holding the p x q matrices column-major, i.e. a contiguous (q, p) tensor
        for tname, tt in (("gam_vb", g0), ("mu_beta_vb", m0_)):
            if not (tt.is_cuda and tt.is_contiguous() and tuple(tt.shape) == (q, p) and str(tt.dtype) == "torch.float64"):
                raise ValueError(f"{tname} on device must be a contiguous float64 CUDA tensor of shape (q, p) "
                                 "(= p x q column-major)")
        keep += [g0, m0_]
        pr.gam_vb = C.cast(g0.data_ptr(), _lib.dp)
        pr.mu_beta_vb = C.cast(m0_.data_ptr(), _lib.dp)
        pr.init_on_device = 1
    else:
        pr.gam_vb = mat(g0, (p, q), "gam_vb")
        pr.mu_beta_vb = mat(m0_, (p, q), "mu_beta_vb")
        pr.init_on_device = 0
    pr.sig02_inv_vb = float(list_init["sig02_inv_vb"])
    pr.sig2_beta_vb = vec(list_init["sig2_beta_vb"], q, "sig2_beta_vb")
    pr.sig2_theta_vb = vec(list_init["sig2_theta_vb"] if scheme != "global" else np.ones(p), p, "sig2_theta_vb")
    pr.tau_vb = vec(list_init["tau_vb"], q, "tau_vb")
    pr.theta_vb = vec(list_init["theta_vb"], p, "theta_vb")
    pr.zeta_vb = vec(list_init["zeta_vb"], q, "zeta_vb")
    pr.has_anneal = 0 if anneal is None else 1
    if anneal is not None:
        pr.anneal = (C.c_double * 3)(*[float(x) for x in anneal])
    pr.tol = float(tol); pr.maxit = int(maxit)
    pr.thinned_elbo_eval = 1 if thinned_elbo_eval else 0
    pr.debug = 1 if debug else 0
    pr.device = int(device); pr.world_size = int(world)
    pr.trait_offset = int(trait_offset)
    pr.scheme = {"global_local": 0, "global": 1}[scheme]
    pr.df = int(df)
    pr.ext_reduce_main = ext_main
    pr.ext_reduce_elbo = ext_elbo
    return pr, keep


class VbRun:
    """A device-resident VB state (aq_vb_handle).  Keeps the host arrays alive while the
    library copies them, drives the aq_vb_advance protocol and fetches results."""

    def __init__(self, Y, X, list_hyper, list_init, anneal, tol, maxit, thinned_elbo_eval=True, debug=True,
                 device=0, q_total=None, process_group=None, trait_offset=0, scheme="global_local", df=1):
        L = lib()
        prep = X if hasattr(X, "x_ptr") else None       # prepared.PreparedData: standardised X and centred Y already on the GPU
        Y = np.asfortranarray(Y, dtype=np.float64)
        if prep is None:
            X = np.asfortranarray(X, dtype=np.float64)
        n, p = X.shape
        if Y.shape[0] != n:
            raise ValueError("X and Y must have the same number of samples.")
        q = Y.shape[1]
        if prep is not None and prep.device != int(device):
            raise ValueError("PreparedData lives on another device")
        self.n, self.p, self.q, self.device = n, p, q, int(device)
        self.q_total = int(q if q_total is None else q_total)
        self.pg = process_group
        self.trait_offset = int(trait_offset)
        self.ranks = None                   # ranks.RankGroup: the collectives over the trait shards
        self.world = 1
        self._red = self._ered = None
        ext_main = ext_elbo = None
        if process_group is not None:
            self.ranks = RankGroup(process_group, device)
            self.world = self.ranks.world
            self._red = self.ranks.device_zeros(L.aq_vb_reduce_len(p))
            self._ered = self.ranks.device_zeros(8)
            ext_main, ext_elbo = self._red.data_ptr(), self._ered.data_ptr()
        pr, keep = _build_problem(Y, X, prep, n, p, q, self.q_total, list_hyper, list_init, anneal, tol, maxit, thinned_elbo_eval,
                                  debug, device, self.world, trait_offset, scheme, df, ext_main, ext_elbo)
        h = C.c_void_p()
        check(L.aq_vb_create(C.byref(pr), C.byref(h)), "aq_vb_create")
        self.h = h
        self._keep = keep

    def close(self):
        if getattr(self, "h", None):
            lib().aq_vb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def advance_until_done(self):
        """aq_vb_advance loop; all-reduces the payloads across the process group."""
        L = lib()
        while True:
            rc = L.aq_vb_advance(self.h)
            if rc < 0:
                check(-rc, "aq_vb_advance")
            if rc == _lib.AQ_VB_DONE:
                return
            self.ranks.allreduce_device(self._red if rc == _lib.AQ_VB_NEED_ALLREDUCE_MAIN else self._ered)

    def run(self):
        if self.pg is None:
            check(lib().aq_vb_run(self.h), "aq_vb_run")
        else:
            self.advance_until_done()
        return self

    def run_sweeps(self, k):
        """Run at most k further sweeps (bench.py's timed region); works with and without a process group."""
        if self.pg is None:
            check(lib().aq_vb_run_sweeps(self.h, int(k)), "aq_vb_run_sweeps")
            return
        check(lib().aq_vb_set_sweep_budget(self.h, int(k)), "aq_vb_set_sweep_budget")
        self.advance_until_done()
        check(lib().aq_vb_set_sweep_budget(self.h, -1), "aq_vb_set_sweep_budget")

    def hotspot_sizes(self, thres=0.5, fdr_adjust=False):
        """Hotspot sizes from the gam_vb resident on the device (no p x q copy to the host): rowSums(gam_vb > thres), or
        rowSums(assign_bFDR(gam_vb) < thres) with fdr_adjust (summary.atlasqtl / plot.atlasqtl,
        R/summarise_output.R:98-105,177-182).  With a process group the counts cover the traits of ALL ranks; the FDR
        ranking is global (assign_bFDR sorts all p q PPIs, R/summarise_output.R:207-223)."""
        rs = np.zeros(self.p, dtype=np.int64)
        tot = C.c_int64(0)
        if self.pg is None or not fdr_adjust:
            check(lib().aq_vb_hotspot_sizes(self.h, float(thres), int(bool(fdr_adjust)), rs.ctypes.data_as(C.POINTER(C.c_int64)),
                                            C.byref(tot)), "aq_vb_hotspot_sizes")
            if self.pg is not None:
                rs = self.ranks.sum(rs)
            return rs, int(rs.sum()) if self.pg is not None else int(tot.value)
        return self._hotspot_sizes_fdr_sharded(float(thres))

    def _hotspot_sizes_fdr_sharded(self, thres):
        """rowSums(assign_bFDR(gam_vb) < thres) over the traits of all ranks: the cutoff of `_fdr_cutoff`, counted per
        predictor by aq_vb_bfdr_rows and summed over the ranks."""
        L = lib()
        check(L.aq_vb_bfdr_begin(self.h), "aq_vb_bfdr_begin")
        try:
            rs = np.zeros(self.p, dtype=np.int64)
            cut = self._fdr_cutoff(thres)
            if cut is None:                                       # FDR of the very first entry >= thres: nothing qualifies
                return rs, 0
            upto, tie_first, take = cut
            check(L.aq_vb_bfdr_rows(self.h, upto, tie_first, take, rs.ctypes.data_as(C.POINTER(C.c_int64))), "aq_vb_bfdr_rows")
            rs = self.ranks.sum(rs)
            return rs, int(rs.sum())
        finally:
            L.aq_vb_bfdr_end(self.h)

    def _fdr_cutoff(self, thres):
        """Between aq_vb_bfdr_begin and aq_vb_bfdr_end: this rank's part (upto, tie_first, take) of the global
        {FDR < thres} set, or None when it is empty (postproc.fdr_cutoff over this handle's sorted shard)."""
        def query(c):
            out = np.zeros(5)
            check(lib().aq_vb_bfdr_query(self.h, c, as_dp(out)), "aq_vb_bfdr_query")
            return out
        return fdr_cutoff(query, self.ranks, thres)

    def associations(self, thres=0.5, fdr_adjust=False, max_pairs=None):
        """The associated (SNP, trait) pairs as a table, from the gam_vb / mu_beta_vb resident on the device (no p x q copy
        to the host): {gam_vb > thres}, or {assign_bFDR(gam_vb) < thres} with fdr_adjust (summary.atlasqtl /
        plot.atlasqtl, R/summarise_output.R:99-106).  Returns a dict of numpy arrays in the order of
        order(as.vector(gam_vb), decreasing = TRUE) -- snp, trait (0-based, trait = global index), ppi,
        beta (= gam_vb * mu_beta_vb) and fdr (= assign_bFDR at those entries) -- and n_pairs, the full count; the arrays
        are shorter only when max_pairs cut them.  With a process group every rank returns the same whole-problem table."""
        thres, fdr_adjust = float(thres), bool(fdr_adjust)
        if max_pairs is not None and int(max_pairs) < 0:
            raise ValueError("max_pairs must be None or >= 0")
        if self.pg is None or not fdr_adjust:
            tab = self._select_pairs(thres, fdr_adjust, max_pairs)
            if self.pg is None:
                return tab
            n_pairs = int(self.ranks.sum(np.array([tab["n_pairs"]], dtype=np.int64))[0])
        else:
            L = lib()
            check(L.aq_vb_bfdr_begin(self.h), "aq_vb_bfdr_begin")
            try:
                upto, tie_first, take = self._fdr_cutoff(thres) or (0, 0, 0)
                n_pairs = int(self.ranks.sum(np.array([upto + take], dtype=np.int64))[0])
                if max_pairs is not None:                     # a rank's share of the first max_pairs rows is among its own first
                    upto = min(upto, int(max_pairs))
                    take = min(take, int(max_pairs) - upto)
                m = upto + take
                tab = dict(snp=np.zeros(m, dtype=np.int32), trait=np.zeros(m, dtype=np.int32), ppi=np.zeros(m), beta=np.zeros(m))
                check(L.aq_vb_bfdr_pairs(self.h, upto, tie_first, take, as_ip(tab["snp"]), as_ip(tab["trait"]), as_dp(tab["ppi"]),
                                         as_dp(tab["beta"])), "aq_vb_bfdr_pairs")
                tab["trait"] = tab["trait"] + np.int32(self.trait_offset)
            finally:
                L.aq_vb_bfdr_end(self.h)
        return merge_pair_tables(self._gather_tables(tab), self.p, max_pairs=max_pairs, n_pairs=n_pairs)

    def _select_pairs(self, thres, fdr_adjust, max_pairs):
        """aq_vb_select_pairs on this handle, trait made global."""
        L = lib()
        tab = _fetch_pairs(lambda cap, *out: L.aq_vb_select_pairs(self.h, thres, int(fdr_adjust), cap, *out),
                           "aq_vb_select_pairs", True, max_pairs)
        tab["trait"] = tab["trait"] + np.int32(self.trait_offset)
        return tab

    def _gather_tables(self, tab):
        """Every rank's rows (snp, global trait, ppi, beta) on every rank (int32 indices travel as doubles, exactly)."""
        rows = np.column_stack([tab["snp"], tab["trait"], tab["ppi"], tab["beta"]]).astype(np.float64)
        return [dict(snp=o[:, 0].astype(np.int32), trait=o[:, 1].astype(np.int32), ppi=o[:, 2].copy(), beta=o[:, 3].copy())
                for o in self.ranks.gather_rows(rows)]

    def value_summary(self, which):
        """Min., 1st Qu., Median, Mean, 3rd Qu., Max. of all p q entries of "gam_vb" or "beta_vb" (= gam_vb * mu_beta_vb), as
        summary(as.vector(object$gam_vb)) / summary(as.vector(object$beta_vb)) of summary.atlasqtl print them
        (R/summarise_output.R:89-93), plus count and n_nan -- from the state resident on the device: a radix select
        (aq_vb_order_stats), no p x q copy and no p x q scratch.  With a process group the numbers cover the traits of ALL
        ranks: the digit histograms of the shards (aq_vb_radix_hist) are summed over the ranks, one small all-reduce per
        digit, and every rank returns the same dict."""
        L = lib()
        w = {"gam_vb": 0, "beta_vb": 1}.get(which)
        if w is None:
            raise ValueError('which must be "gam_vb" or "beta_vb"')
        mom = _lib.AqMoments()
        if self.pg is None:
            check(L.aq_vb_moments(self.h, w, C.byref(mom)), "aq_vb_moments")
            mom, stat = order_stats_(mom.count, lambda *out: L.aq_vb_order_stats(self.h, w, *out), "aq_vb_order_stats")
            return six_numbers_(mom.count, stat, mom.sum, mom.n_nan)
        check(L.aq_vb_moments(self.h, w, C.byref(mom)), "aq_vb_moments")
        count, n_nan = (int(v) for v in self.ranks.sum(np.array([mom.count, mom.n_nan], dtype=np.int64)))
        total = self.ranks.sum_in_rank_order(mom.sum)
        lo, hi = -self.ranks.max(-mom.min), self.ranks.max(mom.max)

        def hist_fn(prefixes, shift):
            pre = np.asarray(prefixes, dtype=np.uint64)
            hist = np.zeros((pre.size, 1 << _lib.AQ_RSEL_BITS), dtype=np.int64)
            check(L.aq_vb_radix_hist(self.h, w, pre.size, pre.ctypes.data_as(C.POINTER(C.c_uint64)), int(shift),
                                     hist.ctypes.data_as(C.POINTER(C.c_int64))), "aq_vb_radix_hist")
            return self.ranks.sum(hist)

        ranks = quantile_ranks_(count)
        stat = dict(zip(ranks, radix_select_(hist_fn, ranks, _lib.AQ_RSEL_BITS)))
        out = six_numbers_(count, stat, total, n_nan)
        if out["min"] != lo or out["max"] != hi:
            raise _lib.AtlasqtlHipError("value_summary: the select's extremes differ from the moments pass's")
        return out

    def get_state(self):
        """The complete loop state between two sweeps as one uint8 array (aq_vb_get_state): unlike the reference's
        write-only checkpoint_ (R/utils.R:571-611), `set_state` on a handle created for the same problem continues
        bit-identically."""
        L = lib()
        if self.status()["it"] == 0:
            self.run_sweeps(0)          # initial residual and column sums, no sweep
        nbytes = L.aq_vb_state_bytes(self.h)
        buf = np.empty(int(nbytes), dtype=np.uint8)
        check(L.aq_vb_get_state(self.h, buf.ctypes.data_as(C.c_void_p), buf.size), "aq_vb_get_state")
        return buf

    def set_state(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        check(lib().aq_vb_set_state(self.h, buf.ctypes.data_as(C.c_void_p), buf.size), "aq_vb_set_state")
        return self

    def status(self):
        st = AqVbStatus()
        check(lib().aq_vb_get_status(self.h, C.byref(st)), "aq_vb_get_status")
        out = {f[0]: getattr(st, f[0]) for f in AqVbStatus._fields_}
        buf = C.create_string_buffer(1024)
        lib().aq_vb_get_overrides(self.h, buf, 1024)
        out["overrides"] = buf.value.decode()          # AQ_* environment hooks in effect ("" = the library's own launch plan)
        return out

    def elbo_trace(self):
        cap = 4096
        its = np.zeros(cap, dtype=np.int32)
        lbs = np.zeros(cap, dtype=np.float64)
        n = lib().aq_vb_get_elbo_trace(self.h, as_ip(its), as_dp(lbs), cap)
        return its[:n].copy(), lbs[:n].copy()

    def residual(self):
        """mis_pat .* (Y - X beta_vb) as the sweep kernel carries it (n x q), see aq_vb_get_residual."""
        R = np.zeros((self.n, self.q), order="F")
        check(lib().aq_vb_get_residual(self.h, as_dp(R)), "aq_vb_get_residual")
        return R

    def predict(self, X_new, center=None, scale=None, checked=False):
        """Yhat = Xt beta_vb (n_new x q) from the gam_vb / mu_beta_vb resident on the device, read in place on the f64 matrix
        pipe (aq_vb_predict): nothing of size p q is formed, so it works where the p x q matrices never leave the GPU.
        X_new: float64 or int8, n_new rows and the p columns of the fitted (compact) matrix; Xt = (X_new - center) / scale
        per column, or X_new itself when both are None (already standardised).  Rows go to the library in batches of at
        most prediction.PREDICT_MAX_ROWS.  With a process group each rank returns the columns of its own traits.
        checked: X_new is what prediction.check_x_new returned for these p columns (the scan for non-finite values is not
        repeated)."""
        X = X_new if checked else prediction.check_x_new(X_new, self.p)
        L = lib()

        def call(xd, x8, n_rows, c, s, out):
            check(L.aq_vb_predict(self.h, xd, x8, n_rows, c, s, out), "aq_vb_predict")

        return prediction.apply_in_batches(call, X, self.q, center, scale)

    def fitted(self, prep):
        """X beta_vb (n x q), the reference's X_beta_vb, on the standardised X of the fit: a prepared.PreparedData (its matrix
        is used where it lies on the device, aq_vb_fitted) or the host matrix the run was given."""
        if not hasattr(prep, "x_ptr"):
            return self.predict(prep)
        if tuple(prep.shape) != (self.n, self.p) or prep.device != self.device:
            raise ValueError("fitted: the PreparedData is not the n x p matrix of this run on its device")
        out = np.empty((self.n, self.q), order="F")
        check(lib().aq_vb_fitted(self.h, prep.x_ptr, as_dp(out)), "aq_vb_fitted")
        return out

    def result(self, full_output=False, dense=True):
        """dense=False skips the p x q matrices (beta_vb, gam_vb, mu_beta_vb): aq_vb_get_result gets NULL for them."""
        out = _result_buffers(self.p, self.q, full_output, dense)
        nul = C.cast(None, _lib.dp)
        check(lib().aq_vb_get_result(self.h, *[as_dp(out[k]) if k in out else nul for k in RESULT_KEYS]), "aq_vb_get_result")
        return out


RESULT_KEYS = ("beta_vb", "gam_vb", "mu_beta_vb", "theta_vb", "zeta_vb", "lam2_inv_vb", "sig2_theta_vb", "tau_vb",
               "sig2_beta_vb")             # in the argument order of aq_vb_get_result


def _result_buffers(p, q, full_output, dense=True):
    """Zeroed output arrays by result key; a key that is absent is not asked for (NULL to the library): the p x q
    matrices without dense, the variational parameters beyond the reference's return list without full_output."""
    out = dict(beta_vb=np.zeros((p, q), order="F"), gam_vb=np.zeros((p, q), order="F")) if dense else {}
    out.update(theta_vb=np.zeros(p), zeta_vb=np.zeros(q))
    if full_output:
        if dense:
            out["mu_beta_vb"] = np.zeros((p, q), order="F")
        out.update(lam2_inv_vb=np.zeros(p), sig2_theta_vb=np.zeros(p), tau_vb=np.zeros(q), sig2_beta_vb=np.zeros(q))
    return out


def vb_partition(q, n_parts):
    """Trait ranges [(k0, k1)] of aq_vb_partition: whole 16-trait tiles per part."""
    out = []
    for r in range(n_parts):
        k0, k1 = C.c_int32(), C.c_int32()
        check(lib().aq_vb_partition(int(q), int(n_parts), r, C.byref(k0), C.byref(k1)), "aq_vb_partition")
        out.append((k0.value, k1.value))
    return out


PLAN_KEYS = ("core_kernel", "split_parts", "tiles_per_group", "chain_segments", "tiles_matrix", "tiles_matrix2", "tiles_recurrence",
             "instance_flags", "n_pad")


def plan_query(n, p, q, max_missing=0, max_short_list=0, ncu=256, total_bytes=-1, overrides=""):
    """The launch plan a handle for this problem would get (aq_plan_query: no device, the environment is not read): the plan
    keys of VbRun.status().  overrides: "NAME=value NAME=value" or a dict of hooks.  total_bytes: the device's memory size;
    -1 = unknown, which is enough up to n = 10240 with complete Y (with missing values it rules the MASK instances out, and
    the wide sample split beyond is refused without it)."""
    if isinstance(overrides, dict):
        overrides = " ".join(f"{k}={v}" for k, v in overrides.items())
    st = AqVbStatus()
    check(lib().aq_plan_query(int(n), int(p), int(q), int(max_missing), int(max_short_list), int(ncu), int(total_bytes),
                              (overrides or "").encode(), C.byref(st)), "aq_plan_query")
    return {k: getattr(st, k) for k in PLAN_KEYS}


def run_multi(Y, X, list_hyper, list_init, anneal, tol, maxit, n_gpus, devices=None, transport=0, thinned_elbo_eval=True,
              debug=True, scheme="global_local", df=1, full_output=True):
    """aq_vb_run_multi: the whole run on n_gpus GPUs of this node from this one process (host threads + RCCL inside the
    library; transport=1 stages the two small all-reduces through host memory and lets devices repeat).  Same result fields
    as atlasqtl_global_local_core_."""
    Y = np.asfortranarray(Y, dtype=np.float64)
    X = np.asfortranarray(X, dtype=np.float64)
    n, p = X.shape
    q = Y.shape[1]
    pr, keep = _build_problem(Y, X, None, n, p, q, q, list_hyper, list_init, anneal, tol, maxit, thinned_elbo_eval, debug,
                              0, 1, 0, scheme, df)
    out = _lib.AqVbMultiOut()
    res = _result_buffers(p, q, full_output)
    for k, v in res.items():
        setattr(out, k, as_dp(v))
    cap = 4096
    its, lbs = np.zeros(cap, dtype=np.int32), np.zeros(cap)
    out.elbo_it, out.elbo_lb, out.elbo_cap = as_ip(its), as_dp(lbs), cap
    dv = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
    if dv is not None and dv.size != n_gpus:
        raise ValueError("devices must list n_gpus ordinals")
    check(lib().aq_vb_run_multi(C.byref(pr), int(n_gpus), as_ip(dv) if dv is not None else None, int(transport), C.byref(out)),
          "aq_vb_run_multi")
    ne = min(out.n_elbo, cap)
    res.update(n=n, p=p, q=q, anneal=anneal, converged=bool(out.converged), it=int(out.it), maxit=maxit, tol=tol,
               lb_opt=out.lb_opt, diff_lb=out.diff_lb, sig02_inv_vb=out.sig02_inv_vb, sig2_inv_vb=out.sig2_inv_vb,
               elbo_trace=(its[:ne].copy(), lbs[:ne].copy()), seconds=out.seconds, core_ms=out.core_ms)
    del keep
    return res


def atlasqtl_global_core_(Y, X, shr_fac_inv, anneal, df, tol, maxit, verbose, list_hyper, list_init, checkpoint_path=None,
                          full_output=False, thinned_elbo_eval=True, debug=False, batch="y", **kw):
    """R/atlasqtl_global_core.R:8-366 on the GPU: the same sweep with ONE global scale for the hotspot propensities (no
    horseshoe local scales; df is not used by that core).  list_init needs no sig2_theta_vb."""
    return atlasqtl_global_local_core_(Y, X, shr_fac_inv, anneal, 1, tol, maxit, verbose, list_hyper, list_init,
                                       checkpoint_path=checkpoint_path, full_output=full_output,
                                       thinned_elbo_eval=thinned_elbo_eval, debug=debug, batch=batch, scheme="global", **kw)



def _run_with_checkpoints(run, checkpoint_path, rate, maxit):
    """checkpoint_ / checkpoint_clean_up_ (R/utils.R:571-627, R/atlasqtl_global_local_core.R:379,388): every `rate`
    iterations write the reference's temporary output list (tmp_output_it_<it>.npz: beta_vb, gam_vb, theta_vb, zeta_vb,
    converged, it, lb_new, diff_lb, lam2_inv_vb, sig02_inv_vb) and keep only the last two; remove them all at the end.
    Beside each, hip_state_it_<it>.npy holds the complete device state for `resume_from` (the reference cannot resume);
    they are removed as well once the run has converged (a run that is killed, or that stops at maxit, leaves its last
    two behind: that is their use)."""
    import glob
    import os
    if not os.path.isdir(checkpoint_path):
        raise ValueError("The directory specified in checkpoint_path does not exist. ")       # R/prepare_atlasqtl.R:21-22
    tag = "" if run.ranks is None else f"_rank{run.ranks.rank}"
    while True:
        st = run.status()
        if st["converged"] or st["it"] >= maxit:
            break
        run.run_sweeps(rate - st["it"] % rate)
        st = run.status()
        it = st["it"]
        if it % rate == 0 and not st["converged"]:
            res = run.result(full_output=True)
            np.savez(os.path.join(checkpoint_path, f"tmp_output_it_{it}{tag}.npz"), beta_vb=res["beta_vb"],
                     gam_vb=res["gam_vb"], theta_vb=res["theta_vb"], zeta_vb=res["zeta_vb"], converged=bool(st["converged"]),
                     it=it, lb_new=st["lb_opt"], diff_lb=st["diff_lb"], lam2_inv_vb=res["lam2_inv_vb"],
                     sig02_inv_vb=st["sig02_inv_vb"])
            np.save(os.path.join(checkpoint_path, f"hip_state_it_{it}{tag}.npy"), run.get_state())
            for stem in (f"tmp_output_it_{it - 2 * rate}{tag}.npz", f"hip_state_it_{it - 2 * rate}{tag}.npy"):
                old = os.path.join(checkpoint_path, stem)          # keep only the last two for comparison
                if os.path.exists(old):
                    os.remove(old)
    # checkpoint_clean_up_ (R/utils.R:614-627) leaves the directory clean; so do the resumable state files once the run
    # has converged (after maxit without convergence the last two stay: resume_from with a larger maxit continues them)
    pats = [f"tmp_output_it_*{tag}.npz"] + ([f"hip_state_it_*{tag}.npy"] if run.status()["converged"] else [])
    for pat in pats:
        for f in glob.glob(os.path.join(checkpoint_path, pat)):
            os.remove(f)


def atlasqtl_global_local_core_(Y, X, shr_fac_inv, anneal, df, tol, maxit, verbose, list_hyper, list_init,
                                checkpoint_path=None, trace_path=None, full_output=False, thinned_elbo_eval=True,
                                debug=False, batch="y", device=0, process_group=None, resume_from=None,
                                checkpoint_rate=100, trait_offset=None, scheme="global_local", sparse_output=None,
                                predict=None, fitted=False):
    """R/atlasqtl_global_local_core.R:8-433 on the GPU.  Returns the reference's list
    (:426-428): beta_vb, gam_vb, theta_vb, zeta_vb, n, p, q, anneal, converged, it, maxit,
    tol, lb_opt, diff_lb (+ the variational parameters with full_output).

    shr_fac_inv is the total number of traits (R/atlasqtl.R:218); with a process group each
    rank passes its own trait columns and shr_fac_inv = q of the whole problem.  trait_offset = global index of
    this rank's first trait: required with a process group when the p x q initial values are drawn on the device
    (the Philox counters are (SNP, global trait), so a sharded run reproduces the single-GPU draws).

    sparse_output = {"thres": 0.5, "fdr_adjust": False, "max_pairs": None} (missing keys take these values) returns the
    thresholded result instead of the p x q matrices: `assoc` (VbRun.associations), `rs_thres` and `nb_pairwise`
    (VbRun.hotspot_sizes), theta_vb, zeta_vb and the scalars -- no gam_vb / beta_vb / mu_beta_vb, which stay on the device.
    With "summary": True (default False) the result also holds `value_summary` = {"gam_vb": ..., "beta_vb": ...}, the six
    numbers of VbRun.value_summary that summary() prints for the p q PPIs and effect sizes, and `sparse_output`, the
    options used.

    predict = X_new, or {"X": X_new, "center": ..., "scale": ..., "checked": False}: rows of the p fitted columns (float64 or int8), already
    standardised or to be standardised by center / scale; the result then holds `predicted` = Xt beta_vb (n_new x q,
    VbRun.predict).  fitted=True: the result holds `X_beta_vb` = X beta_vb (n x q, VbRun.fitted) on the X of the run.  Both are
    taken from the state on the device before it is released, so they work with sparse_output as well; with a process group
    each rank gets the columns of its own traits."""
    sparse = None if sparse_output is None else sparse_output_options(sparse_output)
    if predict is not None:
        predict = dict(predict) if isinstance(predict, dict) else {"X": predict}
        if not predict.get("checked"):                  # atlasqtl() has checked its X_new already, in the original numbering
            predict["X"] = prediction.check_x_new(predict["X"], (X.shape if hasattr(X, "shape") else np.shape(X))[1], "predict")
    if df not in (1, 3, 5, 7):
        raise NotImplementedError("df must be 1, 3, 5 or 7 (compute_integral_hs_, R/utils.R:425-568, is unstable from df = 9 on)")
    if batch != "y":
        raise ValueError("Batch scheme not defined. Exit.")            # :231
    if trace_path is not None:
        raise NotImplementedError("trace_path (trace plots) is outside the accelerated path")
    device_init = list_init.get("gam_vb") is None and list_init.get("mu_beta_vb") is None
    if process_group is not None and device_init and trait_offset is None:
        raise ValueError("trait_offset is required with process_group when the initial values are drawn on the device: "
                         "without it every trait shard would start from the draws of traits 0..q_local-1")
    run = VbRun(Y, X, list_hyper, list_init, anneal, tol, maxit, thinned_elbo_eval, debug, device=device,
                q_total=int(shr_fac_inv), process_group=process_group, trait_offset=int(trait_offset or 0), scheme=scheme,
                df=df)
    try:
        if resume_from is not None:
            run.set_state(np.load(resume_from))
        if checkpoint_path is None:
            run.run()
        else:
            _run_with_checkpoints(run, checkpoint_path, checkpoint_rate, maxit)
        st = run.status()
        if verbose != 0:
            if st["converged"]:
                print(f"Convergence obtained after {st['it']} iterations. \nOptimal marginal log-likelihood "
                      f"variational lower bound (ELBO) = {st['lb_opt']}. \n")
            else:
                import warnings
                warnings.warn("Maximal number of iterations reached before convergence. Exit.")   # :397
        res = run.result(full_output=full_output, dense=sparse is None)
        if sparse is not None:
            res["assoc"] = run.associations(sparse["thres"], sparse["fdr_adjust"], sparse["max_pairs"])
            res["rs_thres"], res["nb_pairwise"] = run.hotspot_sizes(sparse["thres"], sparse["fdr_adjust"])
            if sparse["summary"]:
                res["value_summary"] = {"gam_vb": run.value_summary("gam_vb"), "beta_vb": run.value_summary("beta_vb")}
                res["sparse_output"] = dict(sparse)
        if predict is not None:
            res["predicted"] = run.predict(predict["X"], predict.get("center"), predict.get("scale"), checked=True)
        if fitted:
            res["X_beta_vb"] = run.fitted(X)
        its, lbs = run.elbo_trace()
        res.update(n=run.n, p=run.p, q=run.q, anneal=anneal, converged=bool(st["converged"]), it=int(st["it"]),
                   maxit=maxit, tol=tol, lb_opt=st["lb_opt"], diff_lb=st["diff_lb"])
        if full_output:
            res.update(sig02_inv_vb=st["sig02_inv_vb"], sig2_inv_vb=st["sig2_inv_vb"], elbo_trace=(its, lbs),
                       core_ms=st["core_ms"], core_launches=st["core_launches"], lentz_iters=st["lentz_iters"],
                       core_kernel=st["core_kernel"],
                       # the launched instance of the core kernel (aq_vb_status)
                       **{k: st[k] for k in ("split_parts", "tiles_matrix", "tiles_matrix2", "tiles_recurrence",
                                             "instance_flags", "n_pad")})
        return res
    finally:
        run.close()
