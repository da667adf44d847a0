"""Post-processing that reads results without a VB handle: the reference's assign_bFDR and the thresholded summaries of
summary.atlasqtl / plot.atlasqtl (R/summarise_output.R) on host matrices, and the pure host arithmetic that core.VbRun
shares with them -- the radix select's digit loop, R's six-number summary, the merge of the trait shards' pair tables and
the search for the end of the {FDR < thres} prefix over the shards.
"""
from __future__ import annotations

import ctypes as C
import math
import struct

import numpy as np

from . import _lib
from ._lib import as_dp, as_ip, check, lib


def assign_bFDR(mat_ppi, device=0):
    """assign_bFDR of the reference (R/summarise_output.R:207-223) on the GPU: sort of all p q PPIs (hipCUB radix sort,
    ties in original order), running mean of 1 - PPI, scattered back."""
    m = np.asarray(mat_ppi, dtype=np.float64)
    vec = np.ascontiguousarray(m.reshape(-1, order="F"))
    out = np.empty_like(vec)
    check(lib().aq_assign_bfdr(as_dp(vec), as_dp(out), vec.size, int(device)), "aq_assign_bfdr")
    return out.reshape(m.shape, order="F")


def hotspot_sizes(gam_vb, thres=0.5, fdr_adjust=False, device=0):
    """rs_thres and nb_pairwise of summary.atlasqtl / plot.atlasqtl (R/summarise_output.R:98-105,177-182)."""
    m = np.asfortranarray(gam_vb, dtype=np.float64)
    p, q = m.shape
    rs = np.zeros(p, dtype=np.int64)
    tot = C.c_int64(0)
    check(lib().aq_hotspot_sizes(as_dp(m), p, q, float(thres), int(bool(fdr_adjust)),
                                 rs.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(tot), int(device)), "aq_hotspot_sizes")
    return rs, int(tot.value)


def _key_to_double(key):
    """Inverse of the order-preserving key map of aq_summary.hip (negative: all bits flipped; otherwise: sign bit set)."""
    bits = key ^ (1 << 63) if key >> 63 else ~key & ((1 << 64) - 1)
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def radix_select_(hist_fn, ranks, bits=_lib.AQ_RSEL_BITS):
    """The digit loop of the radix select, for values held elsewhere (on the device, or spread over trait shards): the
    ranks[i]-th smallest values (0-based, ranks ascending), as a list of floats.
    hist_fn(prefixes, shift) -> n_prefix x 2^bits counts: for every prefix (sorted, distinct; a prefix is key >> (shift +
    bits)), the histogram of the digit (key >> shift) & (2^bits - 1) among the values with that prefix; at the top digit
    (shift + bits == 64) prefixes is [0] and all values count.  Per wanted rank the state is (prefix, rank left inside the
    prefix); per digit the bin where the cumulative count first exceeds the rank left is appended to the prefix and the
    count below it subtracted.  After the last digit the prefix is the key.  Counts are Python integers: no 2^32 limit."""
    if 64 % bits:
        raise ValueError("bits must divide 64")
    ranks = [int(r) for r in ranks]
    if any(r < 0 for r in ranks) or any(b < a for a, b in zip(ranks, ranks[1:])):
        raise ValueError("ranks must be non-negative and ascending")
    pre, rem = [0] * len(ranks), list(ranks)
    for shift in range(64 - bits, -1, -bits):
        prefixes = sorted(set(pre))
        hist = np.asarray(hist_fn(prefixes, shift))
        if hist.shape != (len(prefixes), 1 << bits):
            raise ValueError(f"hist_fn must return {len(prefixes)} x {1 << bits} counts")
        row = {pf: [int(c) for c in hist[i]] for i, pf in enumerate(prefixes)}
        for i in range(len(ranks)):
            below = 0
            for d, c in enumerate(row[pre[i]]):
                if below + c > rem[i]:
                    break
                below += c
            else:
                raise ValueError(f"rank {ranks[i]} is not below the number of values")
            rem[i] -= below
            pre[i] = (pre[i] << bits) | d
    return [_key_to_double(k) for k in pre]


_QUARTILES = (("q1", 0.25), ("median", 0.5), ("q3", 0.75))


def quantile_ranks_(count):
    """The order statistics (0-based ranks, sorted, distinct) that min, max and the type-7 quartiles of `count` values
    need: {0, N - 1} and floor / ceil of (N - 1) {1/4, 1/2, 3/4}."""
    N = int(count)
    if N < 1:
        raise ValueError("no value to summarise (all entries are NaN)")
    want = {0, N - 1}
    for _, prob in _QUARTILES:
        index = (N - 1) * prob
        want.update((int(np.floor(index)), int(np.ceil(index))))
    return sorted(want)


def six_numbers_(count, stat, total, n_nan=0):
    """R's summary.default from order statistics: stat[rank] = the rank-th smallest of the `count` values, total their
    sum.  Quartiles as stats::quantile.default, type 7 (third-party arithmetic restated): index = (N - 1) prob, lo = floor,
    hi = ceil; x[lo], unless index > lo and x[hi] != x[lo]: then (1 - h) x[lo] + h x[hi] with h = index - lo."""
    N = int(count)
    out = {"min": float(stat[0])}
    for name, prob in _QUARTILES:
        index = (N - 1) * prob
        lo, hi = int(np.floor(index)), int(np.ceil(index))
        qs = float(stat[lo])
        if index > lo and float(stat[hi]) != qs:
            h = index - lo
            qs = (1 - h) * qs + h * float(stat[hi])
        out[name] = qs
    out["mean"] = float(total) / N
    out["max"] = float(stat[N - 1])
    out.update(count=N, n_nan=int(n_nan))
    return {k: out[k] for k in ("min", "q1", "median", "mean", "q3", "max", "count", "n_nan")}


def six_numbers_host_(x):
    """six_numbers_ of a short host vector (theta_vb, the hotspot sizes: p entries), NaN left out as R leaves out NA."""
    v = np.asarray(x, dtype=np.float64).reshape(-1)
    nan = np.isnan(v)
    s = np.sort(v[~nan])
    return six_numbers_(s.size, {r: s[r] for r in quantile_ranks_(s.size)}, math.fsum(s), int(nan.sum()))


def order_stats_(count, call, what):
    """The order statistics that the six numbers of `count` values need, by one radix select on the device:
    call(n_ranks, ranks, out, moments) is aq_order_stats / aq_vb_order_stats with its leading arguments bound.  Returns the
    select's AqMoments and {rank: value}."""
    ranks = quantile_ranks_(count)
    r = np.asarray(ranks, dtype=np.int64)
    out = np.zeros(r.size)
    mom = _lib.AqMoments()
    check(call(r.size, r.ctypes.data_as(C.POINTER(C.c_int64)), as_dp(out), C.byref(mom)), what)
    return mom, dict(zip(ranks, out.tolist()))


def value_summary(x, device=0):
    """Min., 1st Qu., Median, Mean, 3rd Qu., Max. (R's summary.default; plus count and n_nan) of the entries of a host
    array of any shape -- summary(as.vector(x)) -- by the radix select on the GPU (aq_order_stats)."""
    v = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    if v.size < 1:
        raise ValueError("x has no entry")
    # NaN is left out on the device; its count is not known beforehand, so the ranks are asked for once it is
    n_nan = int(np.isnan(v).sum())
    mom, stat = order_stats_(v.size - n_nan, lambda *out: lib().aq_order_stats(as_dp(v), v.size, *out, int(device)),
                             "aq_order_stats")
    if mom.n_nan != n_nan:
        raise _lib.AtlasqtlHipError(f"aq_order_stats counted {mom.n_nan} NaN, the host {n_nan}")
    return six_numbers_(mom.count, stat, mom.sum, mom.n_nan)


def fdr_cutoff(query, ranks, thres):
    """One rank's part (upto, tie_first, take) of the global {FDR < thres} set over the trait shards, or None when the set
    is empty.  query(c) -> this rank's five numbers of aq_vb_bfdr_query (include/atlasqtl_hip.h) for the PPI value c;
    ranks: the ranks.RankGroup of the shards (every rank makes the same calls: each step is a collective).
    {FDR < thres} is a prefix of the global decreasing PPI order (the running mean of 1 - PPI never decreases along
    it).  M(c) = mean of 1 - PPI over all entries >= c is the estimated FDR at the end of c's tie block; it grows as c
    falls, so a bisection over the bit patterns of c in [0, max PPI] finds the smallest c* with M(c*) < thres: every
    entry >= c* is in.  Of the next tie block down, the first entries (original order: lower ranks, then position) are
    in for as long as the running mean stays below thres.  Every step all-reduces four numbers."""
    thres = float(thres)
    bits = lambda x: struct.unpack("<q", struct.pack("<d", x))[0]
    val = lambda b: struct.unpack("<d", struct.pack("<q", b))[0]

    def ask(c):                # local five numbers, global sums of the first four
        out = np.asarray(query(float(c)), dtype=np.float64)
        return out, ranks.sum(out[:4])

    def below(c):              # M(c) < thres, with at least one entry >= c
        _, g = ask(c)
        return g[0] > 0 and g[1] / g[0] < thres

    vmax = ranks.max(ask(2.0)[0][4])                          # the largest PPI of all
    if not below(vmax):                                       # FDR of the very first entry >= thres: nothing qualifies
        return None
    if below(0.0):
        c_star = 0.0
    else:
        lo, hi = bits(0.0), bits(vmax)                        # below(lo) false, below(hi) true
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if below(val(mid)) else (mid, hi)
        c_star = val(hi)
    loc, g = ask(c_star)
    upto = int(loc[0])                                        # this rank's entries >= c*
    n_star, s_star = float(g[0]), float(g[1])
    tie_val = ranks.max(loc[4])                               # next PPI value down, over all ranks (-1: none)
    take, tie_first = 0, upto
    if tie_val >= 0.0:
        loc_t, g_t = ask(tie_val)
        t_loc, t_glob = int(loc_t[0]) - int(loc_t[2]), int(g_t[0] - g_t[2])
        d = 1.0 - tie_val
        step_ok = lambda i: (s_star + i * d) / (n_star + i) < thres      # running mean after i entries of the block
        i = 0
        if d > thres:                                         # (else the whole block would have qualified)
            i = int(max(0, min(t_glob, np.floor((thres * n_star - s_star) / (d - thres)))))
            while i > 0 and not step_ok(i):
                i -= 1
            while i < t_glob and step_ok(i + 1):
                i += 1
        counts = ranks.gather(np.array([t_loc], dtype=np.int64))
        before = sum(int(c[0]) for c in counts[:ranks.rank])              # ties of lower ranks come first
        take = int(min(max(i - before, 0), t_loc))
    return upto, tie_first, take


def merge_pair_tables(tables, p, max_pairs=None, n_pairs=None):
    """One table from several (the trait shards' own): rows ordered by (-ppi, position j + p k of the whole matrix, i.e.
    `trait` global) as order(as.vector(gam_vb), decreasing = TRUE) orders them, and fdr = cumsum(1 - ppi) / (1:N) along
    it -- assign_bFDR (R/summarise_output.R:207-223) at those entries, because the union of the tables is a prefix of
    that order.  n_pairs: the full count when the tables were already cut to max_pairs rows each."""
    snp = np.concatenate([np.asarray(t["snp"], dtype=np.int32) for t in tables])
    trait = np.concatenate([np.asarray(t["trait"], dtype=np.int32) for t in tables])
    ppi = np.concatenate([np.asarray(t["ppi"], dtype=np.float64) for t in tables])
    beta = np.concatenate([np.asarray(t["beta"], dtype=np.float64) for t in tables])
    order = np.lexsort((snp.astype(np.int64) + int(p) * trait.astype(np.int64), -ppi))
    snp, trait, ppi, beta = snp[order], trait[order], ppi[order], beta[order]
    fdr = np.cumsum(1 - ppi) / np.arange(1, ppi.size + 1)
    m = ppi.size if max_pairs is None else min(ppi.size, int(max_pairs))
    return dict(snp=snp[:m], trait=trait[:m], ppi=ppi[:m], beta=beta[:m], fdr=fdr[:m],
                n_pairs=int(ppi.size if n_pairs is None else n_pairs))


def associations(gam_vb, beta_vb=None, thres=0.5, fdr_adjust=False, max_pairs=None, device=0):
    """The table of VbRun.associations from host matrices (gam_vb, and beta_vb for the effect sizes; without it the table
    has no `beta`): summary.atlasqtl's gam_vb > thres / assign_bFDR(gam_vb) < thres (R/summarise_output.R:99-106)."""
    m = np.asfortranarray(gam_vb, dtype=np.float64)
    p, q = m.shape
    b = None
    if beta_vb is not None:
        b = np.asfortranarray(beta_vb, dtype=np.float64)
        if b.shape != m.shape:
            raise ValueError("beta_vb must have the shape of gam_vb")
    if max_pairs is not None and int(max_pairs) < 0:
        raise ValueError("max_pairs must be None or >= 0")
    args = (as_dp(m), C.cast(None, _lib.dp) if b is None else as_dp(b), p, q, float(thres), int(bool(fdr_adjust)))
    return _fetch_pairs(lambda cap, *out: lib().aq_select_pairs(*args, cap, *out, int(device)), "aq_select_pairs",
                        b is not None, max_pairs)


def _fetch_pairs(call, what, with_beta, max_pairs):
    """Drive aq_select_pairs / aq_vb_select_pairs: call(cap, snp, trait, ppi, beta, fdr, n_pairs).  The count is not known
    beforehand, so without max_pairs the first call offers room for 65 536 rows and only a longer table costs a second call."""
    cap = (1 << 16) if max_pairs is None else int(max_pairs)
    n = C.c_int64(0)
    while True:
        tab = dict(snp=np.zeros(cap, dtype=np.int32), trait=np.zeros(cap, dtype=np.int32), ppi=np.zeros(cap), fdr=np.zeros(cap))
        if with_beta:
            tab["beta"] = np.zeros(cap)
        check(call(cap, as_ip(tab["snp"]), as_ip(tab["trait"]), as_dp(tab["ppi"]),
                   as_dp(tab["beta"]) if with_beta else C.cast(None, _lib.dp), as_dp(tab["fdr"]), C.byref(n)), what)
        if n.value <= cap or max_pairs is not None:
            break
        cap = int(n.value)
    tab = {k: v[:min(cap, n.value)].copy() for k, v in tab.items()}
    tab["n_pairs"] = int(n.value)
    return tab


SPARSE_OUTPUT_DEFAULTS = {"thres": 0.5, "fdr_adjust": False, "max_pairs": None, "summary": False}


def sparse_output_options(sparse_output):
    """The `sparse_output` argument of atlasqtl() / atlasqtl_global_local_core_ with its defaults filled in."""
    if not isinstance(sparse_output, dict) or set(sparse_output) - set(SPARSE_OUTPUT_DEFAULTS):
        raise ValueError("sparse_output must be None or a dict with keys among 'thres', 'fdr_adjust', 'max_pairs', "
                         "'summary'")
    return {**SPARSE_OUTPUT_DEFAULTS, **sparse_output}
