"""The host side of the cis scan, without a GPU: the ABI entries and the mirrored plan struct; the planner -- through
aq_cis_plan_query, and through the stand-alone tests/tools/cis_probe.cpp for the order of the traits, the list of work items
and the forced PB and batch, which the C ABI does not hand out; the argument errors of aq_prep_cis, aq_prep_cis_perm and
aq_prep_cis_time that come before any device call (those that need a handle's p1, q and n run under the probe's and the
query's names here, and on a real handle in tests/test_gpu_cis.py); cis_windows against a double loop; the beta approximation
by hand."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from atlasqtl_amd import _lib
from atlasqtl_amd import cis as CIS
from atlasqtl_amd.prepare import AtlasqtlError, PreparedData

GIB = 1 << 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "atlasqtl_amd", "csrc")
ENTRIES = ("aq_cis_plan_query", "aq_prep_cis", "aq_prep_cis_perm", "aq_prep_cis_time")


def test_header_binding_and_library_agree(hiplib):
    import atlasqtl_amd as A
    txt = open(os.path.join(ROOT, "include", "atlasqtl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in _lib.SYMBOLS and hasattr(hiplib, name), name
    # the argument lists: the C types of the header, in order, against the ctypes of the binding
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "aq_prep_handle": C.c_void_p, "const int32_t *": _lib.ip, "int32_t *": _lib.ip,
             "const double *": _lib.dp, "double *": _lib.dp, "int64_t *": C.POINTER(C.c_int64), "aq_cis_plan *": C.POINTER(_lib.AqCisPlan)}
    for name in ENTRIES:
        args = re.search(r"\bint " + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        types = [re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip() for a in args.split(",")]
        assert [ctype[t] for t in types] == list(_lib.SYMBOLS[name][1]), name
        assert _lib.SYMBOLS[name][0] is C.c_int
    body = re.search(r"typedef struct aq_cis_plan \{(.*?)\} aq_cis_plan;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            typ, names = decl.split(None, 1)
            fields += [(nm.strip(), {"int32_t": C.c_int32, "int64_t": C.c_int64}[typ]) for nm in names.split(",")]
    assert fields == list(_lib.AqCisPlan._fields_)
    assert C.sizeof(_lib.AqCisPlan) == 10 * 4 + 5 * 8
    assert "cis_screen" in A.__all__ and A.cis_screen is CIS.cis_screen


# ---- the planner ----
def _windows(kind, p1, q, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "empty":
        lo = rng.integers(0, p1 + 1, q)
        return lo, lo.copy()
    if kind == "all":
        return np.zeros(q, dtype=np.int64), np.full(q, p1, dtype=np.int64)
    if kind in ("w1", "w63", "w64", "w65"):
        w = min(int(kind[1:]), p1)
        lo = rng.integers(0, p1 - w + 1, q)
        return lo, lo + w
    if kind == "straddle":                             # every window crosses a multiple of 64
        m = 64 * rng.integers(1, max(2, p1 // 64), q)
        m = np.minimum(m, p1 - 1)
        return np.maximum(m - rng.integers(1, 40, q), 0), np.minimum(m + rng.integers(1, 40, q), p1)
    if kind == "one_wide":                             # narrow windows and one over everything
        lo = rng.integers(0, p1 - 3, q)
        hi = lo + rng.integers(0, 4, q)
        lo[q // 2], hi[q // 2] = 0, p1
        return lo, hi
    if kind == "mixed":                                # empty ones among the others, some at the two ends
        lo = rng.integers(0, p1, q)
        hi = np.minimum(lo + rng.integers(0, 200, q), p1)
        hi[::5] = lo[::5]
        lo[1], hi[-1] = 0, p1
        hi[1] = max(hi[1], 1)
        lo[-1] = min(lo[-1], p1 - 1)
        return lo, hi
    raise AssertionError(kind)


def _query(hiplib, n, p1, q, masked, lo, hi, n_perm=0, ncu=256):
    lo32, hi32 = np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)
    pl = _lib.AqCisPlan()
    rc = hiplib.aq_cis_plan_query(n, p1, q, masked, ncu, _lib.as_ip(lo32), _lib.as_ip(hi32), n_perm, C.byref(pl))
    return rc, pl


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/tools/cis_probe.cpp, built with the host compiler: requests in, one answer line each."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    exe = tmp_path_factory.mktemp("cis") / "cis_probe"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "tools", "cis_probe.cpp"), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def ask(lines):
        r = subprocess.run([str(exe)], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout.splitlines()
    return ask


def _request(n, p1, q, masked, lo, hi, n_perm=0, pb=0, batch=0, ncu=256):
    return (f"plan {n} {p1} {q} {masked} {ncu} {n_perm} {pb} {batch} " + ",".join(str(int(v)) for v in lo) + " " +
            ",".join(str(int(v)) for v in hi))


def _ints(field):
    field = field.strip()
    return [] if field == "-" else [int(v) for v in field.split(",")]


CASES = [(p1, q, kind) for (p1, q) in ((3, 1), (130, 130), (1000, 20), (5000, 333)) for kind in
         ("empty", "all", "w1", "w63", "w64", "w65", "straddle", "one_wide", "mixed") if not (kind in ("one_wide", "mixed") and p1 < 10)]


@pytest.mark.parametrize("p1,q,kind", CASES, ids=[f"{p}x{q}-{k}" for p, q, k in CASES])
@pytest.mark.parametrize("masked", [0, 1])
def test_plan_invariants(hiplib, probe, p1, q, kind, masked):
    n, n_perm = 200, 11
    lo, hi = _windows(kind, p1, q, seed=p1 + q)
    assert np.all((0 <= lo) & (lo <= hi) & (hi <= p1))
    ans = probe([_request(n, p1, q, masked, lo, hi, n_perm)])[0].split(" | ")
    assert ans[0] == "0", ans
    W, tiles, qa, pairs, staged, lds, perm_lds, pb, batch, launches, yp_bytes, scratch = (int(v) for v in ans[1].split())
    order, tile_lo, tile_hi, first, item_tile, item_p0 = (_ints(f) for f in ans[2:8])
    # the query on the C ABI says the same
    rc, pl = _query(hiplib, n, p1, q, masked, lo, hi, n_perm)
    assert rc == 0, hiplib.aq_last_error()
    assert (pl.n_items, pl.trait_tiles, pl.q_active, pl.window_pairs, pl.staged_pairs, pl.lds_bytes, pl.perm_lds_bytes, pl.pb, pl.batch,
            pl.launches, pl.yp_bytes, pl.scratch_bytes) == (W, tiles, qa, pairs, staged, lds, perm_lds, pb, batch, launches, yp_bytes, scratch)
    assert (pl.tile, pl.sample_chunk, pl.masked) == (64, 16, masked)
    # order: a permutation, the non-empty windows first by (s_lo, s_hi, t), the empty ones last
    assert sorted(order) == list(range(q))
    width = hi - lo
    assert qa == int((width > 0).sum()) and all(width[t] > 0 for t in order[:qa]) and all(width[t] == 0 for t in order[qa:])
    keys = [(int(lo[t]), int(hi[t]), t) for t in order[:qa]]
    assert keys == sorted(keys)
    assert order[qa:] == sorted(order[qa:])
    # tiles and their items
    assert tiles == -(-qa // 64) == len(tile_lo) == len(tile_hi) and len(first) == tiles + 1
    assert W == len(item_tile) == len(item_p0) and first[0] == 0 and first[-1] == W
    for k in range(tiles):
        members = order[64 * k:min(64 * k + 64, qa)]
        assert tile_lo[k] == min(lo[t] for t in members) and tile_hi[k] == max(hi[t] for t in members)
        items = range(first[k], first[k + 1])
        assert [item_tile[w] for w in items] == [k] * len(items)                       # contiguous
        assert [item_p0[w] for w in items] == list(range(tile_lo[k], tile_hi[k], 64))    # ascending, no gap, no overlap
        assert len(items) >= 1
    # every in-window pair lies in exactly one work item
    seen = np.zeros((p1, q), dtype=np.int32)
    for w in range(W):
        members = order[64 * item_tile[w]:min(64 * item_tile[w] + 64, qa)]
        for t in members:
            a, b = max(item_p0[w], lo[t]), min(item_p0[w] + 64, hi[t])
            if b > a:
                seen[a:b, t] += 1
    want = np.zeros((p1, q), dtype=np.int32)
    for t in range(q):
        want[lo[t]:hi[t], t] = 1
    np.testing.assert_array_equal(seen, want)
    assert pairs == int(width.sum()) <= staged == 64 * 64 * W
    if kind == "all":
        assert W == -(-p1 // 64) * -(-q // 64)
    if kind == "empty":
        assert (W, tiles, qa, pairs) == (0, 0, 0, 0)
    # LDS of the two kernels, and the batch rules of the permutations
    streams = 2 if masked else 1
    assert lds == (1 + streams) * 64 * 18 * 8 + 2 * 64 * 12 + 64 * 32 <= 65536
    assert perm_lds == (1 + streams * pb) * 64 * 18 * 8 + 64 * 24 + 2 * pb * 64 * 8 <= 65536
    assert pb == (1 if masked else 2) and batch >= pb and batch % pb == 0
    panel, per = 8 * max(qa, 1) * n, 16 * q + 4 * n
    assert yp_bytes == batch * panel <= GIB and batch * per <= GIB
    assert scratch == 12 * 64 * W + batch * per
    assert launches * batch >= n_perm > (launches - 1) * batch
    assert max(W, 1) * (batch // pb) < 2 ** 31
    assert batch == -(-n_perm // pb) * pb                        # small panels: one launch holds what was asked for
    # the scan alone
    rc, pl0 = _query(hiplib, n, p1, q, masked, lo, hi, 0)
    assert rc == 0 and (pl0.pb, pl0.batch, pl0.launches, pl0.perm_lds_bytes, pl0.yp_bytes) == (0, 0, 0, 0, 0)
    assert pl0.n_items == W and pl0.scratch_bytes == 12 * 64 * W


def test_plan_batches_at_a_large_shape(hiplib):
    """n = 1000, q = 10 000: a panel is 80 MB, 13 fit in 1 GiB: 12 with PB = 2, 13 with PB = 1 (masked)."""
    p1, q, n = 50000, 10000, 1000
    rng = np.random.default_rng(1)
    lo = rng.integers(0, p1 - 500, q)
    hi = lo + 500
    rc, pl = _query(hiplib, n, p1, q, 0, lo, hi, 1000)
    assert rc == 0 and (pl.pb, pl.batch, pl.launches) == (2, 12, 84) and pl.yp_bytes == 12 * 8 * q * n <= GIB
    rc, pm = _query(hiplib, n, p1, q, 1, lo, hi, 1000)
    assert rc == 0 and (pm.pb, pm.batch, pm.launches) == (1, 13, 77)
    assert pl.window_pairs == 500 * q and pl.n_items == pm.n_items and pl.window_pairs <= pl.staged_pairs
    assert pl.staged_pairs < 0.2 * ((p1 + 63) // 64) * ((q + 63) // 64) * 4096      # the band, not the matrix
    # traits without a window are not gathered: half the traits, half the panel, twice the batch
    hi2 = hi.copy()
    hi2[::2] = lo[::2]
    rc, ph = _query(hiplib, n, p1, q, 1, lo, hi2, 1000)
    assert rc == 0 and ph.q_active == q // 2 and ph.batch == 26


def test_forced_plan_fields(probe):
    n, p1, q = 50, 130, 67
    lo, hi = _windows("mixed", p1, q, 3)
    ok = {(0, 1): 20992, (0, 2): 31232, (0, 4): 51712, (1, 1): 30208, (1, 2): 49664}
    got = probe([_request(n, p1, q, m, lo, hi, 5, pb, 0) for (m, pb) in ok])
    for line, ((m, pb), lds) in zip(got, ok.items()):
        f = line.split(" | ")[1].split()
        assert line.startswith("0 | ") and [int(f[6]), int(f[7]), int(f[8]), int(f[9])] == [lds, pb, -(-5 // pb) * pb, 1], (m, pb, line)
    got = probe([_request(n, p1, q, 0, lo, hi, 5, 2, 2), _request(n, p1, q, 0, lo, hi, 5, 4, 4), _request(n, p1, q, 1, lo, hi, 5, 1, 2),
                 _request(n, p1, q, 0, lo, hi, 5, 0, 2)])
    assert [g.split(" | ")[1].split()[7:10] for g in got] == [["2", "2", "3"], ["4", "4", "2"], ["1", "2", "3"], ["2", "2", "3"]]
    bad = probe([_request(n, p1, q, 0, lo, hi, 5, 3, 0), _request(n, p1, q, 1, lo, hi, 5, 4, 0), _request(n, p1, q, 0, lo, hi, 5, -1, 0),
                 _request(n, p1, q, 0, lo, hi, 5, 2, 3), _request(n, p1, q, 0, lo, hi, 5, 2, -1), _request(n, p1, q, 0, lo, hi, 5, 2, 8)])
    for line in bad[:3]:
        assert line.startswith("1 | probe: AQ_CIS_PB"), line
    for line in bad[3:]:                                               # no multiple of PB; no number; beyond the permutations asked for
        assert line.startswith("1 | probe: AQ_CIS_BATCH"), line
    # forced fields are not looked at without permutations
    assert probe([_request(n, p1, q, 0, lo, hi, 0, 3, 7)])[0].startswith("0 | ")


def test_plan_refusals(hiplib, probe):
    pl = _lib.AqCisPlan()
    lo, hi = np.zeros(5, dtype=np.int32), np.full(5, 10, dtype=np.int32)
    assert hiplib.aq_cis_plan_query(100, 10, 5, 0, 256, _lib.as_ip(lo), _lib.as_ip(hi), 0, None) == 1
    assert b"aq_cis_plan_query: NULL argument" in hiplib.aq_last_error()
    assert hiplib.aq_cis_plan_query(100, 10, 5, 0, 256, None, _lib.as_ip(hi), 0, C.byref(pl)) == 1
    assert b"aq_cis_plan_query: NULL s_lo or s_hi" in hiplib.aq_last_error()
    assert hiplib.aq_cis_plan_query(100, 10, 5, 0, 256, _lib.as_ip(lo), None, 0, C.byref(pl)) == 1
    assert b"aq_cis_plan_query: NULL s_lo or s_hi" in hiplib.aq_last_error()
    for bad in [(0, 10, 5, 0, 256, 0), (100, 0, 5, 0, 256, 0), (100, 10, 0, 0, 256, 0), (100, 10, 5, 2, 256, 0), (100, 10, 5, -1, 256, 0),
                (100, 10, 5, 0, 0, 0), (100, 10, 5, 0, 256, -1)]:
        assert hiplib.aq_cis_plan_query(*bad[:5], _lib.as_ip(lo), _lib.as_ip(hi), bad[5], C.byref(pl)) == 1, bad
        assert b"aq_cis_plan_query" in hiplib.aq_last_error()
    # the windows: what aq_prep_cis, aq_prep_cis_perm and aq_prep_cis_time check with the handle's p1 and q, by the same function
    for blo, bhi, msg in (([0, 0, 11, 0, 0], [10] * 5, b"the window of trait 2, [11, 10), is outside [0, 10]"),
                          ([0] * 5, [10, 10, 10, 11, 10], b"the window of trait 3, [0, 11), is outside [0, 10]"),
                          ([0, -1, 0, 0, 0], [10] * 5, b"the window of trait 1, [-1, 10), is outside [0, 10]"),
                          ([0, 0, 0, 0, 7], [10, 10, 10, 10, 6], b"s_lo > s_hi for trait 4 (7 > 6)")):
        rc, pl = _query(hiplib, 100, 10, 5, 0, blo, bhi)
        assert rc == 1 and b"aq_cis_plan_query: " + msg in hiplib.aq_last_error(), hiplib.aq_last_error()
        assert bytes(pl) == bytes(C.sizeof(pl))                      # nothing but zeroes on failure
        assert probe([_request(100, 10, 5, 0, blo, bhi)])[0] == "1 | probe: " + msg.decode()
    # one panel above 1 GiB; more work items than the grid holds
    rc, _ = _query(hiplib, 82944, 1000, 2000, 0, [0] * 2000, [1000] * 2000, 10)
    assert rc == 3 and b"1 GiB" in hiplib.aq_last_error()
    assert _query(hiplib, 82944, 1000, 2000, 0, [0] * 2000, [1000] * 2000, 0)[0] == 0      # the scan alone gathers one ordered copy
    q, p1 = 1 << 18, (1 << 31) - 1                                       # 4096 trait tiles x 2^25 items each = 2^37
    rc, _ = _query(hiplib, 100, p1, q, 0, np.zeros(q, dtype=np.int32), np.full(q, p1, dtype=np.int32), 0)
    assert rc == 3 and b"work items exceed the grid" in hiplib.aq_last_error()


def test_argument_errors_need_no_gpu(hiplib):
    lo, hi = np.zeros(3, dtype=np.int32), np.ones(3, dtype=np.int32)
    cut = np.zeros(3)
    perm = np.arange(4, dtype=np.int32)[None, :]
    L, ilo, ihi, icut, iperm = hiplib, _lib.as_ip(lo), _lib.as_ip(hi), _lib.as_dp(cut), _lib.as_ip(perm)
    i64 = C.POINTER(C.c_int64)
    outs = (None, None, None, C.cast(None, i64), None, None, C.cast(None, i64), None)
    for args in ((None, None, ihi, icut, 0), (None, ilo, None, icut, 0), (None, ilo, ihi, None, 0)):
        assert L.aq_prep_cis(*args, *outs) == 1
        assert b"aq_prep_cis: NULL s_lo, s_hi or r2_cut" in L.aq_last_error()
    assert L.aq_prep_cis(None, ilo, ihi, icut, -1, *outs) == 1
    assert b"aq_prep_cis: cap >= 0 required, -1 given" in L.aq_last_error()
    assert L.aq_prep_cis(None, ilo, ihi, icut, 0, *outs) == 1
    assert b"aq_prep_cis: NULL handle" in L.aq_last_error()
    for bad in (0, -2):
        assert L.aq_prep_cis_perm(None, ilo, ihi, bad, iperm, None) == 1
        assert b"aq_prep_cis_perm: n_perm >= 1 required" in L.aq_last_error()
    for args in ((None, ihi, 1, iperm), (ilo, None, 1, iperm), (ilo, ihi, 1, None)):
        assert L.aq_prep_cis_perm(None, *args, None) == 1
        assert b"aq_prep_cis_perm: NULL s_lo, s_hi or perm" in L.aq_last_error()
    assert L.aq_prep_cis_perm(None, ilo, ihi, 1, iperm, None) == 1
    assert b"aq_prep_cis_perm: NULL handle" in L.aq_last_error()
    ms = (C.c_double(0.0), C.c_double(0.0))
    assert L.aq_prep_cis_time(None, None, ihi, 0, 1, C.byref(ms[0]), C.byref(ms[1]), None) == 1
    assert b"aq_prep_cis_time: NULL argument" in L.aq_last_error()
    assert L.aq_prep_cis_time(None, ilo, ihi, 0, 1, None, C.byref(ms[1]), None) == 1
    assert b"aq_prep_cis_time: NULL argument" in L.aq_last_error()
    for n_perm, reps in ((-1, 1), (0, 0)):
        assert L.aq_prep_cis_time(None, ilo, ihi, n_perm, reps, C.byref(ms[0]), C.byref(ms[1]), None) == 1
        assert b"aq_prep_cis_time: n_perm >= 0 and reps >= 1 required" in L.aq_last_error()
    assert L.aq_prep_cis_time(None, ilo, ihi, 0, 1, C.byref(ms[0]), C.byref(ms[1]), None) == 1
    assert b"aq_prep_cis_time: NULL handle" in L.aq_last_error()


def test_wrapper_refuses_windows_and_rows_before_the_library():
    prep = PreparedData(None, 4, 10, 2, np.zeros((4, 2)), 0)
    for lo, hi in (([0], [1]), ([0, 0, 0], [1, 1, 1]), ([0.0, 0.0], [1.0, 1.0])):
        with pytest.raises(AtlasqtlError, match="one whole number per trait"):
            prep.cis(np.array(lo), np.array(hi), np.zeros(2), 0)
    for lo, hi in (([0, -1], [1, 1]), ([0, 0], [1, 11]), ([0, 5], [1, 4]), ([0, 0], [1, 2 ** 32 + 1])):
        with pytest.raises(AtlasqtlError, match="0 <= s_lo <= s_hi <= p = 10"):
            prep.cis(np.array(lo), np.array(hi), np.zeros(2), 0)
        with pytest.raises(AtlasqtlError, match="0 <= s_lo <= s_hi <= p = 10"):
            prep.cis_permute(np.array(lo), np.array(hi), np.arange(4)[None, :])
    with pytest.raises(AtlasqtlError, match="one cutoff per trait"):
        prep.cis(np.array([0, 0]), np.array([1, 1]), np.zeros(3), 0)
    with pytest.raises(AtlasqtlError, match="B x n integer array"):
        prep.cis_permute(np.array([0, 0]), np.array([1, 1]), np.arange(5)[None, :])
    with pytest.raises(AtlasqtlError, match="permutation of 0 ... 3"):
        prep.cis_permute(np.array([0, 0]), np.array([1, 1]), np.array([[0, 1, 2, 4]]))


def test_cis_screen_refuses_bad_arguments_before_the_device():
    X, Y = np.zeros((6, 3)), np.zeros((6, 2))
    pos = dict(trait_chrom=["1", "1"], trait_start=[5, 6], snp_chrom=["1"] * 3, snp_pos=[1, 2, 3])
    with pytest.raises(AtlasqtlError, match="cis_screen: at most one of p_value and fdr"):
        CIS.cis_screen(Y, X, p_value=0.1, fdr=0.1, **pos)
    with pytest.raises(AtlasqtlError, match="permutation"):
        CIS.cis_screen(Y, X, permutations=0, **pos)
    with pytest.raises(AtlasqtlError, match="window must be a whole number"):
        CIS.cis_screen(Y, X, window=-1, **pos)
    with pytest.raises(AtlasqtlError, match="snp_chrom and snp_pos are required"):
        CIS.cis_screen(Y, X, ["1", "1"], [5, 6])
    with pytest.raises(AtlasqtlError, match="one value per predictor given"):
        CIS.cis_screen(Y, X, ["1", "1"], [5, 6], snp_chrom=["1"] * 2, snp_pos=[1, 2, 3])


# ---- cis_windows ----
def _brute_windows(chrom, pos, tchrom, start, end, window):
    """The definition by a double loop: the set of predictors of every trait; (0, 0) when it is empty."""
    lo, hi = [], []
    for t in range(len(tchrom)):
        inside = [s for s in range(len(chrom)) if str(chrom[s]) == str(tchrom[t]) and start[t] - window <= pos[s] <= end[t] + window]
        if inside:
            assert inside == list(range(inside[0], inside[-1] + 1))
        lo.append(inside[0] if inside else None)
        hi.append(inside[-1] + 1 if inside else None)
    return lo, hi


def _same_windows(got, want):
    for t, (a, b) in enumerate(zip(*want)):
        if a is None:
            assert got[0][t] == got[1][t], t                              # empty, wherever it lies
        else:
            assert (got[0][t], got[1][t]) == (a, b), t


def test_cis_windows_against_a_double_loop():
    rng = np.random.default_rng(4)
    chrom = ["1"] * 40 + ["2"] * 25 + ["X"] * 35
    pos = np.concatenate([np.sort(rng.integers(0, 5000, m)) for m in (40, 25, 35)])
    pos[5] = pos[6]                                                       # equal positions are in order
    q = 60
    tchrom = [("1", "2", "X", "7")[i] for i in rng.integers(0, 4, q)]     # "7": a chromosome without predictors
    start = rng.integers(-500, 5500, q)
    end = start + rng.integers(0, 300, q)
    for window in (0, 1, 137, 10 ** 6):
        got = CIS.cis_windows(chrom, pos, tchrom, start, end, window)
        assert got[0].dtype == got[1].dtype == np.int32 and got[0].shape == (q,)
        _same_windows(got, _brute_windows(chrom, pos, tchrom, start, end, window))
        _same_windows(CIS.cis_windows(chrom, pos, tchrom, start, None, window), _brute_windows(chrom, pos, tchrom, start, start, window))
    for t in range(q):
        if tchrom[t] == "7":
            assert got[0][t] == got[1][t] == 0
    wide = CIS.cis_windows(chrom, pos, ["2"], [0], window=10 ** 6)
    assert (wide[0][0], wide[1][0]) == (40, 65)
    # window 0 with trait_end: exactly the predictors inside the gene; a position hit exactly is inside on both sides
    g = CIS.cis_windows(chrom, pos, ["1"], [int(pos[10])], [int(pos[20])], 0)
    assert g[0][0] <= 10 and g[1][0] >= 21 and np.all(pos[g[0][0]:g[1][0]] >= pos[10]) and np.all(pos[g[0][0]:g[1][0]] <= pos[20])
    # predictors removed from the middle (what a preparation does): the windows over the kept columns
    kept = np.ones(100, dtype=bool)
    kept[[3, 4, 41, 50, 51, 52, 99]] = False
    ck, pk = [c for c, k in zip(chrom, kept) if k], pos[kept]
    _same_windows(CIS.cis_windows(ck, pk, tchrom, start, end, 137), _brute_windows(ck, pk, tchrom, start, end, 137))
    # integer chromosome labels compare as their strings
    _same_windows(CIS.cis_windows([1] * 40 + [2] * 25 + ["X"] * 35, pos, tchrom, start, end, 137),
                  _brute_windows(chrom, pos, tchrom, start, end, 137))


def test_cis_windows_refusals():
    with pytest.raises(AtlasqtlError, match="positions on chromosome 1 decrease at column 2"):
        CIS.cis_windows(["1", "1", "1", "2"], [10, 20, 19, 5], ["1"], [15])
    with pytest.raises(AtlasqtlError, match="chromosome 1 are not contiguous: column 3 "):
        CIS.cis_windows(["1", "1", "2", "1", "2"], [10, 20, 5, 30, 6], ["1"], [15])
    with pytest.raises(AtlasqtlError, match="one value per predictor"):
        CIS.cis_windows(["1", "1"], [10, 20, 30], ["1"], [15])
    with pytest.raises(AtlasqtlError, match="one value per trait"):
        CIS.cis_windows(["1", "1"], [10, 20], ["1", "1"], [15])
    with pytest.raises(AtlasqtlError, match="trait_end < trait_start for trait 1"):
        CIS.cis_windows(["1", "1"], [10, 20], ["1", "1"], [15, 15], [16, 14])
    for bad in (-1, 2.5, "1000", True):
        with pytest.raises(AtlasqtlError, match="window must be a whole number"):
            CIS.cis_windows(["1", "1"], [10, 20], ["1"], [15], window=bad)


# ---- the beta approximation ----
def test_beta_approximation_by_hand():
    from scipy.stats import beta, t as student
    max_r2 = np.array([[0.10, 0.30, 0.02, -1.0, 0.2],
                       [0.05, 0.20, 0.02, -1.0, 0.1],
                       [0.20, 0.25, 0.02, -1.0, -1.0],
                       [0.08, 0.40, 0.02, -1.0, 0.3]])
    df = np.array([28, 18, 28, 28, 28])
    best_p = np.array([1e-3, 0.04, 0.5, np.nan, 0.01])
    s1, s2, pv = CIS.beta_approximation(max_r2, df, best_p)
    for t in (0, 1):
        pb = []
        for b in range(4):
            r2 = max_r2[b, t]
            tt = np.sqrt(r2) * np.sqrt(df[t] / (1.0 - r2))
            pb.append(2.0 * student.sf(tt, df[t]))
        m = sum(pb) / 4
        v = sum((x - m) ** 2 for x in pb) / 3
        a = m * (m * (1 - m) / v - 1)
        b2 = a * (1 / m - 1)
        assert a > 0 and b2 > 0
        np.testing.assert_allclose([s1[t], s2[t]], [a, b2], rtol=1e-12)
        np.testing.assert_allclose(pv[t], beta(a, b2).cdf(best_p[t]), rtol=1e-12)
        assert 0 < pv[t] < 1
    # v = 0 (every permutation the same); no defined pair; a permutation without a defined pair: NaN in all three
    for t in (2, 3, 4):
        assert np.isnan(s1[t]) and np.isnan(s2[t]) and np.isnan(pv[t]), t
    # B < 2
    for out in CIS.beta_approximation(max_r2[:1], df, best_p):
        assert np.isnan(out).all()
    # a shape <= 0: the p_b at the two ends of (0, 1), a variance above m (1 - m)
    ends = np.array([[1e-12], [0.999999], [1e-12], [0.999999]])
    assert all(np.isnan(out[0]) for out in CIS.beta_approximation(ends, np.array([30]), np.array([0.1])))


def test_permutation_summary_by_hand():
    from scipy.stats import t as student
    max_r2 = np.array([[0.25, 0.10, -1.0], [0.09, 0.30, -1.0], [0.04, 0.05, -1.0], [0.25, 0.01, -1.0]])
    best_r = np.array([-0.5, 0.6, np.nan])             # r^2 = 0.25 (tied with two permutations: >= counts them), 0.36 (none)
    best_snp = np.array([2, 0, -1])
    df = np.array([20, 20, 20])
    best_p = np.array([2 * student.sf(0.5 * np.sqrt(20 / 0.75), 20), 2 * student.sf(0.6 * np.sqrt(20 / 0.64), 20), np.nan])
    s = CIS.cis_permutation_summary(max_r2, best_snp, best_r, best_p, df)
    assert set(s) == {"trait_pvalue", "beta_shape1", "beta_shape2", "trait_pvalue_beta", "trait_qvalue"}
    np.testing.assert_array_equal(s["trait_pvalue"][:2], [3 / 5, 1 / 5])
    assert np.isnan(s["trait_pvalue"][2]) and np.isnan(s["trait_pvalue_beta"][2]) and np.isnan(s["trait_qvalue"][2])
    s1, s2, pb = CIS.beta_approximation(max_r2, df, best_p)
    np.testing.assert_array_equal(s["trait_pvalue_beta"][:2], pb[:2])
    # Benjamini-Hochberg over the two traits with a defined pair
    lo, hi = sorted(pb[:2])
    want = {lo: min(2 * lo, hi, 1.0), hi: min(hi, 1.0)}
    np.testing.assert_allclose(s["trait_qvalue"][:2], [want[pb[0]], want[pb[1]]], rtol=1e-15)
