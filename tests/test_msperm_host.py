"""The host side of the permutation nulls of the marginal screen, without a GPU: the launch planner through
aq_msperm_plan_query, the argument errors of aq_prep_marginal_perm that come before any device call, and the pure helpers of
atlasqtl_amd/marginal.py -- the parsing of `permutations` and the summary of the null statistics.  The checks of
aq_prep_marginal_perm that need a handle's n and q (a NaN cutoff, a row of perm that is no permutation) cannot be reached
through the C ABI without a device, since a handle cannot be made without one: the check of the rows is a pure host function
of aq_msperm_plan.h and runs here through the stand-alone tests/tools/msperm_probe.cpp, as do the planner's forced fields;
tests/test_gpu_msperm.py repeats both and adds the NaN cutoff on a real handle."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from atlasqtl_amd import _lib
from atlasqtl_amd import marginal as M
from atlasqtl_amd.prepare import AtlasqtlError, PreparedData

GIB = 1 << 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "atlasqtl_amd", "csrc")


def _plan(hiplib, n, p1, q, masked, ncu, n_perm):
    pl = _lib.AqMspermPlan()
    rc = hiplib.aq_msperm_plan_query(n, p1, q, masked, ncu, n_perm, C.byref(pl))
    return rc, pl


@pytest.mark.parametrize("n,p1,q,n_perm", [
    (1000, 50000, 10000, 1000),            # the benchmark shape: a panel is 80 MB, 13 of them fit
    (1000, 50000, 10000, 5),               # fewer permutations than a launch could hold
    (1000, 300, 70, 100),
    (37, 70, 5, 5), (50, 130, 67, 5), (96, 200, 150, 5),
    (82944, 1000, 1000, 7),                # one panel is 0.62 GiB: two exceed 1 GiB, so PB = 1 and one permutation per launch
    (20, 3, 1, 1),
])
@pytest.mark.parametrize("masked", [0, 1])
def test_plan_invariants(hiplib, n, p1, q, n_perm, masked):
    rc, pl = _plan(hiplib, n, p1, q, masked, 256, n_perm)
    assert rc == 0, hiplib.aq_last_error()
    ms = _lib.AqMscreenPlan()
    assert hiplib.aq_mscreen_plan_query(n, p1, q, masked, 256, C.byref(ms)) == 0
    assert (pl.tile, pl.tiles_p, pl.tiles_q, pl.masked) == (ms.tile, ms.tiles_p, ms.tiles_q, masked)
    if masked:
        assert pl.tile == 64
    assert pl.pb in (1, 2, 4) and pl.batch >= pl.pb and pl.batch % pl.pb == 0
    assert pl.batch * q * n * 8 == pl.yp_bytes <= GIB
    assert pl.launches * pl.batch >= n_perm > (pl.launches - 1) * pl.batch
    assert 0 < pl.lds_bytes <= 65536
    streams = 2 if masked else 1
    assert pl.lds_bytes == (1 + streams * pl.pb) * pl.tile * 18 * 8 + pl.tile * 20 + 2 * pl.pb * pl.tile * 8
    assert pl.scratch_bytes == pl.batch * (4 * p1 + 16 * q + 4 * n + 24) <= GIB
    assert pl.tiles_p * pl.tiles_q * (pl.batch // pl.pb) < 2 ** 31
    # the batch is the largest the rules allow: one more group of PB breaks one of them
    more = pl.batch + pl.pb
    assert more * q * n * 8 > GIB or more * (4 * p1 + 16 * q + 4 * n + 24) > GIB or more - pl.pb >= n_perm \
        or pl.tiles_p * pl.tiles_q * (more // pl.pb) >= 2 ** 31
    if 2 * q * n * 8 > GIB:
        assert pl.pb == 1 and pl.batch == 1 and pl.launches == n_perm


def test_plan_at_the_bench_shape(hiplib):
    rc, pl = _plan(hiplib, 1000, 50000, 10000, 0, 256, 1000)
    assert rc == 0 and pl.tile == 128 and pl.pb == 1 and pl.batch == 13 and pl.launches == 77
    rc, pl = _plan(hiplib, 1000, 50000, 10000, 1, 256, 1000)
    assert rc == 0 and pl.tile == 64 and pl.pb == 1 and pl.batch == 13 and pl.launches == 77
    rc, pl = _plan(hiplib, 1000, 2000, 1900, 0, 256, 1000)                 # tile 64 for complete Y: PB = 2
    assert rc == 0 and pl.tile == 64 and pl.pb == 2 and pl.batch == 70 and pl.launches == 15


def test_plan_refuses_a_panel_above_one_gib(hiplib):
    for masked in (0, 1):
        rc, _ = _plan(hiplib, 82944, 1000, 2000, masked, 256, 10)        # 1.33e9 bytes
        assert rc == 3
        msg = hiplib.aq_last_error()
        assert b"aq_msperm_plan_query" in msg and b"1 GiB" in msg


def test_plan_query_refuses_bad_arguments(hiplib):
    pl = _lib.AqMspermPlan()
    assert hiplib.aq_msperm_plan_query(100, 10, 5, 0, 256, 10, None) == 1
    assert b"aq_msperm_plan_query" in hiplib.aq_last_error()
    for bad in [(0, 10, 5, 0, 256, 10), (100, 0, 5, 0, 256, 10), (100, 10, 0, 0, 256, 10), (100, 10, 5, 2, 256, 10),
                (100, 10, 5, -1, 256, 10), (100, 10, 5, 0, 0, 10), (100, 10, 5, 0, 256, 0), (100, 10, 5, 0, 256, -3)]:
        assert hiplib.aq_msperm_plan_query(*bad, C.byref(pl)) == 1, bad
        assert b"aq_msperm_plan_query" in hiplib.aq_last_error()


def test_argument_errors_need_no_gpu(hiplib):
    cut = np.zeros(3)
    perm = np.arange(4, dtype=np.int32)[None, :]
    i64 = C.POINTER(C.c_int64)
    none = (None, C.cast(None, i64), C.cast(None, i64), C.cast(None, i64))
    assert hiplib.aq_prep_marginal_perm(None, _lib.as_dp(cut), 0, _lib.as_ip(perm), *none) == 1
    assert b"aq_prep_marginal_perm" in hiplib.aq_last_error() and b"n_perm" in hiplib.aq_last_error()
    assert hiplib.aq_prep_marginal_perm(None, None, 1, _lib.as_ip(perm), *none) == 1
    assert b"aq_prep_marginal_perm: NULL r2_cut or perm" in hiplib.aq_last_error()
    assert hiplib.aq_prep_marginal_perm(None, _lib.as_dp(cut), 1, None, *none) == 1
    assert b"aq_prep_marginal_perm: NULL r2_cut or perm" in hiplib.aq_last_error()
    assert hiplib.aq_prep_marginal_perm(None, _lib.as_dp(cut), 1, _lib.as_ip(perm), *none) == 1
    assert b"aq_prep_marginal_perm: NULL handle" in hiplib.aq_last_error()
    ms = C.c_double(0.0)
    assert hiplib.aq_prep_marginal_perm_time(None, 1, 1, C.byref(ms), None) == 1
    assert b"aq_prep_marginal_perm_time" in hiplib.aq_last_error()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/tools/msperm_probe.cpp, built with the host compiler: requests in, one answer line each."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    exe = tmp_path_factory.mktemp("msperm") / "msperm_probe"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "tools", "msperm_probe.cpp"), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def ask(lines):
        r = subprocess.run([str(exe)], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout.splitlines()
    return ask


def test_rows_of_perm_are_checked_on_the_host(probe):
    """aq_msperm_check_rows, which aq_prep_marginal_perm runs on every row before its first device call: a repeated index and
    an index outside 0 ... n - 1 are AQ_ERR_ARG, and the message names the row.  (On a real handle: tests/test_gpu_msperm.py.)"""
    got = probe(["rows 4 0,1,2,3", "rows 4 3,1,0,2 0,1,2,3 2,3,1,0", "rows 1 0",
                 "rows 4 0,1,2,3 0,2,2,3", "rows 4 0,1,2,4", "rows 4 0,1,2,3 3,2,1,0 -1,0,1,2", "rows 4 0,1,2,2147483647",
                 "rows 4 0,0,0,0"])
    assert got[:3] == ["0 -"] * 3
    assert got[3].startswith("1 probe: row 1 of perm is not a permutation of 0 ... 3") and got[3].endswith("index 2 at position 2 is repeated")
    assert got[4].startswith("1 probe: row 0 of perm") and got[4].endswith("index 4 at position 3 is out of range")
    assert got[5].startswith("1 probe: row 2 of perm") and got[5].endswith("index -1 at position 0 is out of range")
    assert got[6].startswith("1 probe: row 0 of perm") and got[6].endswith("index 2147483647 at position 3 is out of range")
    assert got[7].startswith("1 probe: row 0 of perm") and got[7].endswith("index 0 at position 1 is repeated")


def test_forced_plan_fields(probe):
    """The planner with AQ_MSCREEN_TILE, AQ_MSPERM_PB and AQ_MSPERM_BATCH as aq_prep_marginal_perm hands them over (-1: set,
    but no number >= 1): every instance of the tile kernel is reachable, and nothing else is."""
    shape = "50 130 67"
    ok = {(0, 64, 1): 20736, (0, 64, 2): 30976, (0, 64, 4): 51456, (0, 128, 1): 41472, (1, 64, 1): 29952, (1, 64, 2): 49408}
    req = [f"plan {shape} {m} 256 5 {0 if m else t} {pb} 0" for (m, t, pb) in ok]
    for line, ((m, t, pb), lds) in zip(probe(req), ok.items()):
        assert line.split() == ["0", str(t), str(pb), str(-(-5 // pb) * pb), "1", str(lds)], (m, t, pb, line)
    # forced batches: several launches, the last one ragged
    got = probe([f"plan {shape} 0 256 5 64 2 2", f"plan {shape} 0 256 5 64 4 4", f"plan {shape} 1 256 5 0 1 2", f"plan {shape} 0 256 5 128 1 2"])
    assert [g.split()[1:5] for g in got] == [["64", "2", "2", "3"], ["64", "4", "4", "2"], ["64", "1", "2", "3"], ["128", "1", "2", "3"]]
    bad = probe([f"plan {shape} 0 256 5 128 2 0", f"plan {shape} 0 256 5 64 3 0", f"plan {shape} 1 256 5 0 4 0", f"plan {shape} 0 256 5 64 -1 0",
                 f"plan {shape} 0 256 5 64 2 3", f"plan {shape} 0 256 5 64 2 -1", f"plan {shape} 0 256 5 64 2 8", f"plan {shape} 0 256 5 32 0 0",
                 f"plan {shape} 0 256 5 -1 0 0", "plan 82944 1000 1000 0 256 5 0 2 0"])
    for line in bad[:4]:
        assert line.startswith("1 | probe: AQ_MSPERM_PB"), line
    for line in bad[4:7]:                                            # no multiple of PB; no number; beyond the permutations asked for
        assert line.startswith("1 | probe: AQ_MSPERM_BATCH"), line
    for line in bad[7:9]:
        assert line.startswith("1 | probe: AQ_MSCREEN_TILE"), line
    assert bad[9].startswith("1 | probe: AQ_MSPERM_PB = 2 panels of Y exceed 1 GiB")


def test_wrapper_refuses_rows_before_the_library():
    """PreparedData.marginal_permute checks shapes and the range of the indices before the cast to int32 (the library
    checks every row again, and names it)."""
    prep = PreparedData(None, 4, 3, 2, np.zeros((4, 2)), 0)
    with pytest.raises(AtlasqtlError, match="one cutoff per trait"):
        prep.marginal_permute(np.zeros(3), np.arange(4)[None, :])
    for bad in (np.arange(4), np.arange(5)[None, :], np.zeros((0, 4), dtype=np.int64), np.arange(4.0)[None, :]):
        with pytest.raises(AtlasqtlError, match="B x n integer array"):
            prep.marginal_permute(np.zeros(2), bad)
    for bad in (np.array([[0, 1, 2, 4]]), np.array([[0, 1, 2, -1]]), np.array([[0, 1, 2, 2 ** 32 + 3]])):
        with pytest.raises(AtlasqtlError, match="permutation of 0 ... 3"):
            prep.marginal_permute(np.zeros(2), bad)


def test_permutation_options():
    assert M.permutation_options(None) is None and M.permutation_options(None, 10) is None
    n = 11
    for arg, B, seed in ((4, 4, 0), (np.int64(3), 3, 0), ({"n": 5}, 5, 0), ({"n": 2, "seed": 9}, 2, 9)):
        o = M.permutation_options(arg, n)
        rng = np.random.default_rng(seed)
        want = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int32)
        assert (o["n"], o["seed"]) == (B, seed)
        assert o["perms"].dtype == np.int32 and o["perms"].flags.c_contiguous
        np.testing.assert_array_equal(o["perms"], want)
        assert M.permutation_options(arg) == dict(n=B, seed=seed, perms=None)          # before n is known
    rows = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 3, 2]], dtype=np.int64)      # the identity, and within {0, 1} and {2, 3}
    o = M.permutation_options(rows, 4)
    assert (o["n"], o["seed"]) == (3, None) and o["perms"].dtype == np.int32
    np.testing.assert_array_equal(o["perms"], rows)
    np.testing.assert_array_equal(M.permutation_options(rows.tolist())["perms"], rows)
    for bad in (0, -2, 2.0, np.float64(3), True, "5", {"n": 0}, {"n": 2.5}, {"seed": 1}, {"n": 3, "seeds": 1}, {"n": 3, "seed": -1},
                {"n": 3, "seed": 0.5}):
        with pytest.raises(AtlasqtlError, match="permutations"):
            M.permutation_options(bad, 4)
    with pytest.raises(AtlasqtlError, match="one entry per sample"):
        M.permutation_options(rows, 5)                                               # a wrong width
    for bad in ([[0, 1, 1, 3]], [[0, 1, 2, 4]], [[-1, 0, 1, 2]], [[0, 1, 2, 3], [0, 0, 0, 0]]):
        with pytest.raises(AtlasqtlError, match="is not a permutation"):
            M.permutation_options(np.array(bad), 4)
    with pytest.raises(AtlasqtlError, match="row 1 "):
        M.permutation_options(np.array([[0, 1, 2, 3], [0, 0, 0, 0]]))
    for bad in (np.arange(4), np.arange(4.0)[None, :], np.zeros((0, 4), dtype=int)):
        with pytest.raises(AtlasqtlError, match="B x n integers"):
            M.permutation_options(bad, 4)


def test_permutation_summary_by_hand():
    # B = 4 permutations, q = 3 traits (the last without a defined pair), p = 5 predictors
    max_r2 = np.array([[0.25, 0.10, -1.0],
                       [0.09, 0.30, -1.0],
                       [0.04, 0.05, -1.0],
                       [0.25, 0.01, -1.0]])
    best_r = np.array([-0.5, 0.6, np.nan])             # r^2 = 0.25 (tied with two permutations: >= counts them), 0.36 (none)
    best_snp = np.array([2, 0, -1])
    hs_max = np.array([3, 0, 1, 3])
    n_sel = np.array([6, 0, 1, 5])
    rs = np.array([0, 1, 3, 4, 2])
    s = M.permutation_summary(max_r2, hs_max, n_sel, best_snp, best_r, rs, 10)
    np.testing.assert_array_equal(s["trait_pvalue"][:2], [3 / 5, 1 / 5])
    assert np.isnan(s["trait_pvalue"][2])
    # rs = 0: every permutation reaches it, p = 1; 1: three of four; 3: a tie with two; 4: none; 2: two
    np.testing.assert_array_equal(s["hotspot_pvalue"], [1.0, 4 / 5, 3 / 5, 1 / 5, 3 / 5])
    assert s["expected_null_pairs"] == 3.0 and s["empirical_fdr"] == 0.3
    assert set(s) == {"trait_pvalue", "hotspot_pvalue", "expected_null_pairs", "empirical_fdr"}
    # the clamp, and a screen that selected nothing
    assert M.permutation_summary(max_r2, hs_max, n_sel, best_snp, best_r, rs, 2)["empirical_fdr"] == 1.0
    assert M.permutation_summary(max_r2, hs_max, n_sel, best_snp, best_r, rs, 0)["empirical_fdr"] == 1.0
    assert M.permutation_summary(max_r2, hs_max, 0 * n_sel, best_snp, best_r, rs, 0)["empirical_fdr"] == 0.0
    # a trait's own r^2 recomputed as best_r * best_r: the identity permutation's max_r2 counts (bit-equal by construction)
    r = np.array([0.1 + 0.2])
    one = M.permutation_summary(np.array([[r[0] * r[0]]]), [0], [0], [0], r, [0], 0)
    assert one["trait_pvalue"][0] == 1.0


def test_no_new_key_unless_asked():
    """permutations is off by default in marginal_screen() and screen_handle(); atlasqtl(marginal_screen=...) and its option
    parser are as they were (tests/test_gpu_msperm.py checks the keys of the results)."""
    import atlasqtl_amd as A
    assert "marginal_screen" in A.__all__ and A.marginal_screen is M.marginal_screen
    assert inspect.signature(M.marginal_screen).parameters["permutations"].default is None
    assert inspect.signature(M.screen_handle).parameters["permutations"].default is None
    assert "permutations" not in inspect.signature(M.screen_options).parameters
    assert M.SCREEN_KEYS == ("p_value", "fdr", "max_pairs")
    with pytest.raises(AtlasqtlError, match="marginal_screen must be None, True or a dict"):
        M.screen_arg({"permutations": 10})


def test_marginal_screen_refuses_bad_permutations_before_the_device():
    X, Y = np.zeros((6, 3)), np.zeros((6, 2))
    for bad in (0, 1.5, np.array([[0, 1, 1, 2, 3, 4]])):
        with pytest.raises(AtlasqtlError, match="permutation"):
            M.marginal_screen(Y, X, permutations=bad)
