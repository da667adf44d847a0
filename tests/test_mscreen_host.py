"""The host side of the marginal screen, without a GPU: the launch planner through aq_mscreen_plan_query, the argument errors
of aq_prep_marginal that come before any device call, and the pure helpers of atlasqtl_amd/marginal.py -- option parsing, the
conversion of a p-value threshold into a cutoff on r^2, Benjamini-Hochberg from a complete table, the order of the table."""
import ctypes as C

import numpy as np
import pytest

from atlasqtl_amd import _lib
from atlasqtl_amd import marginal as M
from atlasqtl_amd.prepare import AtlasqtlError


def _plan(hiplib, n, p1, q, masked, ncu):
    pl = _lib.AqMscreenPlan()
    rc = hiplib.aq_mscreen_plan_query(n, p1, q, masked, ncu, C.byref(pl))
    return rc, pl


@pytest.mark.parametrize("n,p1,q,ncu,tile", [
    (1000, 50000, 10000, 256, 128),        # the benchmark shape: 391 x 79 tiles of 128 fill 256 CUs many times over
    (1000, 2048, 2048, 256, 128),          # 16 x 16 = 256 tiles of 128: exactly one per CU
    (1000, 2048, 2047, 257, 64),           # one CU more than tiles of 128: the smaller tile
    (1000, 2048, 1920, 256, 64),           # 16 x 15 = 240 < 256
    (1000, 300, 70, 256, 64),
    (1000, 300, 70, 4, 64),                # 3 x 1 tiles of 128 do not fill 4 CUs ...
    (1000, 300, 70, 3, 128),               # ... but they fill 3
    (20, 3, 1, 1, 128),
])
def test_tile_choice_against_cu_count(hiplib, n, p1, q, ncu, tile):
    rc, pl = _plan(hiplib, n, p1, q, 0, ncu)
    assert rc == 0
    assert pl.tile == tile and pl.masked == 0 and pl.sample_chunk == 16
    assert pl.tiles_p == -(-p1 // tile) and pl.tiles_q == -(-q // tile) and pl.n_tiles == pl.tiles_p * pl.tiles_q
    assert pl.scratch_bytes == 12 * pl.tiles_p * q
    assert pl.lds_bytes == 2 * tile * 18 * 8 + 2 * tile * 12 + tile * 20 <= 65536


@pytest.mark.parametrize("n,p1,q,ncu", [(1000, 50000, 10000, 256), (333, 257, 33, 256), (20, 3, 1, 1)])
def test_masked_plan_has_one_tile_size(hiplib, n, p1, q, ncu):
    rc, pl = _plan(hiplib, n, p1, q, 1, ncu)
    assert rc == 0
    assert pl.tile == 64 and pl.masked == 1
    assert pl.tiles_p == -(-p1 // 64) and pl.tiles_q == -(-q // 64) and pl.n_tiles == pl.tiles_p * pl.tiles_q
    assert pl.scratch_bytes == 12 * pl.tiles_p * q
    assert pl.lds_bytes == 3 * 64 * 18 * 8 + 2 * 64 * 12 + 64 * 20 <= 65536
    complete = _plan(hiplib, n, p1, q, 0, ncu)[1]
    assert pl.lds_bytes > _plan(hiplib, n, p1, q, 0, 10 ** 6)[1].lds_bytes      # against the complete instance at the same tile
    assert complete.n_tiles <= pl.n_tiles


def test_plan_query_refuses_bad_arguments(hiplib):
    pl = _lib.AqMscreenPlan()
    assert hiplib.aq_mscreen_plan_query(100, 10, 5, 0, 256, None) == 1
    assert b"aq_mscreen_plan_query" in hiplib.aq_last_error()
    for bad in [(0, 10, 5, 0, 256), (100, 0, 5, 0, 256), (100, 10, 0, 0, 256), (100, 10, 5, 2, 256), (100, 10, 5, -1, 256),
                (100, 10, 5, 0, 0)]:
        assert hiplib.aq_mscreen_plan_query(*bad, C.byref(pl)) == 1, bad
        assert b"aq_mscreen_plan_query" in hiplib.aq_last_error()


def test_marginal_argument_errors_need_no_gpu(hiplib):
    cut = np.zeros(3)
    assert hiplib.aq_prep_marginal(None, None, 0, None, None, None, None, None, None, None, None, None) == 1
    assert b"NULL r2_cut" in hiplib.aq_last_error()
    assert hiplib.aq_prep_marginal(None, _lib.as_dp(cut), -1, None, None, None, None, None, None, None, None, None) == 1
    assert b"cap" in hiplib.aq_last_error()
    assert hiplib.aq_prep_marginal(None, _lib.as_dp(cut), 0, None, None, None, None, None, None, None, None, None) == 1
    assert b"NULL handle" in hiplib.aq_last_error()
    ms = C.c_double(0.0)
    assert hiplib.aq_prep_marginal_time(None, 1, C.byref(ms), None) == 1
    assert b"aq_prep_marginal_time" in hiplib.aq_last_error()


def test_marginal_screen_is_exported():
    import atlasqtl_amd as A
    assert "marginal_screen" in A.__all__ and A.marginal_screen is M.marginal_screen


def test_option_parsing():
    assert M.screen_options() == dict(mode="bonferroni", level=None, max_pairs=None, dense=False)
    assert M.screen_options(p=50, q=20)["level"] == 0.05 / 1000
    assert M.screen_options(p_value=1e-6, max_pairs=10) == dict(mode="p_value", level=1e-6, max_pairs=10, dense=False)
    assert M.screen_options(fdr=0.05, p=5, q=4) == dict(mode="fdr", level=0.05, max_pairs=None, dense=False)
    assert M.screen_options(p_value=1)["level"] == 1.0
    with pytest.raises(AtlasqtlError, match="at most one of p_value and fdr"):
        M.screen_options(p_value=0.01, fdr=0.05)
    for bad in (0, -0.1, 1.5, float("nan"), "0.05", True):
        with pytest.raises(AtlasqtlError, match="p_value must be a number in"):
            M.screen_options(p_value=bad)
        with pytest.raises(AtlasqtlError, match="fdr must be a number in"):
            M.screen_options(fdr=bad)
    for bad in (0, -3, 2.5, True, "7"):
        with pytest.raises(AtlasqtlError, match="max_pairs"):
            M.screen_options(max_pairs=bad)
    with pytest.raises(AtlasqtlError, match="dense must be"):
        M.screen_options(dense=1)
    assert M.screen_options(dense=True, p=1 << 14, q=1 << 13)["dense"] is True        # 2^27 entries: the last size taken
    with pytest.raises(AtlasqtlError, match="dense=True would return"):
        M.screen_options(dense=True, p=(1 << 14) + 1, q=1 << 13)
    assert M.screen_options(dense=False, p=1 << 20, q=1 << 20)["dense"] is False


def test_the_argument_of_atlasqtl():
    assert M.screen_arg(None) is None
    assert M.screen_arg(True) == {}
    assert M.screen_arg({"fdr": 0.1, "max_pairs": 3}) == {"fdr": 0.1, "max_pairs": 3}
    for bad in ("yes", 3, {"pvalue": 0.1}, {"p_value": 0.1, "dense": True}):
        with pytest.raises(AtlasqtlError, match="marginal_screen must be None, True or a dict"):
            M.screen_arg(bad)
    with pytest.raises(AtlasqtlError, match="at most one"):
        M.screen_arg({"p_value": 0.1, "fdr": 0.1})


def test_cutoff_conversion_inverts_to_the_p_value():
    from scipy.stats import t as student
    df = np.array([1, 2, 5, 30, 198, 998, 9998])
    for level in (0.5, 0.05, 1e-4, 1e-10, 1e-30):
        cut = M.r2_cutoff(level, df)
        assert ((0 < cut) & (cut <= 1)).all()
        ok = cut < 1 - 1e-6               # closer to 1 the way back through 1 - r^2 loses the digits that the p-value depends on
        assert ok.sum() >= 4
        tc = np.sqrt(cut[ok] * df[ok] / (1 - cut[ok]))
        np.testing.assert_allclose(2 * student.sf(tc, df[ok]), level, rtol=1e-7)
        # a pair exactly at the cutoff has the threshold's p-value through the table's own route
        np.testing.assert_allclose(M.t_and_pvalue(np.sqrt(cut[ok]), df[ok])[1], level, rtol=1e-7)
    levels = np.array([0.5, 0.1, 1e-2, 1e-5, 1e-12])
    cuts = np.array([M.r2_cutoff(lv, df) for lv in levels])
    assert (np.diff(cuts, axis=0) > 0).all()                            # a stricter threshold, a larger cutoff, for every df
    assert (np.diff(M.r2_cutoff(1e-3, df)) < 0).all()                   # more degrees of freedom, a smaller cutoff
    np.testing.assert_array_equal(M.r2_cutoff(0.05, [0, -1, -7]), np.inf)      # an unusable trait selects nothing
    assert M.r2_cutoff(1.0, [10])[0] == 0.0                             # p <= 1 selects every defined pair


def test_t_and_pvalue_at_the_ends():
    t, p = M.t_and_pvalue(np.array([0.0, 1.0, -1.0, 0.5]), 10)
    assert t[0] == 0 and p[0] == 1 and t[1] == np.inf and t[2] == -np.inf and p[1] == 0 and p[2] == 0
    np.testing.assert_allclose(t[3], 0.5 * np.sqrt(10 / 0.75))


def _naive_bh(pv, n_tests):
    k = len(pv)
    return np.array([min(1.0, min(pv[j] * n_tests / (j + 1) for j in range(i, k))) for i in range(k)])


def test_bh_against_a_naive_loop():
    rng = np.random.default_rng(3)
    for k, n_tests in ((1, 1), (7, 7), (40, 40), (40, 1000)):
        pv = np.sort(rng.random(k) ** 3)
        np.testing.assert_allclose(M.bh_qvalues(pv, n_tests), _naive_bh(pv, n_tests), rtol=1e-15)
    pv = np.array([1e-6, 1e-6, 1e-6, 2e-3, 2e-3, 0.04, 0.04, 0.04, 0.9])          # ties share their q-value
    q = M.bh_qvalues(pv, 9)
    np.testing.assert_allclose(q, _naive_bh(pv, 9), rtol=1e-15)
    assert q[0] == q[1] == q[2] and q[3] == q[4] and q[5] == q[6] == q[7] and (np.diff(q) >= 0).all()
    assert M.bh_qvalues(np.array([]), 10).size == 0
    with pytest.raises(ValueError, match="ascending"):
        M.bh_qvalues(np.array([0.2, 0.1]), 2)
    # the head of a longer list: exact wherever q <= the level that every value left out exceeds
    allp = np.sort(rng.random(200) ** 4)
    alpha = 0.05
    head = allp[allp <= alpha]
    q_head, q_all = M.bh_qvalues(head, 200), M.bh_qvalues(allp, 200)[:head.size]
    sel = q_all <= alpha
    np.testing.assert_array_equal(q_head <= alpha, sel)
    np.testing.assert_array_equal(q_head[sel], q_all[sel])
    assert (q_head >= q_all).all()


def test_table_order_and_max_pairs():
    p = 10
    snp = np.array([3, 1, 7, 2, 2, 0])
    trait = np.array([0, 1, 0, 2, 1, 0])
    pv = np.array([0.0, 1e-3, 0.0, 1e-3, 1e-9, 0.0])
    t = np.array([-40.0, 3.0, 50.0, -3.0, 6.0, 40.0])
    order = M.table_order(pv, t, snp, trait, p)
    # p = 0 three times: |t| 50 first, then the two |t| = 40 by position 0 < 3; then 1e-9; then the two 1e-3 by position 11 < 22
    np.testing.assert_array_equal(order, [2, 5, 0, 4, 1, 3])
    np.testing.assert_array_equal(order[:4], M.table_order(pv, t, snp, trait, p)[:4])     # max_pairs cuts this order
