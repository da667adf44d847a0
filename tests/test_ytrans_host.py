"""transform_y without a GPU: the host build of Phi^-1 (aq_special_eval(26, u)) against 40-digit mpmath, the launch planner of
the transform through aq_ytrans_plan_query, the parsing of the option and every argument error of the C ABI that is raised
before a device call."""
import ctypes as C

import numpy as np
import pytest

from atlasqtl_amd import _lib
from atlasqtl_amd import prepare as P
from tests import yt_util as YU

AQ_ERR_ARG, AQ_ERR_UNSUPPORTED = 1, 3


def ndtri_host(u):
    L = _lib.lib()
    u = np.ascontiguousarray(u, dtype=np.float64)
    out = np.empty_like(u)
    assert L.aq_special_eval(26, _lib.as_dp(u), None, _lib.as_dp(out), u.size) == 0, L.aq_last_error()
    return out


def ndtri_bar():
    """(bar, scipy's error, the reference): 4 x the error of scipy.special.ndtri against mpmath, max |err| / max(|ref|, 1) on
    the grid -- room for a different rounding of the last bit, nothing more.  It comes from the restatement's own error, never
    from the library."""
    from scipy.special import ndtri
    u = YU.ndtri_grid()
    ref = YU.ndtri_mp(u)
    e_scipy = YU.err_metric(ndtri(u), ref)
    return 4.0 * e_scipy, e_scipy, ref


def test_ndtri_host_build_against_mpmath():
    """Measured on the grid (2001 points in [1e-6, 0.5], the five smallest Blom arguments, 0.5), max |err| / max(|ref|, 1)
    against sqrt(2) erfinv(2 u - 1) with 40 digits: aq_ndtri 3.0e-16, scipy.special.ndtri 6.2e-16; the bar is 4 x scipy's,
    2.5e-15.  (On a wider grid that reaches u = 1e-319 and 0.5 - 1e-16, relative to |ref| alone: 3.7e-16 and 6.2e-16.)
    u = 0.5 gives exactly 0."""
    bar, e_scipy, ref = ndtri_bar()
    u = YU.ndtri_grid()
    got = ndtri_host(u)
    e = YU.err_metric(got, ref)
    print(f"aq_ndtri {e:.3e}  scipy.special.ndtri {e_scipy:.3e}  bar {bar:.3e}")
    assert 1e-16 < e_scipy < 2e-15                            # the yardstick itself is where it was measured
    assert e <= bar, (e, bar)
    assert u[-1] == 0.5 and got[-1] == 0.0 and not np.signbit(got[-1])
    assert got[2000] == 0.0 and np.all(got[:2000] < 0.0) and np.all(got[2001:-1] < 0.0) and np.all(np.diff(got[:2001]) > 0.0)


def test_ndtri_outside_its_range():
    got = ndtri_host([0.0, 0.75, -0.1, np.nan, 1e-300, 5e-324])
    assert got[0] == -np.inf and np.all(np.isnan(got[1:4]))
    ref = YU.ndtri_mp([1e-300])                               # beyond erfc's normal range the steps run on log Phi
    assert abs(got[4] - ref[0]) <= 4e-15 * abs(ref[0]) and -39.0 < got[5] < -38.0


def plan(n, q, free, expect=0):
    pl = _lib.AqYtransPlan()
    rc = _lib.lib().aq_ytrans_plan_query(n, q, free, C.byref(pl))
    assert rc == expect, (n, q, free, rc, _lib.lib().aq_last_error())
    return pl


def test_planner_paths_and_limits(monkeypatch):
    monkeypatch.delenv("AQ_YT_PATH", raising=False)
    GiB = 1 << 30
    pl = plan(16384, 10, GiB)
    assert (pl.path, pl.n_pad, pl.lds_bytes, pl.traits_per_batch, pl.scratch_bytes) == (0, 16384, 131072, 10, 0)
    pl = plan(16385, 10, GiB)
    assert (pl.path, pl.n_pad, pl.lds_bytes, pl.traits_per_batch, pl.scratch_bytes) == (1, 32768, 131072, 10, 10 * 32768 * 8)
    pl = plan(YU.N_MAX, 64, GiB)
    assert (pl.path, pl.n_pad, pl.traits_per_batch) == (1, 131072, 64)
    assert plan(2, 1, 0).n_pad == 2 and plan(1000, 3, 0).n_pad == 1024 and plan(1000, 3, 0).lds_bytes == 8192
    for n in (2, 63, 1000, 16384, 16385, 20000, 40000, 65536, 65537, YU.N_MAX):
        for q in (1, 7, 1000, 20000):
            for free in (0, 1 << 20, 3 << 20, GiB, 64 * GiB):
                pl = _lib.AqYtransPlan()
                rc = _lib.lib().aq_ytrans_plan_query(n, q, free, C.byref(pl))
                n_pad = 1 << max(1, int(np.ceil(np.log2(n))))
                if n_pad > 16384 and free < 8 * n_pad:         # not one column fits
                    assert rc == AQ_ERR_UNSUPPORTED and b"one column" in _lib.lib().aq_last_error(), (n, q, free)
                    continue
                assert rc == 0, (n, q, free)
                assert pl.n_pad == n_pad and pl.path == int(n_pad > 16384)
                assert pl.lds_bytes == 8 * min(n_pad, 16384) <= 160 * 1024
                assert 1 <= pl.traits_per_batch <= q
                assert pl.scratch_bytes == (8 * n_pad * pl.traits_per_batch if pl.path else 0) <= free
    # n beyond the samples a fit takes: AQ_ERR_UNSUPPORTED, as aq_plan_query treats AQ_N_MAX
    plan(YU.N_MAX + 1, 1, GiB, expect=AQ_ERR_UNSUPPORTED)
    assert b"82944" in _lib.lib().aq_last_error()
    st = _lib.AqVbStatus()
    assert _lib.lib().aq_plan_query(YU.N_MAX + 1, 100, 10, 0, 0, 256, 288 * GiB, None, C.byref(st)) == AQ_ERR_UNSUPPORTED
    for bad in ((1, 1, GiB), (10, 0, GiB), (10, 1, -1)):
        plan(*bad, expect=AQ_ERR_ARG)
    assert _lib.lib().aq_ytrans_plan_query(10, 1, GiB, None) == AQ_ERR_ARG


def test_planner_path_override(monkeypatch):
    monkeypatch.setenv("AQ_YT_PATH", "global")
    pl = plan(1000, 17, 1 << 30)
    assert (pl.path, pl.n_pad, pl.lds_bytes, pl.traits_per_batch, pl.scratch_bytes) == (1, 1024, 8192, 17, 17 * 8192)
    assert plan(16384, 2, 1 << 30).path == 1
    monkeypatch.setenv("AQ_YT_PATH", "lds")
    assert plan(16384, 2, 1 << 30).path == 0
    assert plan(16385, 2, 1 << 30).path == 1                  # a column that LDS does not hold is not forced into it
    monkeypatch.setenv("AQ_YT_PATH", "fast")
    plan(1000, 17, 1 << 30, expect=AQ_ERR_ARG)
    assert b"AQ_YT_PATH must be lds or global" in _lib.lib().aq_last_error()


def test_option_parsing():
    assert P.transform_y_options(None) is None
    assert P.transform_y_options("int") == {"method": "int", "offset": 0.375}
    assert P.transform_y_options({"method": "int"}) == {"method": "int", "offset": 0.375}
    assert P.transform_y_options({"method": "int", "offset": 0}) == {"method": "int", "offset": 0.0}
    assert P.transform_y_options({"method": "int", "offset": 0.5})["offset"] == 0.5
    form = "transform_y must be None, 'int' or a dict"
    for bad in (1, True, ["int"], {}, {"offset": 0.375}, {"method": "int", "c": 0.375}):
        with pytest.raises(P.AtlasqtlError, match=form):
            P.transform_y_options(bad)
    for bad in ("log", "INT", {"method": "rankit"}, {"method": 1}):
        with pytest.raises(P.AtlasqtlError, match="transform_y: method must be 'int'"):
            P.transform_y_options(bad)
    for bad in (-0.1, 0.51, float("nan"), float("inf"), "0.375", None, True):
        with pytest.raises(P.AtlasqtlError, match=r"transform_y: offset must be a number in \[0, 1/2\]"):
            P.transform_y_options({"method": "int", "offset": bad})


def test_python_entries_refuse_before_any_device_call():
    """These raise on a machine without a GPU as well: the checks come first."""
    import atlasqtl_amd as A
    Y = np.random.default_rng(0).standard_normal((30, 3))
    X = np.random.default_rng(1).standard_normal((30, 8))
    with pytest.raises(P.AtlasqtlError, match="transform_y: method must be 'int'"):
        A.atlasqtl(Y, X, p0=(2, 4), transform_y="rank", verbose=0)
    with pytest.raises(P.AtlasqtlError, match="transform_y: method must be 'int'"):
        P.prepare_on_device(Y, X, transform_y="rank")
    with pytest.raises(P.AtlasqtlError, match=r"rank_normalize: offset must be a number in \[0, 1/2\]"):
        A.rank_normalize(Y, offset=0.6)
    with pytest.raises(P.AtlasqtlError, match="rank_normalize: Y must be a numeric matrix"):
        A.rank_normalize(Y[:, 0])
    with pytest.raises(P.AtlasqtlError, match="at most 82944"):
        A.rank_normalize(np.zeros((YU.N_MAX + 1, 1)))


def test_abi_argument_errors_need_no_gpu():
    L = _lib.lib()
    n, p, q = 12, 4, 2
    Y = np.asfortranarray(np.random.default_rng(0).standard_normal((n, q)))
    X = np.asfortranarray(np.random.default_rng(1).standard_normal((n, p)))
    out = np.empty_like(Y)
    err = lambda: L.aq_last_error().decode()
    # aq_rank_int
    assert L.aq_rank_int(None, n, q, 0.375, _lib.as_dp(out), None, None, 0) == AQ_ERR_ARG and "aq_rank_int: NULL" in err()
    assert L.aq_rank_int(_lib.as_dp(Y), n, q, 0.375, None, None, None, 0) == AQ_ERR_ARG and "aq_rank_int: NULL" in err()
    assert L.aq_rank_int(_lib.as_dp(Y), 1, q, 0.375, _lib.as_dp(out), None, None, 0) == AQ_ERR_ARG and "n >= 2" in err()
    assert L.aq_rank_int(_lib.as_dp(Y), n, 0, 0.375, _lib.as_dp(out), None, None, 0) == AQ_ERR_ARG and "q >= 1" in err()
    for c in (-1e-9, 0.5000001, float("nan"), float("inf")):
        assert L.aq_rank_int(_lib.as_dp(Y), n, q, c, _lib.as_dp(out), None, None, 0) == AQ_ERR_ARG
        assert "aq_rank_int: the offset c must lie in [0, 1/2]" in err()
    assert L.aq_rank_int(_lib.as_dp(Y), YU.N_MAX + 1, 1, 0.375, _lib.as_dp(out), None, None, 0) == AQ_ERR_ARG
    assert "aq_rank_int: n = 82945 exceeds" in err()
    # aq_prepare_data_opt
    pin = _lib.AqPrepInput()
    pin.n, pin.p, pin.q, pin.X, pin.X_i8, pin.Y, pin.device = n, p, q, _lib.as_dp(X), None, _lib.as_dp(Y), 0
    bed = _lib.AqPrepBedInput()
    yt = _lib.AqPrepYtrans()
    h = C.c_void_p()
    yt.method, yt.offset = 1, 0.375
    assert L.aq_prepare_data_opt(C.byref(pin), None, None, C.byref(yt), None) == AQ_ERR_ARG and "aq_prepare_data_opt: NULL" in err()
    assert L.aq_prepare_data_opt(None, None, None, C.byref(yt), C.byref(h)) == AQ_ERR_ARG and "exactly one of in and bed" in err()
    assert L.aq_prepare_data_opt(C.byref(pin), C.byref(bed), None, C.byref(yt), C.byref(h)) == AQ_ERR_ARG and "exactly one of" in err()
    yt.method = 2
    assert L.aq_prepare_data_opt(C.byref(pin), None, None, C.byref(yt), C.byref(h)) == AQ_ERR_ARG
    assert "aq_prepare_data_opt: unknown transform of Y, method = 2" in err()
    yt.method = 1
    for c in (-0.25, 0.75, float("nan")):
        yt.offset = c
        assert L.aq_prepare_data_opt(C.byref(pin), None, None, C.byref(yt), C.byref(h)) == AQ_ERR_ARG
        assert "aq_prepare_data_opt: the offset c must lie in [0, 1/2]" in err()
    yt.offset = 0.375
    pin.n = YU.N_MAX + 1
    assert L.aq_prepare_data_opt(C.byref(pin), None, None, C.byref(yt), C.byref(h)) == AQ_ERR_ARG and "n = 82945 exceeds" in err()
    pin.n, pin.Y = n, None
    assert L.aq_prepare_data_opt(C.byref(pin), None, None, C.byref(yt), C.byref(h)) == AQ_ERR_ARG and "NULL data pointer" in err()
    assert h.value is None
    # aq_prep_ytrans_info
    assert L.aq_prep_ytrans_info(None, None, None, None, None) == AQ_ERR_ARG and "aq_prep_ytrans_info: NULL handle" in err()
    # Phi^-1 is function 26 of the test hook on both builds; 27 is unknown
    x = np.array([0.25])
    assert L.aq_special_eval(27, _lib.as_dp(x), None, _lib.as_dp(np.empty(1)), 1) == AQ_ERR_ARG
    assert L.aq_special_eval_device(27, _lib.as_dp(x), None, _lib.as_dp(np.empty(1)), 1, 0) == AQ_ERR_ARG
    assert "unknown function id" in err()
