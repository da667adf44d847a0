"""GPU: transform_y, the rank-based inverse normal transform of the traits (aq_rank_int, aq_prepare_data_opt), against its
restatement with scipy (tests/yt_util.py): ranks exact, the two kernels bit-identical, Phi^-1 on the device held to the host
build, and the option through prepare_on_device and atlasqtl()."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests import yt_util as YU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = os.path.join(ROOT, "tests", "golden", "plink_toy")
PATH_CASES = [(1000, 17), (16384, 2)]


def ndtri_device(u):
    from atlasqtl_amd import _lib
    L = _lib.lib()
    u = np.ascontiguousarray(u, dtype=np.float64)
    out = np.empty_like(u)
    assert L.aq_special_eval_device(26, _lib.as_dp(u.reshape(-1)), None, _lib.as_dp(out), u.size, 0) == 0, L.aq_last_error()
    return out


def expected_bits(Y, c):
    """What aq_rank_int must return, bit for bit: the device build of Phi^-1 at the one quotient that scipy's ranks give, with
    the sign of the half the rank lies in, NaN where Y is missing."""
    t2, m = YU.doubled_ranks(Y)
    u, upper = YU.folded_argument(t2, m, c)
    x = ndtri_device(u)
    return np.where(np.isnan(Y), np.nan, np.where(upper, -x, x))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def check_against_restatement(Y, got, c, what):
    """Bits, NaN pattern and counts against the restatement, then the values against scipy.special.ndtri itself.  Measured on an
    MI355X over the eleven shapes: 8.4e-16 at worst with ndtri asked below 1/2 (bar 2.5e-15), 1.5e-13 at worst with it asked as
    the restatement words it (at the top ranks of 82 944 samples, where the allowance is 1.1e-12)."""
    assert np.array_equal(np.isnan(got["Y"]), np.isnan(Y)), what
    assert same_bits(got["Y"], expected_bits(Y, c)), what
    n_obs, n_tied = YU.tied_counts(Y)
    assert np.array_equal(got["n_obs"], n_obs) and np.array_equal(got["n_tied"], n_tied), what
    # scipy's own ndtri, with the bar of the CPU test.  Asked below 1/2 and mirrored it is held to the bar alone; asked at
    # (r - c) / (m + 1 - 2 c) as the restatement words it, its argument next to 1 is itself rounded, which the bar is widened by
    # entry by entry (YU.argument_allowance: the restatement's own error, worked out from the number format)
    obs = ~np.isnan(Y)
    folded, raw = YU.rank_int_folded(Y, c)[obs], YU.rank_int(Y, c)[obs]
    e = YU.err_metric(got["Y"][obs], folded)
    e_raw = np.abs(got["Y"][obs] - raw) / np.maximum(np.abs(raw), 1.0)
    print(f"{what}: against scipy.special.ndtri {e:.3e} (asked below 1/2), {float(np.max(e_raw)):.3e} (as the restatement words it)")
    assert e <= _bar(), (what, e)
    assert np.all(e_raw <= _bar() + YU.argument_allowance(raw)), (what, float(np.max(e_raw)))


_BAR = []


def _bar():
    if not _BAR:
        from tests.test_ytrans_host import ndtri_bar
        _BAR.append(ndtri_bar()[0])
    return _BAR[0]


@pytest.mark.parametrize("n,q", YU.SHAPES)
def test_ranks_are_exact(n, q):
    import atlasqtl_amd as A
    Y = YU.columns(n, q)
    got = A.rank_normalize(Y)
    assert got["Y"].shape == (n, q) and got["n_obs"].shape == (q,) and got["n_tied"].shape == (q,)
    check_against_restatement(Y, got, 0.375, f"n={n} q={q}")


def test_ndtri_device_build_against_host_build():
    """aq_special_eval_device(26, .) against aq_special_eval(26, .) on the grid of the CPU test, relative to the host's value
    with the 5e-15 that tests/test_gpu_special.py allows the other functions of the header (0 against 0 at u = 0.5).
    Measured on an MI355X: 4.0e-16."""
    from tests.test_ytrans_host import ndtri_host
    u = YU.ndtri_grid()
    h, d = ndtri_host(u), ndtri_device(u)
    assert d[-1] == 0.0 and d[2000] == 0.0 and not np.signbit(d[-1])
    nz = h != 0.0
    err = float(np.max(np.abs(h[nz] - d[nz]) / np.abs(h[nz])))
    print(f"device against host build of aq_ndtri: {err:.3e} relative")
    assert err < 5e-15, err


def test_antisymmetry():
    import atlasqtl_amd as A
    for n in (64, 65, 1000, 20000):
        y = np.random.default_rng(n).standard_normal((n, 1))
        out = A.rank_normalize(y)["Y"][:, 0]
        s = out[np.argsort(y[:, 0])]
        assert same_bits(s, -s[::-1] + 0.0), n                 # (+ 0.0: the middle rank of an odd n is +0.0 on both sides)
        assert np.all(np.diff(s) > 0) and (n % 2 == 0 or s[n // 2] == 0.0)


def _run_child(path, tmp_path):
    out = str(tmp_path / f"{path}.npz")
    env = dict(os.environ, AQ_YT_PATH=path)
    shapes = [f"{n},{q}" for n, q in PATH_CASES]
    r = subprocess.run([sys.executable, "-m", "tests.yt_path_child", out] + shapes, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


def test_path_independence(tmp_path):
    lds, glob = _run_child("lds", tmp_path), _run_child("global", tmp_path)
    for n, q in PATH_CASES:
        s = f"{n},{q}"
        assert int(lds[f"path_{s}"]) == 0 and int(glob[f"path_{s}"]) == 1
        assert np.array_equal(lds[f"Y_{s}"], glob[f"Y_{s}"], equal_nan=True) and same_bits(lds[f"Y_{s}"], glob[f"Y_{s}"])
        assert np.array_equal(lds[f"n_obs_{s}"], glob[f"n_obs_{s}"]) and np.array_equal(lds[f"n_tied_{s}"], glob[f"n_tied_{s}"])
        assert same_bits(lds[f"Y_{s}"], expected_bits(YU.columns(n, q), 0.375))


@pytest.mark.parametrize("c", [0.0, 0.375, 0.5])
def test_offsets(c):
    import atlasqtl_amd as A
    Y = YU.columns(65, 5)
    check_against_restatement(Y, A.rank_normalize(Y, offset=c), c, f"c={c}")


def test_errors():
    import atlasqtl_amd as A
    from atlasqtl_amd import prepare as P
    rng = np.random.default_rng(5)
    n, p, q = 65, 40, 5
    X = rng.binomial(2, 0.3, size=(n, p)).astype(float)
    msg = "column {} of Y has fewer than two distinct observed values; it cannot be rank-normalised"
    Y = rng.standard_normal((n, q))
    Y[:, 2] = 7.0                                               # all equal
    with pytest.raises(A.AtlasqtlError, match=msg.format(3)):
        A.rank_normalize(Y)
    with pytest.raises(A.AtlasqtlError, match=msg.format(3)):
        P.prepare_on_device(Y, X, transform_y="int")
    Y[:, 2] = np.where(rng.random(n) < 0.5, 0.0, -0.0)          # the two zeros are one value
    with pytest.raises(A.AtlasqtlError, match=msg.format(3)):
        A.rank_normalize(Y)
    Y = rng.standard_normal((n, q))
    Y[:, 4] = np.nan
    Y[11, 4] = 1.0                                              # one observed value among NaN
    with pytest.raises(A.AtlasqtlError, match=msg.format(5)):
        A.rank_normalize(Y)
    with pytest.raises(A.AtlasqtlError, match=r"Column\(s\) 5 of matrix Y have more than 97.5% missing values"):
        P.prepare_on_device(Y, X, transform_y="int")             # the guard comes first, with its own message
    Y[:, 4] = np.nan
    Y[:5, 4] = 3.0                                              # passes the guards (5 / 65 observed), all equal
    with pytest.raises(A.AtlasqtlError, match=msg.format(5)):
        P.prepare_on_device(Y, X, transform_y="int")
    Y[:, :] = np.nan
    Y[0, :] = 1.0
    with pytest.raises(A.AtlasqtlError, match="Too few non-NA values in matrix Y"):
        P.prepare_on_device(Y, X, transform_y="int")


def _prep(Y, X, **kw):
    from atlasqtl_amd import prepare as P
    prep, cst, coll, dup = P.prepare_on_device(Y, X, **kw)
    try:
        return dict(Xs=prep.X_host(), Yc=prep.Y.copy(), cst=cst, coll=coll, dup=dup, n_obs=prep.y_n_obs, n_tied=prep.y_n_tied)
    finally:
        prep.close()


def _same_preparation(a, b, plain):
    assert same_bits(a["Yc"], b["Yc"])
    for k in ("Xs", "cst", "coll", "dup"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], plain[k]), k
    assert same_bits(a["Xs"], plain["Xs"])
    assert not same_bits(a["Yc"], plain["Yc"])                   # the option does something


def test_prepare_path():
    import atlasqtl_amd as A
    from tests import cov_util as CU
    rng = np.random.default_rng(9)
    n, p, q = 65, 40, 5
    X = rng.binomial(2, 0.3, size=(n, p)).astype(float)
    X[:, 7] = X[:, 3]
    Y = np.exp(rng.standard_normal((n, q)))
    Y[rng.random((n, q)) < 0.1] = np.nan
    Y[:, 1] = np.round(Y[:, 1])                                  # ties
    rn = A.rank_normalize(Y)
    a, b, plain = _prep(Y, X, transform_y="int"), _prep(rn["Y"], X), _prep(Y, X)
    _same_preparation(a, b, plain)
    assert np.array_equal(a["n_obs"], rn["n_obs"]) and np.array_equal(a["n_tied"], rn["n_tied"])
    assert np.array_equal(a["n_obs"], YU.tied_counts(Y)[0]) and b["n_obs"] is None and plain["n_tied"] is None
    Z = CU.covariates(n, 3, rng)
    _same_preparation(_prep(Y, X, covariates=Z, transform_y="int"), _prep(rn["Y"], X, covariates=Z), _prep(Y, X, covariates=Z))
    c = _prep(Y, X, transform_y={"method": "int", "offset": 0.5})
    assert same_bits(c["Yc"], _prep(A.rank_normalize(Y, offset=0.5)["Y"], X)["Yc"]) and not same_bits(c["Yc"], a["Yc"])
    bed = lambda: A.PlinkBed(TOY, missing="mean")                # 6 samples x 3 variants
    Yb = np.exp(rng.standard_normal((6, 3)))
    Yb[2, 1] = np.nan
    _same_preparation(_prep(Yb, bed(), transform_y="int"), _prep(A.rank_normalize(Yb)["Y"], bed()), _prep(Yb, bed()))


def test_whole_run():
    import atlasqtl_amd as A
    from atlasqtl_amd import synth
    d = synth.simulate(100, 75, 20, p_act=10, seed=123, prob_assoc=1.0)      # the size of the toy goldens
    Y = np.exp(d["Y"] / d["Y"].std())
    Y[np.random.default_rng(3).random(Y.shape) < 0.03] = np.nan
    kw = dict(p0=(5, 25), user_seed=4, verbose=0)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        a = A.atlasqtl(Y, d["X"], transform_y="int", **kw)
    assert not [w for w in caught if "transform_y" in str(w.message)]      # continuous traits: no tie warning
    b = A.atlasqtl(A.rank_normalize(Y)["Y"], d["X"], **kw)
    assert a["it"] == b["it"] and a["converged"] and np.array_equal(a["gam_vb"], b["gam_vb"])
    assert a["transform_y"] == {"method": "int", "offset": 0.375}
    n_obs, n_tied = YU.tied_counts(Y)
    assert np.array_equal(a["y_n_obs"], n_obs) and np.array_equal(a["y_n_tied"], n_tied)
    for key in ("transform_y", "y_n_obs", "y_n_tied"):
        assert key not in b
    s = A.atlasqtl(Y, d["X"], transform_y={"method": "int"}, sparse_output={"thres": 0.5}, **kw)
    assert s["it"] == a["it"] and s["assoc"]["n_pairs"] == int((a["gam_vb"] > 0.5).sum()) and s["transform_y"] == a["transform_y"]


def test_tie_warning():
    import atlasqtl_amd as A
    from atlasqtl_amd import synth
    d = synth.simulate(100, 75, 20, p_act=10, seed=123, prob_assoc=1.0)
    Y = d["Y"].copy()
    Y[:, 6] = np.round(Y[:, 6] / Y[:, 6].std())                  # an integer-valued trait: a handful of distinct values
    with pytest.warns(UserWarning, match=r"transform_y: more than half of the observed values are tied in 1 response\(s\) \(Resp_7\)"):
        res = A.atlasqtl(Y, d["X"], p0=(5, 25), user_seed=4, verbose=0, transform_y="int")
    assert 2 * res["y_n_tied"][6] > res["y_n_obs"][6] and np.all(res["y_n_tied"][np.arange(20) != 6] == 0)
