"""Host: prediction (aq_vb_predict, aq_vb_fitted, aq_predict; atlasqtl(predict=, fitted=, keep_predictor=), predict()) as far
as it needs no device -- the symbols and the export, the launch plan of aq_predict_plan_query, the argument errors of the C
entries, and every refusal of the Python layer, all of which come before the first device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import atlasqtl_amd as A
from atlasqtl_amd import _lib, prediction
from atlasqtl_amd.prepare import AtlasqtlError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    txt = open(os.path.join(ROOT, "include", "atlasqtl_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(aq_[a-z0-9_]+)\s*\(", txt))


ENTRIES = ("aq_predict_plan_query", "aq_vb_predict", "aq_vb_fitted", "aq_predict", "aq_vb_predict_time")
N_MAX = 82944


# ---- ABI and export ----
def test_symbols_in_header_binding_and_library(hiplib):
    names = declared_functions()
    for name in ENTRIES:
        assert name in names and name in _lib.SYMBOLS and hasattr(hiplib, name), name
    # the binding's copy of AQ_N_MAX against the header that defines it
    const = open(os.path.join(ROOT, "atlasqtl_amd", "csrc", "aq_plan_const.h")).read()
    cmax = int(re.search(r"AQ_LA_CMAX = (\d+)", const).group(1))
    a, b = re.search(r"AQ_N_MAX = AQ_LA_CMAX \* (\d+) \* (\d+)", const).groups()
    assert _lib.AQ_N_MAX == cmax * int(a) * int(b) == N_MAX and prediction.PREDICT_MAX_ROWS == _lib.AQ_N_MAX


def test_export():
    assert "predict" in A.__all__ and A.predict is prediction.predict
    assert callable(A.VbRun.predict) and callable(A.VbRun.fitted)


def test_plan_struct_and_binding_agree():
    txt = open(os.path.join(ROOT, "include", "atlasqtl_hip.h")).read()
    body = re.search(r"typedef struct aq_predict_plan \{(.*?)\} aq_predict_plan;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    fields = [(d.split()[1], ctype[d.split()[0]]) for d in body.split(";") if d.strip()]
    assert fields == list(_lib.AqPredictPlan._fields_)
    assert C.sizeof(_lib.AqPredictPlan) == 8 * 4 + 2 * 8


def test_the_unit_is_in_the_build_and_behind_the_isa_check():
    mk = open(os.path.join(ROOT, "atlasqtl_amd", "csrc", "Makefile")).read()
    assert "$(BUILD)/aq_predict.o" in mk.split("OUT    =")[0]                      # among the objects of the library
    link = re.search(r"^\$\(OUT\):(.*)$", mk, flags=re.M).group(1)
    assert "$(BUILD)/aq_predict.isa_ok" in link                                    # the link waits for the checker's stamp
    assert "check_isa_operands.py --quiet $(BUILD)/aq_predict-hip-amdgcn-amd-amdhsa-$(ARCH).s" in mk
    plan = open(os.path.join(ROOT, "atlasqtl_amd", "csrc", "aq_predict_plan.h")).read()
    assert "hip/" not in plan and "getenv" not in re.sub(r"//[^\n]*", "", plan)    # pure: no HIP header, no environment


# ---- the plan ----
def _plan(hiplib, n_new, p, q, ncu=256):
    pl = _lib.AqPredictPlan()
    rc = hiplib.aq_predict_plan_query(n_new, p, q, ncu, C.byref(pl))
    return rc, pl


SHAPES = [(1, 5, 1), (15, 16, 16), (17, 33, 17), (130, 257, 40), (64, 1000, 130), (35, 33, 17), (1000, 50000, 10000),
          (N_MAX, 50000, 10000), (257, 1, 1), (2000, 700, 33)]


@pytest.mark.parametrize("n_new,p,q", SHAPES)
@pytest.mark.parametrize("ncu", [1, 64, 256, 304])
def test_plan_fields(hiplib, n_new, p, q, ncu, monkeypatch):
    monkeypatch.delenv("AQ_PREDICT_SPLITS", raising=False)
    rc, pl = _plan(hiplib, n_new, p, q, ncu)
    assert rc == 0, hiplib.aq_last_error()
    tiles_n, tiles_q = -(-n_new // 16), -(-q // 16)
    # the sample blocks cover every row once: block b owns the tiles [b sample_tiles, (b + 1) sample_tiles)
    assert pl.sample_tiles in (4, 8, 16) and pl.sample_blocks == -(-tiles_n // pl.sample_tiles)
    assert pl.n_pad == 16 * pl.sample_tiles * pl.sample_blocks and n_new <= pl.n_pad < n_new + 16 * pl.sample_tiles
    owner = np.repeat(np.arange(pl.sample_blocks), 16 * pl.sample_tiles)[:n_new]   # the block of every row
    assert owner.size == n_new and (np.bincount(owner, minlength=pl.sample_blocks)[:-1] == 16 * pl.sample_tiles).all()
    # as many accumulator rows per wave as the samples fill
    assert pl.sample_tiles == (16 if tiles_n > 8 else 8 if tiles_n > 4 else 4)
    # the trait groups cover every tile once; two tiles per workgroup only where every CU still gets workgroups
    assert pl.trait_tiles in (1, 2) and pl.trait_groups == -(-tiles_q // pl.trait_tiles) and tiles_q <= 65535
    assert (pl.trait_tiles == 2) == (tiles_q >= 2 and pl.sample_blocks * tiles_q >= 4 * ncu)
    # the splits cover every predictor exactly once: split s owns the chunks [s cps, (s + 1) cps)
    chunks = -(-p // pl.chunk)
    assert pl.chunk == 16 and 1 <= pl.splits <= 64 and pl.chunks_per_split == -(-chunks // pl.splits)
    lo = np.minimum(np.arange(pl.splits, dtype=np.int64) * pl.chunks_per_split * 16, p)
    hi = np.minimum(lo + pl.chunks_per_split * 16, p)
    assert lo[0] == 0 and hi[-1] == p and (lo[1:] == hi[:-1]).all() and int((hi - lo).sum()) == p
    # one split when the tiles alone give two workgroups per CU; otherwise no more workgroups than that needs, and no split
    # the plan chose itself is shorter than 8 chunks
    wgs = pl.sample_blocks * pl.trait_groups
    if wgs >= 2 * ncu:
        assert pl.splits == 1
    else:
        assert (pl.splits - 1) * wgs < 2 * ncu
    assert pl.splits == 1 or pl.splits <= chunks // 8
    # the memory follows from the fields
    p_pad = 16 * -(-p // 16)
    assert pl.panel_bytes == pl.n_pad * p_pad * 8
    assert pl.scratch_bytes == pl.splits * tiles_q * pl.n_pad * 16 * 8
    rc2, pl2 = _plan(hiplib, n_new, p, q, ncu)
    assert rc2 == 0 and bytes(pl) == bytes(pl2)


@pytest.mark.parametrize("splits", [1, 3, 64])
@pytest.mark.parametrize("n_new,p,q", SHAPES[:7])
def test_forced_splits_are_honoured(hiplib, n_new, p, q, splits, monkeypatch):
    """AQ_PREDICT_SPLITS = 1, 3, 64 whatever p and the CU count say (at p = 5 all but the first split are empty); the splits
    still cover every predictor exactly once and the scratch follows from them."""
    monkeypatch.setenv("AQ_PREDICT_SPLITS", str(splits))
    rc, pl = _plan(hiplib, n_new, p, q)
    assert rc == 0, hiplib.aq_last_error()
    chunks = -(-p // 16)
    assert pl.splits == splits and pl.chunks_per_split == -(-chunks // splits)
    lo = np.minimum(np.arange(splits, dtype=np.int64) * pl.chunks_per_split * 16, p)
    hi = np.minimum(lo + pl.chunks_per_split * 16, p)
    assert lo[0] == 0 and hi[-1] == p and (lo[1:] == hi[:-1]).all() and int((hi - lo).sum()) == p
    assert pl.scratch_bytes == splits * -(-q // 16) * pl.n_pad * 16 * 8
    monkeypatch.delenv("AQ_PREDICT_SPLITS")
    rc, own = _plan(hiplib, n_new, p, q)
    assert rc == 0 and (own.sample_tiles, own.trait_tiles, own.sample_blocks, own.trait_groups, own.n_pad, own.panel_bytes) == \
        (pl.sample_tiles, pl.trait_tiles, pl.sample_blocks, pl.trait_groups, pl.n_pad, pl.panel_bytes)      # nothing else moves


def test_forced_splits_out_of_range_are_refused(hiplib, monkeypatch):
    for bad in ("0", "65", "-3", "x"):
        monkeypatch.setenv("AQ_PREDICT_SPLITS", bad)
        rc, _ = _plan(hiplib, 64, 1000, 130)
        assert rc == 1 and "aq_predict_plan_query: AQ_PREDICT_SPLITS must lie in [1, 64]" in hiplib.aq_last_error().decode()


def test_plan_at_the_shapes_it_is_for(hiplib, monkeypatch):
    monkeypatch.delenv("AQ_PREDICT_SPLITS", raising=False)
    rc, pl = _plan(hiplib, 1000, 50000, 10000)
    assert rc == 0 and (pl.sample_tiles, pl.trait_tiles, pl.sample_blocks, pl.trait_groups, pl.splits) == (16, 2, 4, 313, 1)
    assert pl.panel_bytes == 1024 * 50000 * 8 and pl.scratch_bytes == 625 * 1024 * 16 * 8
    rc, pl = _plan(hiplib, 64, 1000, 130)                  # 9 workgroups, 63 chunks: no split below 8 chunks
    assert rc == 0 and (pl.sample_tiles, pl.trait_tiles, pl.sample_blocks, pl.trait_groups, pl.splits) == (4, 1, 1, 9, 7)
    rc, pl = _plan(hiplib, 1, 5, 1)
    assert rc == 0 and (pl.sample_blocks, pl.trait_groups, pl.splits, pl.chunks_per_split, pl.n_pad) == (1, 1, 1, 1, 64)
    assert prediction.plan_query(1000, 50000, 10000)["splits"] == 1


def test_plan_argument_errors(hiplib, monkeypatch):
    monkeypatch.delenv("AQ_PREDICT_SPLITS", raising=False)
    assert hiplib.aq_predict_plan_query(10, 10, 4, 256, None) == 1
    assert "aq_predict_plan_query" in hiplib.aq_last_error().decode() and "NULL" in hiplib.aq_last_error().decode()
    for n_new, p, q, ncu in ((0, 10, 4, 256), (-1, 10, 4, 256), (N_MAX + 1, 10, 4, 256), (10, 0, 4, 256), (10, 10, 0, 256),
                             (10, 10, 4, 0)):
        rc, _ = _plan(hiplib, n_new, p, q, ncu)
        msg = hiplib.aq_last_error().decode()
        assert rc == 1 and "aq_predict_plan_query" in msg and "82944" in msg
    assert _plan(hiplib, N_MAX, 10, 1)[0] == 0
    assert _plan(hiplib, 16, 10, 16 * 65535, 256)[0] == 0
    for ncu in (1, 256):                                   # more trait tiles than the y dimension of the reduce kernel's grid holds
        rc, _ = _plan(hiplib, 16, 10, 16 * 65535 + 1, ncu)
        assert rc == 3 and "exceeds 1048560 traits" in hiplib.aq_last_error().decode()
    with pytest.raises(AtlasqtlError, match="aq_predict_plan_query"):
        prediction.plan_query(0, 10, 4)


# ---- the C entries: NULL and shape errors return 1 with a message, without a device ----
def test_argument_errors_of_the_entries_come_before_the_device(hiplib):
    X, X8, Yh, v = np.zeros((3, 2), order="F"), np.zeros((3, 2), dtype=np.int8, order="F"), np.zeros((3, 4), order="F"), np.ones(2)
    beta = np.zeros((2, 4), order="F")
    dp, i8 = _lib.as_dp, lambda a: a.ctypes.data_as(C.POINTER(C.c_int8))

    def err(rc, who, what):
        msg = hiplib.aq_last_error().decode()
        assert rc == 1 and who in msg and what in msg, (rc, msg)

    err(hiplib.aq_vb_predict(None, dp(X), None, 3, None, None, dp(Yh)), "aq_vb_predict", "NULL handle")
    err(hiplib.aq_vb_fitted(None, None, dp(Yh)), "aq_vb_fitted", "NULL handle")
    ms = C.c_double(0.0)
    err(hiplib.aq_vb_predict_time(None, 3, 1, C.byref(ms), None), "aq_vb_predict_time", "NULL")
    args = lambda **kw: [kw.get("beta", dp(beta)), kw.get("p", 2), kw.get("q", 4), kw.get("X", dp(X)), kw.get("X8", None),  # noqa: E731
                         kw.get("n", 3), kw.get("c", None), kw.get("s", None), kw.get("out", dp(Yh)), 0]
    err(hiplib.aq_predict(*args(beta=None)), "aq_predict", "NULL handle or beta_vb")
    err(hiplib.aq_predict(*args(X=None)), "aq_predict", "NULL matrix")
    err(hiplib.aq_predict(*args(out=None)), "aq_predict", "NULL output")
    err(hiplib.aq_predict(*args(p=0)), "aq_predict", "p >= 1")
    err(hiplib.aq_predict(*args(q=0)), "aq_predict", "q >= 1")
    err(hiplib.aq_predict(*args(n=0)), "aq_predict", "n_new must lie in [1, 82944]")
    err(hiplib.aq_predict(*args(n=N_MAX + 1)), "aq_predict", "n_new must lie in [1, 82944]")
    err(hiplib.aq_predict(*args(c=dp(v))), "aq_predict", "both")
    err(hiplib.aq_predict(*args(s=dp(v))), "aq_predict", "both")
    for bad in (0.0, -1.0, np.inf, np.nan):
        err(hiplib.aq_predict(*args(c=dp(v), s=dp(np.array([1.0, bad])))), "aq_predict", "predictor 2")
    err(hiplib.aq_predict(*args(c=dp(np.array([np.nan, 0.0])), s=dp(v))), "aq_predict", "predictor 1")
    if hiplib.aq_device_count() == 0:                      # a well-formed call reaches the device, and says that there is none
        assert hiplib.aq_predict(*args(X=None, X8=i8(X8), c=dp(v), s=dp(v))) == 2
        assert "no HIP device" in hiplib.aq_last_error().decode()


# ---- the refusals of the Python layer ----
def _data(n=40, p=9, q=2, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, q)), rng.normal(size=(n, p))


KW = dict(p0=(2, 4), verbose=0)


def test_predict_with_covariates_or_genotype_pcs_is_refused():
    Y, X = _data()
    Z = np.random.default_rng(1).normal(size=(40, 2))
    for extra in (dict(covariates=Z), dict(genotype_pcs=2), dict(covariates=Z, genotype_pcs={"k": 1})):
        with pytest.raises(AtlasqtlError, match="predict= cannot be combined with covariates= or genotype_pcs=.*covariate coefficients"):
            A.atlasqtl(Y, X, predict=X[:3], **extra, **KW)
        with pytest.raises(AtlasqtlError, match="keep_predictor=True cannot be combined with covariates= or genotype_pcs="):
            A.atlasqtl(Y, X, keep_predictor=True, **extra, **KW)


def test_wrong_columns_nan_and_shapes_are_refused_before_the_device():
    Y, X = _data()
    with pytest.raises(AtlasqtlError, match="predict has 8 columns, but the fit was given 9 predictors"):
        A.atlasqtl(Y, X, predict=X[:3, :8], **KW)
    with pytest.raises(AtlasqtlError, match="predict has 10 columns"):
        A.atlasqtl(Y, X, predict=np.zeros((3, 10), dtype=np.int8), **KW)
    bad = X[:3].copy()
    bad[1, 4] = np.nan
    with pytest.raises(AtlasqtlError, match="predict must be finite, without missing values"):
        A.atlasqtl(Y, X, predict=bad, **KW)
    for inf in (np.inf, -np.inf):
        bad_inf = X[:3].copy()
        bad_inf[2, 0] = inf
        with pytest.raises(AtlasqtlError, match="predict must be finite"):
            A.atlasqtl(Y, X, predict=bad_inf, **KW)
    # X itself may be anything that converts to a matrix, a nested list for instance: the column count is read from its shape
    with pytest.raises(AtlasqtlError, match="predict has 8 columns, but the fit was given 9 predictors"):
        A.atlasqtl(Y, X.tolist(), predict=X[:3, :8], **KW)
    for shape_bad in (X[0], np.zeros((0, 9)), np.zeros((2, 9, 1))):
        with pytest.raises(AtlasqtlError, match="non-empty numeric matrix"):
            A.atlasqtl(Y, X, predict=shape_bad, **KW)
    with pytest.raises(AtlasqtlError, match="numeric matrix"):
        A.atlasqtl(Y, X, predict=[["a"] * 9], **KW)
    # the same checks guard the core's own argument and the matrix-level call
    prob_hyper = dict(A2_inv=1.0, m0=0.0, nu=1.0, rho=1.0, t02=1.0, eta=1.0, kappa=1.0, n0=-1.0)
    with pytest.raises(AtlasqtlError, match="predict has 8 columns"):
        A.atlasqtl_global_local_core_(Y, X, 2, None, 1, 0.1, 5, 0, prob_hyper, {}, predict=X[:3, :8])
    with pytest.raises(AtlasqtlError, match="missing values"):
        A.atlasqtl_global_local_core_(Y, X, 2, None, 1, 0.1, 5, 0, prob_hyper, {}, predict={"X": bad})
    assert prediction.check_x_new(np.ones((2, 9), dtype=np.int8), 9).dtype == np.int8
    assert prediction.check_x_new(np.ones((2, 9), dtype=np.int32), 9).dtype == np.float64


def test_a_plinkbed_as_x_new_is_refused():
    bed = object.__new__(A.PlinkBed)                       # the check looks at the type alone
    with pytest.raises(AtlasqtlError, match="PlinkBed is not supported for prediction"):
        prediction.check_x_new(bed, 9)


def _dense_result(p_given=6, kept=(0, 2, 3, 5), q=3):
    rng = np.random.default_rng(2)
    return dict(beta_vb=np.asfortranarray(rng.normal(size=(len(kept), q))),
                predictor=dict(kept_x=np.array(kept), x_center=np.zeros(len(kept)), x_scale=np.ones(len(kept)), p_given=p_given))


def test_predict_refuses_what_it_cannot_apply():
    X_new = np.zeros((2, 6))
    res = _dense_result()
    sparse = {k: v for k, v in res.items() if k != "beta_vb"}
    sparse["assoc"] = {}
    with pytest.raises(AtlasqtlError, match="a sparse result holds no beta_vb.*predict=X_new"):
        A.predict(sparse, X_new)
    with pytest.raises(AtlasqtlError, match="keep_predictor=True"):
        A.predict({"beta_vb": res["beta_vb"]}, X_new)
    back = dict(res, names_x_all=[f"x{j}" for j in range(5)], beta_vb=np.zeros((5, 3)))
    with pytest.raises(AtlasqtlError, match="add_collinear_back=True.*count twice"):
        A.predict(back, X_new)
    with pytest.raises(AtlasqtlError, match="add_collinear_back=True"):
        A.predict(dict(res, beta_vb=np.zeros((5, 3))), X_new)      # rows that the kept columns do not explain
    with pytest.raises(AtlasqtlError, match="X_new has 4 columns, but the fit was given 6 predictors"):
        A.predict(res, np.zeros((2, 4)))
    with pytest.raises(AtlasqtlError, match="missing values"):
        A.predict(res, np.full((2, 6), np.nan))
    with pytest.raises(AtlasqtlError, match="PlinkBed"):
        A.predict(res, object.__new__(A.PlinkBed))
    if _lib.lib().aq_device_count() == 0:                  # a well-formed call gets as far as the device
        with pytest.raises(_lib.AtlasqtlHipError, match="no HIP device"):
            A.predict(res, X_new)
        with pytest.raises(_lib.AtlasqtlHipError, match="no HIP device"):
            A.predict(res, X_new.astype(np.int8))


def test_predictor_of_and_the_standardisation_arguments():
    rm = np.array([False, True, False, False, True, False])
    pr = prediction.predictor_of(rm, np.arange(6.0), 10 + np.arange(6.0))
    assert set(pr) == {"kept_x", "x_center", "x_scale", "p_given"}
    np.testing.assert_array_equal(pr["kept_x"], [0, 2, 3, 5])
    np.testing.assert_array_equal(pr["x_center"], [0, 2, 3, 5])
    np.testing.assert_array_equal(pr["x_scale"], [10, 12, 13, 15])
    assert pr["p_given"] == 6
    X = np.zeros((3, 4))
    with pytest.raises(AtlasqtlError, match="both be given or both be None"):
        prediction.apply_in_batches(None, X, 2, center=np.zeros(4))
    with pytest.raises(AtlasqtlError, match="one value per predictor"):
        prediction.apply_in_batches(None, X, 2, center=np.zeros(3), scale=np.ones(3))


def test_row_batches_cover_every_row_once(monkeypatch):
    """The host loop: batches of at most PREDICT_MAX_ROWS rows, in order, each written to its own rows of the result."""
    monkeypatch.setattr(prediction, "PREDICT_MAX_ROWS", 16)
    X = np.asfortranarray(np.arange(35 * 3, dtype=np.float64).reshape(35, 3))
    seen = []

    def call(xd, x8, n_rows, c, s, out):
        assert x8 is None and not c and not s
        xb = np.ctypeslib.as_array(xd, shape=(3, n_rows)).T
        seen.append(n_rows)
        np.ctypeslib.as_array(out, shape=(2, n_rows)).T[:] = xb[:, :2] + 1

    got = prediction.apply_in_batches(call, X, 2)
    assert seen == [16, 16, 3]
    np.testing.assert_array_equal(got, X[:, :2] + 1)
    X8 = np.asfortranarray((np.arange(20 * 2) % 3).reshape(20, 2).astype(np.int8))
    seen8 = []

    def call8(xd, x8, n_rows, c, s, out):
        assert not xd and c and s
        seen8.append(np.ctypeslib.as_array(x8, shape=(2, n_rows)).T.copy())
        np.ctypeslib.as_array(out, shape=(1, n_rows)).T[:] = 0

    prediction.apply_in_batches(call8, X8, 1, np.zeros(2), np.ones(2))
    np.testing.assert_array_equal(np.vstack(seen8), X8)


def test_no_new_key_unless_asked():
    """The three arguments are off by default, in atlasqtl() and in the core (tests/test_gpu_predict.py checks the keys of
    the results)."""
    import inspect
    sig = inspect.signature(A.atlasqtl)
    assert sig.parameters["predict"].default is None and sig.parameters["fitted"].default is False
    assert sig.parameters["keep_predictor"].default is False
    core = inspect.signature(A.atlasqtl_global_local_core_)
    assert core.parameters["predict"].default is None and core.parameters["fitted"].default is False
