"""GPU: prediction -- Yhat = Xt (gam_vb * mu_beta_vb) read in place from a handle (VbRun.predict / fitted, atlasqtl(predict=,
fitted=)) and from a dense result (predict()) -- against a yardstick computed independently of the package, in long double,
from the dense beta_vb of the same run (tests/predict_util.py, where the bound is derived), at shapes chosen for the kernels'
edges: one row, one predictor tile short of full, one past a tile in every dimension, more than one sample block, more than
one trait group and a ragged last trait tile; with the plan's own splits and with 1, 3 and 64 forced ones (at p = 5 all but
one are empty)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import predict_util as PU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("AQ_PREDICT_SPLITS", "AQ_KERNEL", "AQ_NCU")


def _child(tmp_path, shapes, **env):
    out = str(tmp_path / "y.npz")
    names = [",".join(str(v) for v in shape) for shape in shapes]
    r = subprocess.run([sys.executable, "-m", "tests.predict_child", out] + names, env=dict(os.environ, **env), cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    return [{k: got[f"{k}_{name}"] for k in ("beta", "y8", "y8b", "y64", "yd", "splits", "sample_tiles", "trait_tiles", "core_kernel")} for name in names]


# ---- the kernels at their edges ----
@pytest.mark.parametrize("n_new,p,q", PU.SHAPES)
def test_edge_shapes_with_the_plans_own_splits(n_new, p, q, monkeypatch):
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    out = PU.run_shape(n_new, p, q)
    from atlasqtl_amd import prediction
    assert out["splits"] == prediction.plan_query(n_new, p, q, ncu=_ncu())["splits"]
    PU.check_shape(out, n_new, p, q, f"n_new={n_new} p={p} q={q}")


# Two trait tiles per workgroup need sample_blocks x trait tiles >= 4 CUs: AQ_NCU = 1 for the prediction calls brings that down
# to these shapes.  An odd number of trait tiles (5, the last one ragged: the second tile of the last group does not exist)
# with 1, 2 and 4 accumulator rows per wave (n_new = 17, 100 in 65 ... 128, 130), and an even one.
TT2_SHAPES = [(17, 33, 70, 4), (100, 33, 70, 8), (130, 257, 72, 16), (64, 100, 64, 4)]       # (n_new, p, q, sample_tiles)


@pytest.mark.parametrize("n_new,p,q,st", TT2_SHAPES)
def test_two_trait_tiles_per_workgroup(n_new, p, q, st, monkeypatch):
    """The <NS, 2> instances, with mu (the handle) and without (the dense result), against the same yardstick."""
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    out = PU.run_shape(n_new, p, q, ncu=1)
    assert (out["trait_tiles"], out["sample_tiles"], out["splits"]) == (2, st, 1)
    PU.check_shape(out, n_new, p, q, f"TT=2 n_new={n_new} p={p} q={q}")


def test_eight_sample_tiles_per_workgroup(monkeypatch):
    """n_new in 65 ... 128 with the device's own CU count: <2, 1>."""
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    out = PU.run_shape(100, 257, 40)
    assert (out["trait_tiles"], out["sample_tiles"]) == (1, 8)
    PU.check_shape(out, 100, 257, 40, "n_new=100 p=257 q=40")


@functools.lru_cache(maxsize=None)
def _ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("splits", [1, 3, 64])
def test_forced_splits_in_a_fresh_process(splits, tmp_path):
    """AQ_PREDICT_SPLITS = 1, 3 and 64 in a child process of its own: the entries' plan has that many splits and every shape
    stays within the same bound."""
    for (n_new, p, q), out in zip(PU.SHAPES, _child(tmp_path, PU.SHAPES, AQ_PREDICT_SPLITS=str(splits))):
        assert int(out["splits"]) == splits
        PU.check_shape(out, n_new, p, q, f"S={splits} n_new={n_new} p={p} q={q}")


@pytest.mark.parametrize("kernel", [2, 3])
def test_handles_of_the_two_other_sweep_kernels(kernel, tmp_path):
    """AQ_KERNEL = 2 (generic) and 3 (masked two-barrier, which the plan takes only for Y with missing values) keep gam_vb /
    mu_beta_vb in the same trait-tiled layout as the look-ahead kernel (aq_vb_create allocates and fills them the same way
    whatever the kernel; aq_vb_get_result reads them the same way for all three), so the same entries serve them."""
    na = kernel == 3
    (out,) = _child(tmp_path, [(17, 33, 17, int(na))], AQ_KERNEL=str(kernel))
    assert int(out["core_kernel"]) == kernel
    PU.check_shape(out, 17, 33, 17, f"AQ_KERNEL={kernel}", na=na)


def _handle(p, q, sweeps=2, na=False, **kw):
    from atlasqtl_amd.core import VbRun
    c = PU.fit_case(p, q, na)
    return c, VbRun(c["Y"], c["X"], c["list_hyper"], c["list_init"], None, 0.1, sweeps, True, True, **kw)


def test_row_batches_give_the_bits_of_one_call(monkeypatch):
    """n_new = 2 x 16 + 3 rows in batches of 16, 16 and 3 against one call (p = 33: one split in every plan, so the order of
    summation of an entry does not depend on the batch it is in)."""
    from atlasqtl_amd import prediction
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    c, run = _handle(33, 17)
    try:
        run.run()
        Xn = PU.new_rows(35, 33)
        whole = run.predict(Xn, c["center"], c["scale"])
        monkeypatch.setattr(prediction, "PREDICT_MAX_ROWS", 16)
        for X in (Xn, Xn.astype(np.float64)):
            assert run.predict(X, c["center"], c["scale"]).tobytes() == whole.tobytes()
        want, bound = PU.yardstick(Xn, c["center"], c["scale"], run.result()["beta_vb"])
        PU.assert_within(whole, want, bound, "35 rows")
    finally:
        run.close()


def test_two_calls_give_the_same_bits_with_several_splits(monkeypatch):
    monkeypatch.delenv("AQ_KERNEL", raising=False)
    monkeypatch.setenv("AQ_PREDICT_SPLITS", "3")
    c, run = _handle(1000, 130)
    try:
        run.run()
        Xn = PU.new_rows(64, 1000)
        a, b = (run.predict(Xn, c["center"], c["scale"]) for _ in range(2))
        assert a.tobytes() == b.tobytes()
        want, bound = PU.yardstick(Xn, c["center"], c["scale"], run.result()["beta_vb"])
        PU.assert_within(a, want, bound, "S=3 64 x 1000 x 130")
        # already standardised rows: center and scale None
        Xt = np.asfortranarray((Xn.astype(np.float64) - c["center"]) / c["scale"])
        want, bound = PU.yardstick(Xt, 0.0, 1.0, run.result()["beta_vb"])
        PU.assert_within(run.predict(Xt), want, bound, "standardised input")
    finally:
        run.close()


def test_a_trait_shard_returns_its_own_columns(monkeypatch):
    """A handle that holds the traits [16, 33) of 33 (trait_offset 16, q_total 33: what a rank of a trait-sharded run holds;
    there is no prediction in the one-process multi-GPU entry) predicts its own 17 columns."""
    from atlasqtl_amd.core import VbRun
    from tests.util import shard_lists
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    c = PU.fit_case(70, 33)
    lh, li = shard_lists(c["list_hyper"], c["list_init"], 16, 33)
    run = VbRun(np.asfortranarray(c["Y"][:, 16:33]), c["X"], lh, li, None, 0.1, 2, True, True, q_total=33, trait_offset=16)
    try:
        run.run()
        Xn = PU.new_rows(21, 70)
        got = run.predict(Xn, c["center"], c["scale"])
        assert got.shape == (21, 17)
        want, bound = PU.yardstick(Xn, c["center"], c["scale"], run.result()["beta_vb"])
        PU.assert_within(got, want, bound, "shard [16, 33)")
    finally:
        run.close()


# ---- fitted values ----
@pytest.mark.parametrize("na", [False, True])
def test_fitted_values_on_the_prepared_matrix(na, monkeypatch):
    """X_beta_vb from the standardised matrix where it lies on the device (aq_vb_fitted) against the yardstick on that matrix;
    for complete Y also against Yc - residual, the residual being what the sweeps carry: they agree up to its drift, for which
    tests/test_gpu_bigp.py allows 1e-10 of the trait's rms."""
    from atlasqtl_amd import hyper_init as H
    from atlasqtl_amd import prepare as P
    from atlasqtl_amd.core import VbRun
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    n, p, q = 130, 70, 20
    G = PU.dosages(n, p, seed=11)
    rng = np.random.default_rng(12)
    Y = G[:, :3].astype(np.float64) @ rng.normal(size=(3, q)) + rng.normal(size=(n, q))
    if na:
        Y[rng.random(Y.shape) < 0.1] = np.nan
    prep = P.prepare_on_device(Y, G)[0]
    try:
        assert prep.p == p
        rm = np.zeros(p, dtype=bool)
        lh = H.prepare_list_hyper_(None, prep.Y, p, (5, 25), rm)
        li = H.prepare_list_init_(None, prep.Y, p, (5, 25), rm, q, 456)
        run = VbRun(prep.Y, prep, lh, li, None, 0.1, 6, True, True)
        try:
            run.run()
            fit = run.fitted(prep)
            beta = run.result()["beta_vb"]
            Xs = prep.X_host()
            want, bound = PU.yardstick(Xs, 0.0, 1.0, beta)
            assert fit.shape == (n, q)
            PU.assert_within(fit, want, bound, f"fitted na={na}")
            assert run.fitted(prep).tobytes() == fit.tobytes()
            # the host matrix the run could have been given instead goes through aq_vb_predict: the same kernels, the same bits
            assert run.fitted(Xs).tobytes() == fit.tobytes()
            if not na:
                Yc = prep.Y
                scale = np.sqrt((Yc ** 2).sum(0) / n)
                drift = float(np.max(np.abs((Yc - run.residual()) - fit) / scale[None, :]))
                print(f"|(Yc - residual) - X_beta_vb| / rms = {drift:.3g}")
                assert drift < 1e-10
        finally:
            run.close()
    finally:
        prep.close()


# ---- atlasqtl(predict=, fitted=, keep_predictor=) and predict() ----
N_API, P_API, Q_API = 60, 40, 20
CST, DUP, LDC = 3, 10, 20            # a constant column, a copy of column 5, and column 19 with one genotype changed


@functools.lru_cache(maxsize=None)
def _api_data():
    G = np.array(PU.dosages(N_API, P_API, seed=21))
    G[:, CST] = 1
    G[:, DUP] = G[:, 5]
    G[:, LDC] = G[:, LDC - 1]
    G[20, LDC] = (G[20, LDC] + 1) % 3
    G = np.asfortranarray(G)
    rng = np.random.default_rng(22)
    Y = G[:, [0, 7, 30]].astype(np.float64) @ rng.normal(size=(3, Q_API)) + rng.normal(size=(N_API, Q_API))
    Xn = np.asfortranarray(rng.binomial(2, 0.3, size=(37, P_API)).astype(np.int8))
    for a in (G, Y, Xn):
        a.setflags(write=False)
    return G, Y, Xn


def _fit(**kw):
    import atlasqtl_amd as A
    G, Y, _ = _api_data()
    return A.atlasqtl(Y, G, p0=(2, 4), anneal=None, maxit=6, user_seed=3, verbose=0, ld_prune={"r2": 0.8, "window": 10}, **kw)


@functools.lru_cache(maxsize=None)
def _dense():
    return _fit(predict=_api_data()[2], fitted=True, keep_predictor=True)


def _clean_env(monkeypatch):
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)


def test_predict_argument_of_a_dense_run(monkeypatch):
    import atlasqtl_amd as A
    _clean_env(monkeypatch)
    G, Y, Xn = _api_data()
    res = _dense()
    kept = np.array([j for j in range(P_API) if j not in (CST, DUP, LDC)])
    pr = res["predictor"]
    assert set(pr) == {"kept_x", "x_center", "x_scale", "p_given"} and pr["p_given"] == P_API
    np.testing.assert_array_equal(pr["kept_x"], kept)
    assert res["names_x"] == [f"Cov_x_{j + 1}" for j in kept] and res["beta_vb"].shape == (kept.size, Q_API)
    Gk = G[:, kept].astype(np.float64)
    np.testing.assert_allclose(pr["x_center"], Gk.mean(0), rtol=1e-13)
    np.testing.assert_allclose(pr["x_scale"], Gk.std(0, ddof=1), rtol=1e-13)
    want, bound = PU.yardstick(Xn[:, kept], pr["x_center"], pr["x_scale"], res["beta_vb"])
    assert res["predicted"].shape == (37, Q_API) and np.abs(res["beta_vb"]).max() > 0
    PU.assert_within(res["predicted"], want, bound, "atlasqtl(predict=)")
    # the matrix-level twin on the dense result, int8 and fp64
    later = A.predict(res, Xn)
    PU.assert_within(later, want, bound, "predict(res, X_new)")
    assert A.predict(res, Xn.astype(np.float64)).tobytes() == later.tobytes()
    # X_beta_vb on the prepared X against the dense result applied to the X of the fit, within the same bound
    _, bound_g = PU.yardstick(G[:, kept], pr["x_center"], pr["x_scale"], res["beta_vb"])
    assert res["X_beta_vb"].shape == (N_API, Q_API)
    assert np.all(np.abs(res["X_beta_vb"] - A.predict(res, G)) <= bound_g.astype(np.float64))
    # ... and X_beta_vb against the yardstick on the prepared matrix itself, which the same preparation gives again
    from atlasqtl_amd import prepare as P
    prep = P.prepare_on_device(Y, G, ld_prune={"r2": 0.8, "window": 10})[0]
    try:
        assert prep.p == kept.size
        want_x, bound_x = PU.yardstick(prep.X_host(), 0.0, 1.0, res["beta_vb"])
    finally:
        prep.close()
    PU.assert_within(res["X_beta_vb"], want_x, bound_x, "atlasqtl(fitted=True)")


def test_a_sparse_run_predicts_the_same_bits(monkeypatch):
    import atlasqtl_amd as A
    _clean_env(monkeypatch)
    _, _, Xn = _api_data()
    dense = _dense()
    sparse = _fit(predict=Xn, fitted=True, sparse_output={"thres": 0.5})
    assert "beta_vb" not in sparse and "gam_vb" not in sparse and "predictor" not in sparse and "assoc" in sparse
    assert sparse["predicted"].tobytes() == dense["predicted"].tobytes()
    assert sparse["X_beta_vb"].tobytes() == dense["X_beta_vb"].tobytes()
    want, bound = PU.yardstick(Xn[:, dense["predictor"]["kept_x"]], dense["predictor"]["x_center"], dense["predictor"]["x_scale"],
                               dense["beta_vb"])
    PU.assert_within(sparse["predicted"], want, bound, "sparse run")
    assert np.all(np.abs(sparse["predicted"] - A.predict(dense, Xn)) <= bound.astype(np.float64))
    with pytest.raises(A.AtlasqtlError, match="sparse result"):
        A.predict(sparse, Xn)


def test_removed_columns_of_x_new_do_not_matter(monkeypatch):
    import atlasqtl_amd as A
    _clean_env(monkeypatch)
    _, _, Xn = _api_data()
    dense = _dense()
    X2 = np.array(Xn)
    for j in (CST, DUP, LDC):
        X2[:, j] = (X2[:, j] + 1 + np.arange(37)) % 3
    assert (X2 != Xn).any()
    assert A.predict(dense, X2).tobytes() == A.predict(dense, Xn).tobytes()
    again = _fit(predict=X2)
    assert again["predicted"].tobytes() == dense["predicted"].tobytes()
    assert "X_beta_vb" not in again and "predictor" not in again
    X3 = np.array(Xn)
    X3[:, 7] = (X3[:, 7] + 1) % 3                          # a kept column does matter
    assert A.predict(dense, X3).tobytes() != A.predict(dense, Xn).tobytes()


def test_no_new_key_unless_asked(monkeypatch):
    _clean_env(monkeypatch)
    plain = _fit()
    assert not {"predicted", "X_beta_vb", "predictor"} & set(plain)
    assert plain["beta_vb"].tobytes() == _dense()["beta_vb"].tobytes()
    only = _fit(keep_predictor=True)
    assert "predictor" in only and not {"predicted", "X_beta_vb"} & set(only)


def test_add_collinear_back_results_are_refused(monkeypatch):
    import atlasqtl_amd as A
    _clean_env(monkeypatch)
    G, Y, Xn = _api_data()
    res = A.atlasqtl(Y, G, p0=(2, 4), anneal=None, maxit=3, user_seed=3, verbose=0, add_collinear_back=True, keep_predictor=True)
    assert "names_x_all" in res and res["beta_vb"].shape[0] == len(res["predictor"]["kept_x"]) + 1
    with pytest.raises(A.AtlasqtlError, match="add_collinear_back=True"):
        A.predict(res, Xn)
