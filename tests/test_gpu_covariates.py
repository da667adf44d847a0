"""GPU: covariates regressed out of X and Y on the device (aq_prepare_data_cov / aq_prepare_data_bed_cov, the kernels of
atlasqtl_amd/csrc/aq_cov_kernels.h) against the long-double restatement of tests/cov_util.py, and whole runs of
atlasqtl(..., covariates=).  The bars are absolute (the residuals are no longer small integers, and entries near zero make
a per-entry relative error meaningless): 1e-12 on the standardised X, 1e-12 max|Y| on the residual Y -- the bars of
tests/test_gpu_prepare.py.  An fp64 restatement of the device algorithm is within 1e-14 of the truth on every shape here."""
import ctypes as C

import numpy as np
import pytest

from tests import bed_util
from tests import cov_util as CU
from tests.test_gpu_prepare import _case

pytestmark = pytest.mark.gpu

BINARY_COPY = 9        # the column of X set equal to the binary covariate (d >= 2): the covariates absorb it


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _prepared(Y, X, Z):
    """prepare_on_device(Y, X, covariates=Z) brought to the host."""
    from atlasqtl_amd.prepare import prepare_on_device
    prep, cst, coll, dup = prepare_on_device(Y, X, covariates=Z)
    try:
        return dict(cst=cst, coll=coll, dup=dup, Xs=prep.X_host(), Yc=prep.Y.copy(), p=prep.p, n_cov=prep.n_cov,
                    absorbed=prep.cov_absorbed, r2=prep.cov_r2)
    finally:
        prep.close()


def _assert_same_bits(a, b):
    for key in ("cst", "coll", "dup", "Xs", "Yc", "absorbed", "r2"):
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, key
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key


@pytest.mark.parametrize("n,p,q,d,na", [(50, 16, 3, 1, 0.0), (333, 100, 7, 5, 0.1), (1000, 257, 5, 20, 0.3), (200, 64, 4, 96, 0.2),
                                        (5000, 40, 2, 32, 0.05)])
def test_residuals_match_the_long_double_truth(n, p, q, d, na):
    G, Y = _case(n, p, q, seed=n + p, na=na)
    rng = np.random.default_rng(7 * n + d)
    Z = CU.covariates(n, d, rng)
    if d >= 2:
        G[:, BINARY_COPY] = Z[:, 1].astype(np.int8)
    if n == 333:
        Y[rng.random(n) < 0.9, 0] = np.nan                    # one trait with about 26 observed rows
        assert 6 < (~np.isnan(Y[:, 0])).sum() < 60
    ref = CU.truth(Y, G.astype(np.float64), Z)
    assert ref["absorbed"].sum() == (1 if d >= 2 else 0) and (d < 2 or ref["absorbed"][BINARY_COPY])
    y_bar = 1e-12 * np.nanmax(np.abs(Y))
    outs = []
    for X in (G.astype(np.float64), G):                       # fp64 and int8 dosage input
        got = _prepared(Y, X, Z)
        assert got["n_cov"] == d
        np.testing.assert_array_equal(got["cst"], ref["cst"])
        np.testing.assert_array_equal(got["coll"], ref["coll"])
        np.testing.assert_array_equal(got["absorbed"], ref["absorbed"])
        assert set(np.where(got["coll"])[0]) == {7, 11, p - 1}
        assert got["dup"][7] == 1 and got["dup"][11] == 1 and got["dup"][p - 1] == 4
        assert got["p"] == ref["Xs"].shape[1] == p - 5 - int(ref["absorbed"].sum())
        Xs = got["Xs"]
        err_x = np.abs(Xs - ref["Xs"]).max()
        err_y = np.nanmax(np.abs(got["Yc"] - ref["Yc"]))
        ortho = np.abs(ref["Q"].T @ Xs).max()
        sums = np.abs(np.nansum(got["Yc"], axis=0)).max()
        err_r2 = np.nanmax(np.abs(got["r2"] - ref["r2"]))
        print(f"n={n} d={d} {X.dtype}: |Xs - ref| {err_x:.2e}  |Y - ref| {err_y:.2e} (bar {y_bar:.2e})  |Q'Xs| {ortho:.2e} "
              f"(bar {1e-12 * np.sqrt(n):.2e})  |sum y| {sums:.2e}  |r2 - ref| {err_r2:.2e}")
        assert Xs.shape == ref["Xs"].shape and err_x <= 1e-12
        np.testing.assert_allclose((Xs ** 2).sum(0), n - 1.0, rtol=1e-12)
        assert ortho <= 1e-12 * np.sqrt(n)
        np.testing.assert_array_equal(np.isnan(got["Yc"]), np.isnan(Y))
        assert err_y <= y_bar
        assert sums <= 1e-12 * n
        np.testing.assert_array_equal(np.isnan(got["r2"]), np.isnan(ref["r2"]))
        assert err_r2 <= 1e-12
        outs.append(got)
    _assert_same_bits(outs[0], outs[1])                       # the two input types give the same bits


def test_plink_input_with_covariates(tmp_path):
    from atlasqtl_amd import PlinkBed
    n, p, q, d = 333, 100, 7, 5
    G, Y = _case(n, p, q, seed=11, na=0.1)
    rng = np.random.default_rng(12)
    Z = CU.covariates(n, d, rng)
    G[:, BINARY_COPY] = Z[:, 1].astype(np.int8)
    bed_util.write_fileset(tmp_path / "g", G, pad_rng=rng)
    want = _prepared(Y, G, Z)
    assert want["absorbed"][BINARY_COPY] and want["cst"][BINARY_COPY]
    _assert_same_bits(_prepared(Y, PlinkBed(tmp_path / "g"), Z), want)
    # missing calls, missing = "mean": the imputed fp64 matrix is what gets residualised
    Gm = G.astype(np.int64)
    Gm[rng.random(Gm.shape) < 0.03] = bed_util.NA
    bed_util.write_fileset(tmp_path / "m", Gm, pad_rng=rng)
    n_het, n_hom, n_obs = (Gm == 1).sum(0), (Gm == 2).sum(0), (Gm != bed_util.NA).sum(0)
    fill = np.float64(n_het + 2 * n_hom) / np.float64(n_obs)
    G_imp = np.where(Gm == bed_util.NA, fill[None, :], Gm.astype(np.float64))
    got = _prepared(Y, PlinkBed(tmp_path / "m", missing="mean"), Z)
    _assert_same_bits(got, _prepared(Y, G_imp, Z))


def test_collinear_on_the_observed_rows_is_an_error_and_leaks_nothing():
    from atlasqtl_amd import _lib
    from atlasqtl_amd.prepare import AtlasqtlError, prepare_on_device
    rng = np.random.default_rng(21)
    n = 100
    X = rng.binomial(2, 0.3, size=(n, 12)).astype(np.int8)
    live = _lib.lib().aq_debug_live_device_bytes
    # a batch indicator whose batch is entirely missing for trait 2: constant on the rows observed there
    Z = np.column_stack([rng.normal(size=n), (np.arange(n) < 30).astype(float)])
    Y = rng.normal(size=(n, 3))
    Y[:30, 1] = np.nan
    before = live()
    with pytest.raises(AtlasqtlError, match="collinear on the samples observed for column 2 of Y"):
        prepare_on_device(Y, X, covariates=Z)
    assert live() == before
    # a trait with no more observed rows than d + 1
    Z = rng.normal(size=(n, 10))
    Y = rng.normal(size=(n, 3))
    Y[11:, 1] = np.nan                                        # 11 observed = D; 11 % of the rows: the missingness guards pass
    with pytest.raises(AtlasqtlError, match="collinear on the samples observed for column 2 of Y"):
        prepare_on_device(Y, X.astype(np.float64), covariates=Z)
    assert live() == before
    Y[11, 1] = 0.5                                            # 12 observed > D: fine
    prep, *_ = prepare_on_device(Y, X, covariates=Z)
    prep.close()
    assert live() == before


@pytest.mark.parametrize("na", [0.0, 0.1])
def test_whole_run_equals_the_run_on_the_residuals(na):
    """atlasqtl(Y, X_int8, covariates=Z) against atlasqtl on the restatement's residuals, at the project's parity bars."""
    import atlasqtl_amd as A
    from atlasqtl_amd import synth
    n, p, q, d = 200, 130, 24, 3
    sim = synth.simulate(n, p, q, p_act=8, seed=5, maf=0.25, prob_assoc=0.4)
    rng = np.random.default_rng(31)
    Z = CU.covariates(n, d, rng)
    G = sim["X"].astype(np.int8)
    Y = sim["Y"] + ((Z - Z.mean(0)) / Z.std(0)) @ rng.normal(size=(d, q))
    if na > 0:
        Y[rng.random(Y.shape) < na] = np.nan
    Xr, absorbed, _ = CU.residualise_x(G.astype(np.float64), Z)
    assert not absorbed.any()
    kw = dict(p0=(3, 9), user_seed=4, verbose=0, full_output=True)
    a = A.atlasqtl(Y, G, covariates=Z, **kw)
    b = A.atlasqtl(CU.residualise_y(Y, Z), Xr, **kw)
    assert a.n_covariates == d and a.rmvd_cov_x is None and a.cov_r2_x.shape == (p,) and "n_covariates" not in b
    assert a.converged and b.converged and a.it == b.it
    assert abs(a.lb_opt - b.lb_opt) <= 1e-9 * abs(b.lb_opt)
    np.testing.assert_allclose(a.gam_vb, b.gam_vb, rtol=0, atol=1e-6)


def test_covariates_remove_a_confounded_hotspot():
    """A null SNP whose dosage follows a covariate that also drives every trait: without the covariates it is a hotspot of all
    30 traits; with them it is gone and the true hotspot keeps its 12 traits (CPU restatement on this seed: 30 / 0.04 / 0.99998)."""
    import atlasqtl_amd as A
    rng = np.random.default_rng(1)
    n, p, q = 200, 60, 30
    z = rng.normal(size=(n, 2))
    X = rng.binomial(2, 0.25, size=(n, p)).astype(float)
    X[:, 5] = rng.binomial(2, 1 / (1 + np.exp(-1.5 * z[:, 0])))
    Y = rng.normal(size=(n, q))
    Y += np.outer(z[:, 0], 1.5 * rng.normal(size=q))
    Y[:, :12] += np.outer(X[:, 20], 0.8 * np.where(rng.random(12) < 0.5, 1, -1))
    kw = dict(p0=(2, 4), user_seed=4, verbose=0)
    raw = A.atlasqtl(Y, X, **kw)
    assert (raw.gam_vb[5] > 0.5).sum() == 30
    adj = A.atlasqtl(Y, X, covariates=z, **kw)
    print(f"adjusted: max PPI of the confounded SNP {adj.gam_vb[5].max():.3g}, min PPI of the true hotspot {adj.gam_vb[20, :12].min():.6g}")
    assert adj.gam_vb[5].max() < 0.5 and adj.gam_vb[20, :12].min() > 0.99
    assert adj.n_covariates == 2 and adj.rmvd_cov_x is None and len(adj.cov_r2_x) == p
    assert np.argmax(adj.cov_r2_x) == 5                       # the covariates explain the confounded SNP best
    sp = A.atlasqtl(Y, X, covariates=z, sparse_output={"thres": 0.5}, **kw)
    assert sp.rs_thres[5] == 0 and sp.rs_thres[20] >= 12 and sp.n_covariates == 2


def test_absorbed_predictor_is_named_in_the_result():
    import atlasqtl_amd as A
    rng = np.random.default_rng(2)
    n, p, q = 120, 20, 6
    Z = CU.covariates(n, 3, rng)
    X = rng.binomial(2, 0.3, size=(n, p)).astype(np.int8)
    X[:, 4] = Z[:, 1].astype(np.int8)
    res = A.atlasqtl(rng.normal(size=(n, q)), X, p0=(2, 4), user_seed=1, verbose=0, covariates=Z)
    assert res.rmvd_cov_x == ["Cov_x_5"] and "Cov_x_5" in res.rmvd_cst_x and "Cov_x_5" not in res.names_x
    assert res.gam_vb.shape == (p - 1, q) and res.cov_r2_x[4] > 1 - 1e-10


def test_nothing_changes_without_covariates():
    from atlasqtl_amd import _lib
    from atlasqtl_amd.prepare import prepare_on_device
    G, Y = _case(333, 100, 7, seed=3, na=0.1)
    outs = []
    for kw in ({}, {"covariates": None}):
        prep, cst, coll, dup = prepare_on_device(Y, G, **kw)
        assert prep.n_cov == 0 and prep.cov_absorbed is None and prep.cov_r2 is None
        outs.append((cst, coll, dup, prep.X_host(), prep.Y.copy()))
        prep.close()
    # the C entry with cov = NULL and with d = 0 is aq_prepare_data
    L = _lib.lib()
    Yf, Gf = np.asfortranarray(Y), np.asfortranarray(G)
    for cov in (None, _lib.AqPrepCov(0, None)):
        pin = _lib.AqPrepInput()
        pin.n, pin.p, pin.q, pin.X, pin.X_i8, pin.Y, pin.device = 333, 100, 7, None, Gf.ctypes.data_as(C.POINTER(C.c_int8)), _lib.as_dp(Yf), 0
        h = C.c_void_p()
        _lib.check(L.aq_prepare_data_cov(C.byref(pin), None if cov is None else C.byref(cov), C.byref(h)), "aq_prepare_data_cov")
        pk, d = C.c_int32(0), C.c_int32(-1)
        _lib.check(L.aq_prep_info(h, C.byref(pk), None, None, None, None, None))
        _lib.check(L.aq_prep_cov_info(h, C.byref(d), None, None))
        assert d.value == 0
        Xs, Yc = np.empty((333, pk.value), order="F"), np.empty((333, 7), order="F")
        _lib.check(L.aq_prep_get(h, _lib.as_dp(Xs), _lib.as_dp(Yc)))
        L.aq_prep_destroy(h)
        outs.append((outs[0][0], outs[0][1], outs[0][2], Xs, Yc))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))
