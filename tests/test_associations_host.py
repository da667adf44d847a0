"""The sparse table of associations (summary.atlasqtl's gam_vb > thres / assign_bFDR(gam_vb) < thres,
R/summarise_output.R:99-106): the parts that need no GPU -- argument errors of the C entries, the collinear add-back on
tables, and the host merge of the trait shards' tables."""
import ctypes as C

import numpy as np
import pytest

from atlasqtl_amd import _lib


def reference_table(gam, beta, thres, fdr):
    """The table the dense matrices imply, on the oracle's assign_bFDR: rows in the order of
    order(as.vector(gam_vb), decreasing = TRUE), restricted to the selected set."""
    from oracle.atlasqtl_oracle import assign_bFDR
    p = gam.shape[0]
    v = gam.reshape(-1, order="F")
    ind = np.argsort(-v, kind="stable")
    f = assign_bFDR(gam).reshape(-1, order="F")
    keep = (f < thres) if fdr else (v > thres)
    rows = ind[keep[ind]]
    return dict(snp=(rows % p).astype(np.int32), trait=(rows // p).astype(np.int32), ppi=v[rows],
                beta=beta.reshape(-1, order="F")[rows], fdr=f[rows], n_pairs=int(rows.size))


def assert_tables_equal(got, ref, fdr_exact=True):
    assert got["n_pairs"] == ref["n_pairs"]
    np.testing.assert_array_equal(got["snp"], ref["snp"])
    np.testing.assert_array_equal(got["trait"], ref["trait"])
    np.testing.assert_array_equal(got["ppi"], ref["ppi"])
    np.testing.assert_array_equal(got["beta"], ref["beta"])
    if fdr_exact:
        np.testing.assert_array_equal(got["fdr"], ref["fdr"])
    else:
        np.testing.assert_allclose(got["fdr"], ref["fdr"], rtol=1e-9, atol=1e-15)


def _matrix(p=60, q=50, seed=11):
    rng = np.random.default_rng(seed)
    gam = rng.beta(0.05, 1.0, size=(p, q))
    gam[rng.random((p, q)) < 0.05] = 0.97          # a tie block that spans the shards
    return gam, rng.standard_normal((p, q)) * gam


def test_argument_errors_come_before_any_device_call(hiplib):
    m = np.asfortranarray(np.full((3, 2), 0.7))
    n = C.c_int64(-5)
    nul_i, nul_d = C.cast(None, _lib.ip), C.cast(None, _lib.dp)
    outs = (nul_i, nul_i, nul_d, nul_d, nul_d)
    ARG = 1
    op = lambda mat, thres, cap, np_: hiplib.aq_select_pairs(mat, nul_d, 3, 2, thres, 0, cap, *outs, np_, 0)
    assert op(nul_d, 0.5, 0, C.byref(n)) == ARG
    assert op(_lib.as_dp(m), float("nan"), 0, C.byref(n)) == ARG
    assert op(_lib.as_dp(m), 0.5, -1, C.byref(n)) == ARG
    assert op(_lib.as_dp(m), 0.5, 0, None) == ARG
    assert b"aq_select_pairs" in hiplib.aq_last_error()
    # the handle is not looked at before the arguments are: any non-NULL value stands in for one here
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    vb = lambda h, thres, cap, np_: hiplib.aq_vb_select_pairs(h, thres, 0, cap, *outs, np_)
    assert vb(None, 0.5, 0, C.byref(n)) == ARG
    assert vb(fake, float("nan"), 0, C.byref(n)) == ARG
    assert vb(fake, 0.5, -1, C.byref(n)) == ARG
    assert vb(fake, 0.5, 0, None) == ARG
    assert b"aq_vb_select_pairs" in hiplib.aq_last_error()
    assert hiplib.aq_vb_bfdr_pairs(None, 0, 0, 0, nul_i, nul_i, nul_d, nul_d) == ARG
    assert n.value == -5


def test_valid_call_fails_loudly_without_device(hiplib):
    if hiplib.aq_device_count() > 0:
        pytest.skip("a HIP device is visible here")
    import atlasqtl_amd as A
    gam, beta = _matrix(7, 3)
    with pytest.raises(_lib.AtlasqtlHipError, match="no HIP device"):
        A.associations(gam, beta, 0.5)


def test_collinear_add_back_on_the_table_equals_the_dense_add_back():
    """Two duplicate groups, one of them with two copies: the expanded table is the reference table of the dense
    add_collinear_back_ output."""
    from atlasqtl_amd.api import add_collinear_back_, add_collinear_back_pairs_
    gam, beta = _matrix(9, 6, seed=3)
    gam[2, 1] = gam[5, 1] = 0.97                   # ties between a duplicated and another row
    theta = np.arange(9.0)
    names_x = [f"x{j}" for j in range(9)]
    initial = ["x0", "d2a", "x1", "x2", "x3", "d6", "x4", "x5", "d2b", "x6", "x7", "x8"]
    rmvd = {"d2a": "x2", "d2b": "x2", "d6": "x6"}
    for thres in (0.5, 0.01, -1.0):
        tab = reference_table(gam, beta, thres, False)
        rs = (gam > thres).sum(1)
        beta_d, gam_d, theta_d = add_collinear_back_(beta, gam, theta, initial, rmvd, names_x)
        ref = reference_table(gam_d, beta_d, thres, False)
        got, rs_x, theta_x = add_collinear_back_pairs_(tab, rs, theta, initial, rmvd, names_x)
        assert ref["n_pairs"] > tab["n_pairs"] > 0
        assert_tables_equal(got, ref)
        np.testing.assert_array_equal(rs_x, (gam_d > thres).sum(1))
        np.testing.assert_array_equal(theta_x, theta_d)
        cut, _, _ = add_collinear_back_pairs_(tab, rs, theta, initial, rmvd, names_x, max_pairs=5)
        assert cut["n_pairs"] == ref["n_pairs"]
        assert_tables_equal(cut, {k: (v if k == "n_pairs" else v[:5]) for k, v in ref.items()})


def test_collinear_add_back_with_sparse_fdr_mode_is_refused_before_any_gpu_work():
    import atlasqtl_amd as A
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((30, 8)), rng.standard_normal((30, 4))
    with pytest.raises(ValueError, match="FDR"):
        A.atlasqtl(Y, X, (2, 4), verbose=0, add_collinear_back=True, sparse_output={"fdr_adjust": True})
    with pytest.raises(ValueError, match="sparse_output"):
        A.atlasqtl_global_local_core_(Y, X, 4, None, 1, 0.1, 5, 0, {}, {}, sparse_output={"threshold": 0.5})


@pytest.mark.parametrize("fdr,thres", [(False, 0.5), (False, 0.9), (False, 0.97), (True, 0.02), (True, 0.05), (True, 0.2),
                                       (True, 0.6)])
def test_merged_shard_tables_are_the_table_of_the_whole_matrix(fdr, thres):
    """What the sharded path does on the host: the shards' own rows (local order, global trait index) merged by
    (-ppi, global position), FDR as the running mean along the merged prefix -- equal to assign_bFDR there, both being
    sequential sums in the same order."""
    from atlasqtl_amd.core import merge_pair_tables
    gam, beta = _matrix()
    p = gam.shape[0]
    ref = reference_table(gam, beta, thres, fdr)
    assert 0 < ref["n_pairs"] < gam.size
    cuts = [0, 16, 32, 50]
    tables = []
    for k0, k1 in zip(cuts[:-1], cuts[1:]):
        mine = (ref["trait"] >= k0) & (ref["trait"] < k1)         # this shard's rows of the global set ...
        t = {k: ref[k][mine] for k in ("snp", "trait", "ppi", "beta")}
        o = np.lexsort((t["snp"] + p * (t["trait"] - k0), -t["ppi"]))   # ... in the shard's own table order
        tables.append({k: v[o] for k, v in t.items()})
    assert sum(len(t["snp"]) > 0 for t in tables) > 1
    assert_tables_equal(merge_pair_tables(tables, p), ref)
    cut = merge_pair_tables([{k: v[:7] for k, v in t.items()} for t in tables], p, max_pairs=7, n_pairs=ref["n_pairs"])
    assert_tables_equal(cut, {k: (v if k == "n_pairs" else v[:7]) for k, v in ref.items()})
