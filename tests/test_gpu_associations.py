"""GPU: the sparse table of associations (aq_select_pairs / aq_vb_select_pairs / aq_vb_bfdr_pairs,
VbRun.associations, atlasqtl(..., sparse_output=...)) against the table the dense matrices imply
(R/summarise_output.R:99-106 on the oracle's assign_bFDR)."""
import numpy as np
import pytest

from tests.test_associations_host import assert_tables_equal, reference_table

pytestmark = pytest.mark.gpu

PPI_THRES, FDR_THRES = (0.5, 0.9), (0.05, 0.2)
TIE_FDR_THRES = (0.002, 0.02, 0.05, 0.2, 0.6)


def _bfdr_matrix(shape):
    """The inputs of test_assign_bfdr_matches_oracle."""
    rng = np.random.default_rng(5)
    m = rng.beta(0.05, 1.0, size=shape)
    m[rng.random(shape) < 0.1] = 1e-3
    if m.size > 5:
        m.flat[:3] = 1.0
    return m


def _assert_fdr_margin(gam, thresholds):
    """The exact set comparison in FDR mode is honest only if no oracle FDR value lies within ten summation bounds
    (relative 1e-8) of a threshold."""
    from oracle.atlasqtl_oracle import assign_bFDR
    f = assign_bFDR(gam)
    for t in thresholds:
        assert np.min(np.abs(f - t)) > 1e-8 * t, (t, np.min(np.abs(f - t)))


def _check_operator(gam, beta, thres, fdr):
    import atlasqtl_amd as A
    ref = reference_table(gam, beta, thres, fdr)
    got = A.associations(gam, beta, thres, fdr)
    print(f"shape {gam.shape} thres {thres} fdr {fdr}: {ref['n_pairs']} of {gam.size} selected, device {got['n_pairs']}")
    assert_tables_equal(got, ref, fdr_exact=False)
    nobeta = A.associations(gam, None, thres, fdr)
    assert "beta" not in nobeta
    np.testing.assert_array_equal(nobeta["snp"], ref["snp"])
    np.testing.assert_array_equal(nobeta["trait"], ref["trait"])
    return ref["n_pairs"]


@pytest.mark.parametrize("idx64", [False, True])
@pytest.mark.parametrize("fdr", [False, True])
def test_operator_on_host_matrices_matches_the_reference_table(fdr, idx64, monkeypatch):
    if idx64:
        monkeypatch.setenv("AQ_BFDR_IDX64", "1")
    thresholds = FDR_THRES if fdr else PPI_THRES
    selected = []
    for shape in [(1, 1), (7, 3), (130, 49), (2000, 300)]:
        gam = _bfdr_matrix(shape)
        beta = gam * np.random.default_rng(6).standard_normal(shape)
        if fdr:
            _assert_fdr_margin(gam, thresholds)
        for thres in thresholds:
            n = _check_operator(gam, beta, thres, fdr)
            if shape != (1, 1):
                assert 0 < n < gam.size
            selected.append(n)
    assert sum(selected) > 0


@pytest.mark.parametrize("idx64", [False, True])
@pytest.mark.parametrize("ties", [False, True])
def test_operator_fdr_cut_inside_tie_blocks(ties, idx64, monkeypatch):
    from tests.test_gpu_postproc import _fdr_problem
    if idx64:
        monkeypatch.setenv("AQ_BFDR_IDX64", "1")
    _, gam, _ = _fdr_problem(ties)
    beta = gam * np.random.default_rng(6).standard_normal(gam.shape)
    _assert_fdr_margin(gam, TIE_FDR_THRES)
    selected = [_check_operator(gam, beta, thres, True) for thres in TIE_FDR_THRES]
    assert all(0 < n < gam.size for t, n in zip(TIE_FDR_THRES, selected) if ties or t != 0.002)
    assert sum(selected) > 0
    if ties:   # a PPI exactly equal to the threshold stays out (0.5 occurs in this matrix)
        assert np.any(gam == 0.5)
        n = _check_operator(gam, beta, 0.5, False)
        assert n == int((gam > 0.5).sum()) > 0


def _converged_run(na_frac=0.0):
    from atlasqtl_amd.core import VbRun
    from tests.util import make_problem
    prob = make_problem(200, 130, 49, p_act=10, prob_assoc=0.3, na_frac=na_frac)
    return VbRun(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], (1, 2, 10), 0.1, 400, True, True).run()


def test_padding_rows_and_traits_are_never_selected():
    """p = 130 pads to 144 rows per tile, q = 49 leaves 15 padding traits in the last tile: with a threshold below every
    PPI the table has exactly p q rows, each (j, k) once."""
    run = _converged_run()
    tab = run.associations(-1.0, False)
    dense = run.result()
    run.close()
    p, q = 130, 49
    assert tab["n_pairs"] == p * q == len(tab["snp"])
    assert tab["snp"].min() == 0 and tab["snp"].max() == p - 1 and tab["trait"].min() == 0 and tab["trait"].max() == q - 1
    assert np.unique(tab["snp"].astype(np.int64) + p * tab["trait"]).size == p * q
    assert_tables_equal(tab, reference_table(dense["gam_vb"], dense["beta_vb"], -1.0, False), fdr_exact=False)


@pytest.mark.parametrize("na_frac", [0.0, 0.05])
@pytest.mark.parametrize("fdr", [False, True])
def test_resident_handle_matches_the_table_of_its_dense_result(fdr, na_frac):
    run = _converged_run(na_frac)
    thres = 0.05 if fdr else 0.5
    dense = run.result()
    tab = run.associations(thres, fdr)
    rs, nb = run.hotspot_sizes(thres, fdr)
    first = run.associations(thres, fdr, max_pairs=5)
    none = run.associations(thres, fdr, max_pairs=0)
    run.close()
    ref = reference_table(dense["gam_vb"], dense["beta_vb"], thres, fdr)
    if fdr:
        _assert_fdr_margin(dense["gam_vb"], [thres])
    print(f"na {na_frac} fdr {fdr}: {tab['n_pairs']} pairs")
    assert_tables_equal(tab, ref, fdr_exact=False)
    assert tab["n_pairs"] == nb > 5
    np.testing.assert_array_equal(np.bincount(tab["snp"], minlength=130), rs)
    # max_pairs below the count: the first rows of the full table, n_pairs still the full count; cap = 0 counts only
    assert_tables_equal(first, {k: (v if k == "n_pairs" else v[:5]) for k, v in ref.items()}, fdr_exact=False)
    assert none["n_pairs"] == nb and len(none["snp"]) == 0


def test_count_only_call_of_the_c_entry_agrees():
    import ctypes as C
    from atlasqtl_amd import _lib
    run = _converged_run()
    nul_i, nul_d = C.cast(None, _lib.ip), C.cast(None, _lib.dp)
    for thres, fdr in ((0.5, 0), (0.05, 1)):
        n = C.c_int64(-1)
        assert _lib.lib().aq_vb_select_pairs(run.h, thres, fdr, 0, nul_i, nul_i, nul_d, nul_d, nul_d, C.byref(n)) == 0
        assert n.value == run.hotspot_sizes(thres, bool(fdr))[1] > 0
        # only some of the arrays asked for
        snp = np.full(3, -1, dtype=np.int32)
        assert _lib.lib().aq_vb_select_pairs(run.h, thres, fdr, 3, _lib.as_ip(snp), nul_i, nul_d, nul_d, nul_d, C.byref(n)) == 0
        np.testing.assert_array_equal(snp, run.associations(thres, bool(fdr))["snp"][:3])
    run.close()


def _assoc_shard_worker(rank, world, port, outdir, ties):
    import os
    from tests.util import gloo_rank, shard_lists
    dist = gloo_rank(rank, world, port)
    from atlasqtl_amd.core import VbRun
    from tests.test_gpu_postproc import _fdr_problem
    prob, gam, cuts = _fdr_problem(ties)
    q = gam.shape[1]
    k0, k1 = cuts[rank], cuts[rank + 1]
    lh, li = shard_lists(prob["list_hyper"], prob["list_init"], k0, k1)
    li["gam_vb"] = np.asfortranarray(gam[:, k0:k1])
    run = VbRun(prob["Y"][:, k0:k1], prob["X"], lh, li, None, 0.1, 5, True, False, q_total=q, process_group=dist.group.WORLD,
                trait_offset=k0)
    run.run_sweeps(0)                       # the PPIs resident on the device are the crafted initial values
    out = {}
    for tag, thres, fdr in [(f"fdr_{t}", t, True) for t in TIE_FDR_THRES] + [("ppi_0.5", 0.5, False)]:
        for suffix, mp_ in (("", None), ("_cut", 4)):
            tab = run.associations(thres, fdr, max_pairs=mp_)
            for k, v in tab.items():
                out[f"{tag}{suffix}_{k}"] = v
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
    run.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("ties", [False, True])
def test_three_trait_shards_return_the_table_of_the_whole_matrix(ties, tmp_path):
    """Every rank returns the same whole-problem table: global trait indices, beta = the crafted gam_vb times the initial
    mu_beta_vb bit for bit (no sweep has run)."""
    from tests.test_gpu_postproc import _fdr_problem
    from tests.util import spawn_ranks
    spawn_ranks(_assoc_shard_worker, 3, str(tmp_path), ties)
    prob, gam, _ = _fdr_problem(ties)
    beta = gam * np.asarray(prob["list_init"]["mu_beta_vb"])
    _assert_fdr_margin(gam, TIE_FDR_THRES)
    res = [np.load(tmp_path / f"rank{r}.npz") for r in range(3)]
    some = 0
    for tag, thres, fdr in [(f"fdr_{t}", t, True) for t in TIE_FDR_THRES] + [("ppi_0.5", 0.5, False)]:
        ref = reference_table(gam, beta, thres, fdr)
        cut = {k: (v if k == "n_pairs" else v[:4]) for k, v in ref.items()}
        print(f"ties {ties} {tag}: {ref['n_pairs']} pairs")
        for r in res:
            for suffix, want in (("", ref), ("_cut", cut)):
                got = {k: r[f"{tag}{suffix}_{k}"] for k in ("snp", "trait", "ppi", "beta", "fdr")}
                got["n_pairs"] = int(r[f"{tag}{suffix}_n_pairs"])
                assert_tables_equal(got, want, fdr_exact=False)
        some += ref["n_pairs"]
    assert some > 0


def test_atlasqtl_sparse_output_equals_the_table_of_the_dense_call():
    """Same user_seed -> the same run (the sweep's reductions are fixed-order, as test_state_roundtrip_continues_bit_identically
    relies on): the sparse call's table is the reference table of the dense call's matrices, bit for bit."""
    import atlasqtl_amd as A
    from tests.test_gpu_api import _data
    X, Y, _ = _data(100, 75, 20, seed=123)
    dense = A.atlasqtl(Y=Y, X=X, p0=(5, 25), user_seed=1, verbose=0)
    assert set(dense) == {"beta_vb", "gam_vb", "theta_vb", "zeta_vb", "n", "p", "q", "anneal", "converged", "it", "maxit", "tol",
                          "lb_opt", "diff_lb", "p0", "rmvd_cst_x", "rmvd_coll_x", "names_x", "names_y"}
    for opts in ({}, {"thres": 0.05, "fdr_adjust": True}, {"thres": 0.5, "max_pairs": 3}):
        vb = A.atlasqtl(Y=Y, X=X, p0=(5, 25), user_seed=1, verbose=0, sparse_output=opts, full_output=True)
        assert not {"gam_vb", "beta_vb", "mu_beta_vb"} & set(vb)
        assert (vb.it, vb.converged, vb.lb_opt) == (dense.it, dense.converged, dense.lb_opt)
        np.testing.assert_array_equal(vb.theta_vb, dense.theta_vb)
        np.testing.assert_array_equal(vb.zeta_vb, dense.zeta_vb)
        assert vb.tau_vb.shape == (vb.q,) and vb.lam2_inv_vb.shape == (vb.p,)
        thres, fdr = opts.get("thres", 0.5), opts.get("fdr_adjust", False)
        ref = reference_table(dense.gam_vb, dense.beta_vb, thres, fdr)
        if fdr:
            _assert_fdr_margin(dense.gam_vb, [thres])
        assert ref["n_pairs"] > 3
        if "max_pairs" in opts:
            ref = {k: (v if k == "n_pairs" else v[:3]) for k, v in ref.items()}
        assert_tables_equal(vb.assoc, ref, fdr_exact=False)
        from oracle import atlasqtl_oracle as O
        rs_ref, nb_ref = O.hotspot_sizes(dense.gam_vb, thres, fdr)
        np.testing.assert_array_equal(vb.rs_thres, rs_ref)
        assert vb.nb_pairwise == nb_ref == vb.assoc["n_pairs"]
        assert list(vb.assoc["snp_name"]) == [vb.names_x[j] for j in vb.assoc["snp"]]
        assert list(vb.assoc["trait_name"]) == [vb.names_y[k] for k in vb.assoc["trait"]]


def test_atlasqtl_sparse_output_with_collinear_add_back():
    import atlasqtl_amd as A
    from tests.test_gpu_api import _data
    X, Y, _ = _data()
    X[:, 9] = X[:, 2]
    X[:, 20] = X[:, 2]
    X[:, 30] = X[:, 11]
    dense = A.atlasqtl(Y=Y, X=X, p0=(3, 9), user_seed=7, verbose=0, add_collinear_back=True)
    vb = A.atlasqtl(Y=Y, X=X, p0=(3, 9), user_seed=7, verbose=0, add_collinear_back=True, sparse_output={"thres": 0.3})
    assert dense.gam_vb.shape[0] == X.shape[1] and len(vb.rmvd_coll_x) == 3
    ref = reference_table(dense.gam_vb, dense.beta_vb, 0.3, False)
    assert ref["n_pairs"] > 0
    assert_tables_equal(vb.assoc, ref)
    np.testing.assert_array_equal(vb.rs_thres, (dense.gam_vb > 0.3).sum(1))
    np.testing.assert_array_equal(vb.theta_vb, dense.theta_vb)
    assert vb.nb_pairwise == ref["n_pairs"]


def test_expired_in_kernel_wait_is_reported_by_select_pairs(monkeypatch):
    import ctypes as C
    from atlasqtl_amd import _lib
    from atlasqtl_amd.core import VbRun
    from tests.util import make_problem
    prob = make_problem(300, 130, 49, p_act=8, prob_assoc=0.3)
    run = VbRun(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], (1, 2, 10), 0.1, 400, True, True)
    run.run_sweeps(3)
    assert run.associations(0.5)["n_pairs"] >= 0
    assert _lib.lib().aq_vb_debug_raise_errflag(run.h) == 0
    n = C.c_int64(0)
    nul_i, nul_d = C.cast(None, _lib.ip), C.cast(None, _lib.dp)
    assert _lib.lib().aq_vb_select_pairs(run.h, 0.5, 0, 0, nul_i, nul_i, nul_d, nul_d, nul_d, C.byref(n)) == 2
    with pytest.raises(_lib.AtlasqtlHipError, match=r"\[2\].*bounded wait"):
        run.associations(0.5)
    run.close()
