"""GPU: problems with more than 10 240 samples -- the look-ahead kernel's wide sample split (9 ... AQ_LA_CMAX parts per trait
group, split_exchange_wide) and, for Y with missing values, the per-trait Gram blocks of aq_k_gk_blocks_g -- against the
CPU oracle, which works in Gram space and so stays cheap at large n with small p."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_MAX = 48 * 108 * 16   # AQ_N_MAX, aq_core_sweep.h
C_MAX = 48      # AQ_LA_CMAX


def _problem(n, p=70, q=33, na=0.0, seed=123):
    from tests.util import make_problem
    return make_problem(n, p, q, p_act=8, prob_assoc=0.3, na_frac=na, seed=seed)


def _plan(prob):
    from atlasqtl_amd.core import VbRun
    run = VbRun(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], (1, 2, 10), 0.1, 1000)
    try:
        st = run.status()
        return st["core_kernel"], st["split_parts"]
    finally:
        run.close()


def _check(prob, scheme="global_local", df=1, anneal=(1, 2, 10)):
    """The parity checks of tests/test_gpu_sharded.py::_check_against_oracle, for either scheme and any df."""
    import atlasqtl_amd as A
    from oracle import atlasqtl_oracle as O
    q = prob["Y"].shape[1]
    tr = []
    ref = O.atlasqtl_global_local_core_(prob["Y"], prob["X"], q, anneal, df, 0.1, 1000, prob["list_hyper"], prob["list_init"],
                                        trace=tr, full_output=True, scheme=scheme)
    got = A.atlasqtl_global_local_core_(prob["Y"], prob["X"], q, anneal, df, 0.1, 1000, 0, prob["list_hyper"], prob["list_init"],
                                        full_output=True, debug=True, scheme=scheme)
    assert got["core_kernel"] == 0
    assert got["it"] == ref["it"]
    lref = np.array([r["lb"] for r in tr if r["lb"] is not None])
    np.testing.assert_allclose(got["elbo_trace"][1], lref, rtol=1e-9)
    np.testing.assert_allclose(got["mu_beta_vb"], ref["mu_beta_vb"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(got["gam_vb"], ref["gam_vb"], atol=1e-9)
    np.testing.assert_allclose(got["theta_vb"], ref["theta_vb"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(got["tau_vb"], ref["tau_vb"], rtol=1e-8)
    return got


@pytest.mark.parametrize("n", [10241, 12301, 20000, 50000])
def test_complete_y_large_n_matches_oracle(n):
    """Complete Y beyond 10 240 samples (ragged p and q), annealed: the wide split is planned and matches the oracle."""
    prob = _problem(n)
    kernel, parts = _plan(prob)
    assert kernel == 0 and 8 < parts <= C_MAX
    _check(prob)


@pytest.mark.parametrize("na", [0.05, 0.40])
def test_missing_values_large_n_matches_oracle(na):
    """Y with NA at n = 20 000: 5 % (lists of missing samples) and 40 % (more than 1024 missing per trait)."""
    prob = _problem(20000, na=na)
    kernel, parts = _plan(prob)
    assert kernel == 0 and parts > 8
    _check(prob)


def test_one_trait_mostly_missing_uses_observed_list():
    """One trait 97 % missing: its Gram blocks come from the list of its observed samples (the complement form)."""
    prob = _problem(20000, na=0.02)
    rng = np.random.default_rng(7)
    Y = prob["Y"].copy()
    Y[rng.random(Y.shape[0]) < 0.97, 5] = np.nan
    Y[:, 5] -= np.nanmean(Y[:, 5])
    prob["Y"] = Y
    _check(prob)


@pytest.mark.parametrize("C", [12, 24, C_MAX])
@pytest.mark.parametrize("na", [0.0, 0.08])
def test_forced_wide_split_moderate_n(C, na, monkeypatch):
    """AQ_LA_C = 9 ... AQ_LA_CMAX forces the many-part exchange at moderate n."""
    monkeypatch.setenv("AQ_LA_C", str(C))
    prob = _problem(4000, p=50, q=21, na=na)
    assert _plan(prob) == (0, C)
    _check(prob)


def test_global_scheme_large_n():
    _check(_problem(12301), scheme="global")


def test_df3_annealed_large_n():
    _check(_problem(12301), df=3)


def test_deterministic_and_resumable_large_n():
    """Two runs are bit-identical; get_state / set_state continues bit-identically; the residual is mis .* (Y - X beta)."""
    from atlasqtl_amd.core import VbRun
    prob = _problem(20000, na=0.05)

    def new():
        return VbRun(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], (1, 2, 10), 0.1, 1000)

    a, b = new(), new()
    try:
        a.run()
        b.run_sweeps(4)
        st = b.get_state()
        b.close()
        b = new().set_state(st)
        b.run()
        ra, rb = a.result(full_output=True), b.result(full_output=True)
        np.testing.assert_array_equal(ra["gam_vb"], rb["gam_vb"])
        np.testing.assert_array_equal(ra["mu_beta_vb"], rb["mu_beta_vb"])
        R = a.residual()
        mis = ~np.isnan(prob["Y"])
        ref = np.where(mis, np.nan_to_num(prob["Y"]) - prob["X"] @ ra["beta_vb"], 0.0)
        np.testing.assert_allclose(R, ref, atol=1e-9, rtol=0)
    finally:
        a.close()
        b.close()


AQ_ERR_ARG, AQ_ERR_UNSUPPORTED = 1, 3   # include/atlasqtl_hip.h


def _create_error(prob):
    """(code, message) of a failing aq_vb_create."""
    from atlasqtl_amd._lib import AtlasqtlHipError
    with pytest.raises(AtlasqtlHipError) as e:
        _plan(prob)
    msg = str(e.value)
    return int(msg.split("[", 1)[1].split("]", 1)[0]), msg


def test_n_beyond_limit_is_unsupported():
    code, msg = _create_error(_problem(N_MAX + 1, p=20, q=3))
    assert code == AQ_ERR_UNSUPPORTED and str(N_MAX) in msg


def test_gram_blocks_that_do_not_fit_fail_with_sharding_hint(monkeypatch):
    monkeypatch.setenv("AQ_GK_MAX_GB", "0.000001")
    code, msg = _create_error(_problem(12301, p=40, q=17, na=0.05))
    assert code == AQ_ERR_UNSUPPORTED and "shard the traits" in msg


@pytest.mark.parametrize("n,C", [(12301, 5), (12301, C_MAX + 1), (3000, C_MAX + 1)])
def test_forced_part_count_outside_the_wide_range_is_rejected(n, C, monkeypatch):
    """AQ_LA_C beyond AQ_LA_CMAX, or 2 ... 8 where only the wide split serves n: AQ_ERR_ARG, never a silent other plan."""
    monkeypatch.setenv("AQ_LA_C", str(C))
    code, msg = _create_error(_problem(n, p=20, q=5))
    assert code == AQ_ERR_ARG and "AQ_LA_C" in msg


def test_two_trait_shards_on_one_gpu_match_single_run():
    """aq_vb_run_multi with two trait shards on device 0 (host-staged all-reduce): each shard is a wide-split handle of its
    own, and the run equals the single-handle run."""
    import atlasqtl_amd as A
    from atlasqtl_amd.core import run_multi
    prob = _problem(20000, q=40, na=0.05)
    ref = A.atlasqtl_global_local_core_(prob["Y"], prob["X"], prob["q"], (1, 2, 10), 1, 0.1, 1000, 0, prob["list_hyper"],
                                        prob["list_init"], full_output=True, debug=True)
    got = run_multi(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], (1, 2, 10), 0.1, 1000, n_gpus=2,
                    devices=[0, 0], transport=1)
    assert got["it"] == ref["it"] and got["converged"] == ref["converged"]
    np.testing.assert_allclose(got["elbo_trace"][1], ref["elbo_trace"][1], rtol=1e-11)
    for k in ("gam_vb", "mu_beta_vb", "theta_vb", "zeta_vb", "tau_vb"):
        assert np.max(np.abs(got[k] - ref[k]) / np.maximum(np.abs(ref[k]), 1e-6)) < 1e-9, k


def test_atlasqtl_int8_dosages_end_to_end_large_n():
    """atlasqtl() on int8 dosages at n = 20 000: device prepare (column statistics, standardisation, centring of Y with NA)
    and the wide split, against the oracle path (NumPy prepare_data_, host hyper-parameters and init, oracle core)."""
    import atlasqtl_amd as A
    from atlasqtl_amd import hyper_init as H
    from atlasqtl_amd import synth
    from oracle import atlasqtl_oracle as O
    from oracle import prepare_oracle as PO
    d = synth.simulate(20000, 60, 19, p_act=6, seed=5, maf=0.25, prob_assoc=0.4, na_frac=0.03)
    G = d["X"].astype(np.int8)
    assert np.array_equal(G.astype(np.float64), d["X"])
    got = A.atlasqtl(Y=d["Y"], X=G, p0=(3, 9), user_seed=4, verbose=0, full_output=True)
    Xs, Yc, cst, coll = PO.prepare_xy(d["Y"], G.astype(np.float64))
    rm = cst.copy()
    rm[~cst] = coll
    q, p = Yc.shape[1], Xs.shape[1]
    lh = H.prepare_list_hyper_(None, Yc, p, (3, 9), rm)
    li = H.prepare_list_init_(None, Yc, p, (3, 9), rm, q, 4)
    tr = []
    ref = O.atlasqtl_global_local_core_(Yc, Xs, q, (1, 2, 10), 1, 0.1, 1000, lh, li, trace=tr, full_output=True)
    assert got["it"] == ref["it"]
    lref = np.array([r["lb"] for r in tr if r["lb"] is not None])
    np.testing.assert_allclose(got["elbo_trace"][1], lref, rtol=1e-9)
    np.testing.assert_allclose(got["mu_beta_vb"], ref["mu_beta_vb"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(got["gam_vb"], ref["gam_vb"], atol=1e-9)
