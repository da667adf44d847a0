"""Who owns device memory: aq_debug_live_device_bytes() counts the bytes held by the library's own allocations, so a handle
or an entry that forgets a buffer shows up as a counter that does not come back.  Every handle case uses the smallest shape
at which the split, chained and masked plans all exist (tests/test_gpu_api.py uses it for the same plan families).  The
tests count bytes on the host and compare results; they provoke no fault."""
import functools
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAMILIES = [({}, False), ({}, True), ({"AQ_LA_C": "2"}, False), ({"AQ_LA_C": "2"}, True), ({"AQ_CHAIN": "4"}, False),
            ({"AQ_KERNEL": "3", "AQ_MIS_C": "3"}, True), ({"AQ_KERNEL": "2"}, True)]


@functools.lru_cache(maxsize=None)
def _problem(na):
    from tests.util import make_problem
    if na:
        return make_problem(300, 130, 49, p_act=8, prob_assoc=0.3, na_frac=0.04)
    return make_problem(300, 130, 49, p_act=8, prob_assoc=0.3)


def _live():
    from atlasqtl_amd._lib import lib
    gc.collect()      # handles that an earlier test dropped without close() are destroyed now, not between two readings
    return int(lib().aq_debug_live_device_bytes())


def _vbrun(prob, li=None):
    from atlasqtl_amd.core import VbRun
    return VbRun(prob["Y"], prob["X"], prob["list_hyper"], li if li is not None else prob["list_init"], None, 0.1, 400, True, True)


def _family_id(v):
    if isinstance(v, dict):
        return "-".join(f"{k}={x}" for k, x in v.items()) or "default"
    return "na" if v else "complete"


@pytest.mark.parametrize("env,na", FAMILIES, ids=_family_id)
def test_create_run_query_close_returns_every_byte(monkeypatch, env, na):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = _problem(na)
    before = _live()
    for _ in range(5):
        run = _vbrun(prob)
        assert _live() > before
        run.run_sweeps(3)
        st = run.status()
        assert st["it"] == 3 and st["core_kernel"] == (int(env["AQ_KERNEL"]) if "AQ_KERNEL" in env else 0)
        run.result()
        run.get_state()
        run.hotspot_sizes(fdr_adjust=True)
        run.associations()
        run.value_summary("gam_vb")      # which = 0 of aq_vb_order_stats
        assert _live() > before
        run.close()
        assert _live() == before


def test_failed_creates_hold_nothing(monkeypatch):
    from atlasqtl_amd._lib import AtlasqtlHipError
    prob = _problem(True)
    before = _live()
    li = dict(prob["list_init"])          # init_generate with init_gam_sd = 0: AQ_ERR_ARG after every buffer has been allocated
    li["gam_vb"] = li["mu_beta_vb"] = None
    li["device_seed"], li["device_gam_mean"], li["device_gam_sd"] = 7, 0.0, 0.0
    with pytest.raises(AtlasqtlHipError, match="init_gam_sd"):
        _vbrun(prob, li)
    assert _live() == before
    with monkeypatch.context() as m:      # the planner's budget error: the wide split has no fallback kernel
        m.setenv("AQ_GK_MAX_GB", "0.000001")
        m.setenv("AQ_LA_C", "9")
        with pytest.raises(AtlasqtlHipError, match="Gram blocks"):
            _vbrun(prob)
    assert _live() == before
    run = _vbrun(prob)                    # and the next create succeeds
    assert _live() > before
    run.run_sweeps(1)
    run.close()
    assert _live() == before


def test_free_standing_entries_return_every_byte():
    import atlasqtl_amd as A
    from atlasqtl_amd import _lib, core, prepare
    from tests.util import operator_inputs
    rng = np.random.default_rng(5)
    ppi = np.asfortranarray(rng.uniform(size=(130, 49)) ** 4)
    beta = np.asfortranarray(rng.normal(size=(130, 49)))
    before = _live()
    core.assign_bFDR(ppi)
    assert _live() == before
    for fdr in (False, True):
        core.hotspot_sizes(ppi, 0.5, fdr_adjust=fdr)
        core.associations(ppi, beta, 0.5, fdr_adjust=fdr)
        assert _live() == before
    core.value_summary(ppi)
    assert _live() == before
    a = operator_inputs(6, 2)
    A.coreDualLoop(a["cp_X"], a["cp_Y_X"], a["gam_vb"], a["log_Phi"], a["log_1mPhi"], a["log_sig2_inv_vb"], a["log_tau_vb"],
                   a["m1_beta"], a["cp_betaX_X"], a["mu_beta_vb"], a["sig2_beta_vb"], a["tau_vb"], a["shuffled_ind"], a["sample_q"])
    assert _live() == before
    b = operator_inputs(6, 2, mis=True)
    A.coreDualMisLoop(b["cp_X"], b["cp_X_rm"], b["cp_Y_X"], b["gam_vb"], b["log_Phi"], b["log_1mPhi"], b["log_sig2_inv_vb"],
                      b["log_tau_vb"], b["m1_beta"], b["cp_betaX_X"], b["mu_beta_vb"], b["sig2_beta_vb"], b["tau_vb"],
                      b["shuffled_ind"], b["sample_q"])
    assert _live() == before
    x = np.linspace(-3.0, 3.0, 100)
    out = np.empty_like(x)
    assert _lib.lib().aq_special_eval_device(3, _lib.as_dp(np.abs(x) + 0.5), _lib.as_dp(np.full_like(x, 2.0)), _lib.as_dp(out), x.size, 0) == 0
    assert _live() == before
    truth = _problem(False)["truth"]
    prep = prepare.prepare_on_device(truth["Y"], truth["X"])[0]   # aq_prepare_data ...
    assert _live() > before
    prep.close()                                                  # ... aq_prep_destroy
    assert _live() == before


def test_set_up_results_survive_the_early_frees():
    """The row panels XR and the staging buffers are released inside aq_vb_create as soon as the set-up kernels that read them
    have finished.  A release that came too early would let the second handle's allocations land on memory the first one's
    set-up still reads: two handles created one after the other must give the same bits."""
    prob = _problem(True)
    res = []
    for _ in range(2):
        run = _vbrun(prob)
        run.run_sweeps(3)
        res.append(run.result(full_output=True))
        run.close()
    assert set(res[0]) >= {"beta_vb", "gam_vb", "mu_beta_vb", "theta_vb", "zeta_vb", "tau_vb", "sig2_beta_vb"}
    for key in res[0]:
        np.testing.assert_array_equal(res[0][key], res[1][key], err_msg=key)
