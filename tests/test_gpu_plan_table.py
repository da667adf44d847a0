"""GPU: live handles against the planner's device-free entry and against tests/golden/plan_table_parent.json.

tests/test_plan_host.py replays the table through aq_plan_query; this file closes the loop through aq_vb_create: for a sample
of the table's rows a handle is created (no sweep) for a problem with the row's sizes and missingness counts under the row's
hooks.  What the handle reports (aq_vb_get_status, aq_vb_get_overrides, or the refusal) must be what aq_plan_query gives for this
device's CU count and memory -- the scan of Y, the device queries and the environment lookup of aq_vb_create feed the planner
what the arguments of aq_plan_query say -- and, where that is the row's plan, the row's overrides string."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(n, p, q, mm, ms):
    """Trait 0 misses mm samples; if the longest short list is not its own, trait 1 misses ms."""
    rng = np.random.default_rng(n + 3 * q + p)
    X = np.asfortranarray(rng.normal(size=(n, p)))
    Y = np.asfortranarray(rng.normal(size=(n, q)))
    Y[:mm, 0] = np.nan
    if ms != min(mm, n - mm):
        Y[n - ms:, 1] = np.nan
    miss = np.isnan(Y).sum(axis=0)
    assert int(miss.max()) == mm and int(np.minimum(miss, n - miss).max()) == ms
    lh = dict(A2_inv=1.0, m0=0.0, nu=1.0, rho=1.0, t02=0.1, eta=np.ones(q), kappa=np.ones(q), n0=-np.ones(q))
    li = dict(gam_vb=np.full((p, q), 0.05, order="F"), mu_beta_vb=np.full((p, q), 0.01, order="F"), sig02_inv_vb=1.0,
              sig2_beta_vb=np.full(q, 0.1), sig2_theta_vb=np.full(p, 0.1), tau_vb=np.ones(q), theta_vb=np.zeros(p), zeta_vb=-np.ones(q))
    return X, Y, lh, li


def test_live_handles_match_plan_query_and_the_table(hiplib, monkeypatch):
    import torch
    from atlasqtl_amd import _lib
    from atlasqtl_amd.core import PLAN_KEYS, VbRun
    with open(os.path.join(ROOT, "tests", "golden", "plan_table_parent.json")) as f:
        doc = json.load(f)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    total = torch.cuda.mem_get_info(0)[1]
    for k in [k for k in os.environ if k.startswith("AQ_") and k != "AQ_LIB"]:
        monkeypatch.delenv(k)
    rows = [r for r in doc["rows"] if r["n"] * r["q"] <= 250000 and (r["max_short_list"] == min(r["max_missing"], r["n"] - r["max_missing"]) or r["q"] >= 2)]
    assert len(rows) >= 200
    same_plan = refused = 0
    for r in rows:
        X, Y, lh, li = _problem(r["n"], r["p"], r["q"], r["max_missing"], r["max_short_list"])
        ov = " ".join(f"{k}={v}" for k, v in r["env"].items())
        st = _lib.AqVbStatus()
        rc = hiplib.aq_plan_query(r["n"], r["p"], r["q"], r["max_missing"], r["max_short_list"], ncu, total, ov.encode() or None, C.byref(st))
        want = {k: getattr(st, k) for k in PLAN_KEYS} if rc == 0 else hiplib.aq_last_error().decode()
        with monkeypatch.context() as m:
            for k, v in r["env"].items():
                m.setenv(k, v)
            try:
                run = VbRun(Y, X, lh, li, (1, 2, 10), 0.1, 12, True, True)
            except _lib.AtlasqtlHipError as e:
                got_rc, got = re.match(r"aq_vb_create: \[(-?\d+)\] (.*)$", str(e), flags=re.S).groups()
                assert (int(got_rc), got) == (rc, want), r
                refused += 1
                continue
            try:
                live = run.status()
            finally:
                run.close()
        assert rc == 0 and {k: live[k] for k in PLAN_KEYS} == want, (r, live, rc, want)
        assert set(live["overrides"].split()) <= set(ov.split()), (r, live["overrides"])
        if want == r["plan"]:
            assert live["overrides"] == r["overrides"], (r, live["overrides"])
            same_plan += 1
    print(f"\nrows {len(rows)} refused {refused} with the table's plan {same_plan} (device: {ncu} CUs, {total} bytes; table: {doc['ncu']}, {doc['total_bytes']})")
    assert refused >= 3
    if (ncu, total) == (doc["ncu"], doc["total_bytes"]):
        assert same_plan + refused == len(rows)
