"""CPU: the inputs of tests/test_gpu_regimes.py hold what they claim -- on the data, the planner and the oracle alone.

tests/util.make_regime_problem promises neighbouring SNPs in LD across block and segment borders, rare variants whose carriers
are all missing in a trait, traits whose scales span 1e8 inside one trait tile, and hyper-parameters distinct in every trait.
These are conditions on the inputs: they are asserted here for every distinct input the GPU file uses, so that an edit to the
builder or to the case table cannot quietly shrink what the GPU tests cover.  Also here: the planner gives every case the kernel
instance it is written for (aq_plan_query, no device), the oracle converges within the whole-run budget on every input, the
committed reference-side measurements admit every input, and a hyper-parameter vector shifted by one trait moves the oracle's
result by more than 1000 times the bars -- so the GPU cases can see a shifted index."""
import warnings

import numpy as np
import pytest

from tests import test_gpu_regimes as T
from tests.util import REGIME_BLOCK, block_borders, chain_borders, r2_pair, rare_columns

INPUTS = sorted(T.all_inputs().items(), key=str)
MEM = 288 * 10**9          # device memory of the planned cases: more than any of them needs


_iid = T.input_id


def _id(item):
    return _iid(item[0])


DATA = sorted({i[:4] for i, _ in INPUTS}, key=str)      # (shape, regime, na, hyper): what the data and the lists depend on
CHAINED = {i[:4] for i, e, x in T.CASES.values() if "AQ_CHAIN" in e}


@pytest.mark.parametrize("key", DATA, ids=[_iid(k + (None, 1, "")) for k in DATA])
def test_inputs_hold_what_they_claim(key):
    (n, p, q), regime, na, hyper = key
    prob = T.problem(key)
    X, Y = prob["X"], prob["Y"]
    assert prob["p"] == X.shape[1] == p == prob["p_drawn"], "prepare_xy removed a column: the block borders have moved"
    assert p % REGIME_BLOCK != 0 and q % REGIME_BLOCK != 0 and -(-p // REGIME_BLOCK) >= 6      # ragged last block and tile
    np.testing.assert_allclose((X ** 2).sum(0), n - 1.0, rtol=1e-12)
    if "ld" in regime:
        border = {c: r2_pair(X, c - 1, c) for c in block_borders(p)}
        assert sum(v >= 0.95 for v in border.values()) >= 3, border
        if key in CHAINED:
            seg = chain_borders(p, 3)
            assert seg == [48, 96] and all(border[c] >= 0.95 for c in seg), (seg, border)
        assert {47, 48} <= set(prob["active"].tolist()) and r2_pair(X, 47, 48) >= 0.9
        # between neighbours the Gram terms are of the size of the diagonal, which make_problem never reaches
        r2n = np.array([r2_pair(X, j - 1, j) for j in range(1, p)])
        assert np.sum(r2n >= 0.9) >= 10 and r2n.max() >= 0.98
    else:
        assert max(r2_pair(X, j - 1, j) for j in range(1, p)) < 0.2
    if "rare" in regime:
        G = prob["truth"]["X"]
        cols = rare_columns(p)
        assert cols == list(range(4, p, 5)) and 79 in cols and 79 % REGIME_BLOCK == REGIME_BLOCK - 1
        counts = {int((G[:, j] == 1).sum()) for j in cols}
        assert counts == {1, 2, 3} and all(np.all((G[:, j] == 0) | (G[:, j] == 1)) for j in cols)
        assert X[:, cols].max() > 0.55 * np.sqrt(n)              # one carrier: (1 - 1/n) / sqrt(1/n) standardised; three: / sqrt(3)
        assert np.abs(np.delete(X, cols, axis=1)).max() < 0.35 * np.sqrt(n)
    if na > 0:
        mis = np.isnan(Y)
        assert 0.05 <= mis.mean() <= 0.08
        xn = T.x_norm_sq(prob)
        if "rare" in regime:
            dropped = prob["dropped"]
            assert len(dropped) >= 3 and any(j == 79 for j, k in dropped)
            tiles = {k // REGIME_BLOCK for j, k in dropped}
            assert len(tiles) == min(len(dropped), -(-q // REGIME_BLOCK)) >= 3
            for j, k in dropped:
                assert np.all(mis[prob["carriers"][j], k]) and xn[j, k] < T.NO_CARRIER
            # (the random missingness also takes the only carrier of a singleton here and there: the same kind of entry)
            assert xn.min() < 2.0 and np.all(xn[xn >= T.NO_CARRIER] > 0.25 * n)
    if "scale" in regime:
        v = np.nanvar(Y, axis=0, ddof=1)
        t_last = REGIME_BLOCK * ((q - 1) // REGIME_BLOCK)
        for lo, hi in ((0, REGIME_BLOCK), (t_last, q)):
            assert v[lo:hi].max() / v[lo:hi].min() >= 1e6, (lo, hi)
        assert v.max() / v.min() >= 1e14
    lh, li = prob["list_hyper"], prob["list_init"]
    if hyper == "per_trait":
        from atlasqtl_amd import hyper_init as H
        auto = H.auto_set_hyper_(Y, p, (5, 25))
        for name, vec in (("eta", lh["eta"]), ("kappa", lh["kappa"]), ("n0", lh["n0"]), ("tau_vb", li["tau_vb"])):
            vec = np.asarray(vec)
            assert vec.shape == (q,) and np.unique(vec).size == q, f"{name} repeats a value"
        assert (lh["nu"], lh["rho"]) == (0.5, 3.0) and lh["t02"] == 2.5 * auto["t02"] and lh["A2_inv"] == 1.0
        assert (lh["nu"], lh["rho"]) != (auto["nu"], auto["rho"])
        v = np.nanvar(Y, axis=0, ddof=1)
        assert np.all(lh["kappa"] / v >= 0.2) and np.all(lh["kappa"] / v <= 5.0)        # kappa follows the trait's scale
        assert np.all(li["tau_vb"] * v >= 0.5) and np.all(li["tau_vb"] * v <= 2.0)
    else:
        for name in ("eta", "kappa", "n0"):
            assert np.unique(np.asarray(lh[name])).size == 1


@pytest.mark.parametrize("item", INPUTS, ids=[_id(i) for i in INPUTS])
def test_oracle_runs_every_input_and_converges_within_the_whole_run_budget(item):
    """Every sweep count of the GPU file: finite, monotone (debug = True raises otherwise), and the whole run converges in fewer
    than WHOLE_MAXIT sweeps."""
    inputs, sweeps_list = item
    assert set(sweeps_list) | {s for (i, s) in T.EXCLUDED_RUNS if i == _iid(inputs)} == set(T.SWEEPS) and len(sweeps_list) >= 3
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        for s in T.SWEEPS:
            ref, lref = T.run_oracle(inputs, s)
            for f in ("theta_vb", "zeta_vb", "mu_beta_vb", "gam_vb", "tau_vb", "lam2_inv_vb", "sig2_theta_vb"):
                assert np.all(np.isfinite(ref[f])), (s, f)
            if s == T.WHOLE:
                assert ref["converged"] and ref["it"] < T.WHOLE_MAXIT and lref.size >= 2
            else:
                assert ref["it"] == T.maxit_of(inputs, s)
            if s == T.ELBO:
                assert lref.size >= T.ELBO_EVALS
    if "scale" in inputs[1]:
        tau = T.run_oracle(inputs, T.WHOLE)[0]["tau_vb"]
        # (the automatic kappa = 1 of every trait bounds tau_vb = eta_vb / kappa_vb by about n / 2 whatever the trait's scale)
        assert tau.max() / tau.min() >= (1e14 if inputs[3] == "per_trait" else 1e9)


PER_TRAIT = [i for i, _ in INPUTS if i[3] == "per_trait"]


@pytest.mark.parametrize("inputs", PER_TRAIT, ids=[_iid(i) for i in PER_TRAIT])
def test_a_hyper_vector_shifted_by_one_trait_is_seen(inputs):
    """eta, kappa and n0 each rolled by one trait, on the oracle: tau_vb and zeta_vb move by more than 1000 times their bars
    (after one sweep tau_vb = eta_vb / kappa_vb already reads eta and kappa, after three zeta_vb has read n0)."""
    from oracle import atlasqtl_oracle as O
    shape, regime, na, hyper, anneal, df, scheme = inputs
    prob = T.problem(inputs)
    for s in (3, T.ELBO):
        ref, _ = T.run_oracle(inputs, s)
        for name, field in (("eta", "tau_vb"), ("kappa", "tau_vb"), ("n0", "zeta_vb")):
            lh = type(prob["list_hyper"])(prob["list_hyper"])
            lh[name] = np.roll(np.asarray(lh[name]), 1)
            alt = O.atlasqtl_global_local_core_(prob["Y"], prob["X"], shape[2], anneal, df, 0.1, T.maxit_of(inputs, s), lh,
                                                prob["list_init"], thinned_elbo_eval=False, debug=False, full_output=True, scheme=scheme)
            moved = float(np.max(np.abs(alt[field] - ref[field]) / np.maximum(np.abs(ref[field]), T.FLOOR[field])))
            assert moved > 1000.0 * T.CAP[field] >= 1000.0 * T.bar(s, field, inputs), (s, name, field, moved)


def _plan_of(inputs, env):
    from atlasqtl_amd.core import plan_query
    (n, p, q), regime, na = inputs[:3]
    prob = T.problem(inputs)
    m = np.isnan(prob["Y"]).sum(axis=0)
    return plan_query(n, p, q, max_missing=int(m.max()), max_short_list=int(np.minimum(m, n - m).max()), ncu=256, total_bytes=MEM,
                      overrides=dict(env))


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_planner_gives_every_case_its_instance(name):
    """What the GPU test proves from aq_vb_status, from the planner alone at 256 CUs."""
    inputs, env, expect = T.CASES[name]
    st = _plan_of(inputs, env)
    assert st["core_kernel"] == expect["core_kernel"], st
    if expect["core_kernel"] != 0:
        return
    got = {k: st[k] for k in ("instance_flags", "split_parts", "tiles_per_group", "chain_segments")}
    assert got == {k: expect[k] for k in got}, st
    if expect["split_parts"] > 1:
        assert (st["tiles_matrix"], st["tiles_matrix2"]) == expect["geom"], st
    assert st["n_pad"] >= inputs[0][0]


def test_case_table_covers_the_instances_of_the_issue():
    """Plain-data check of the case table: every regime, hyper form, kernel, launch form and scheme it is meant to hold."""
    cases = T.CASES
    planned = {name: _plan_of(i, e) for name, (i, e, x) in cases.items()}

    def forms(pred):
        return {(planned[nm]["instance_flags"], planned[nm]["split_parts"], planned[nm]["tiles_per_group"], e.get("AQ_LA_XHELPER"),
                 i[0][0]) for nm, (i, e, x) in cases.items() if planned[nm]["core_kernel"] == 0 and pred(i)}
    for regime in T.REGIME_SETS:
        for hyper in T.HYPERS:
            f = forms(lambda i: i[1] == regime and i[2] == 0.0 and i[3] == hyper and i[5] == 1 and i[6] == "global_local")
            assert {(0, 1, 1, None, 300), (0, 1, 2, None, 1000), (0, 1, 1, None, 1000), (T.SEG, 1, 1, None, 300),
                    (0, 2, 1, None, 1100), (T.WIDE, 12, 1, None, 4000)} <= f, (regime, hyper, f)
            assert {(0, C, 1, x, 300) for C in (2, 3) for x in ("0", "1")} <= f, (regime, hyper, f)
    for hyper in T.HYPERS:
        f = forms(lambda i: i[1] == T.ALL and i[2] > 0 and i[3] == hyper)
        assert {(T.MASK, 1, 1, None, 300), (T.MASK, 1, 1, None, 1000), (T.MASK, 2, 1, None, 1100), (T.MASK | T.SEG, 1, 1, None, 300),
                (T.MASK, 2, 1, None, 300), (T.MASK | T.WIDE, 12, 1, None, 4000)} <= f, (hyper, f)
    fall = {(planned[nm]["core_kernel"], i[2] > 0) for nm, (i, e, x) in cases.items() if i[1] == T.ALL and i[3] == "per_trait"}
    assert {(2, False), (2, True), (3, True)} <= fall
    schemes = {(i[6], i[5], i[4] is not None) for i, e, x in cases.values() if i[1] == T.ALL and i[3] == "per_trait"}
    assert {("global", 1, True), ("global_local", 3, True), ("global_local", 5, False)} <= schemes
    assert T.SHARD_INPUT[1] == ("scale",) and T.SHARD_INPUT[3] == "per_trait" and T.SHARD_INPUT[0][2] == 40
    assert T.SHARD_RANGES[0][1] == T.SHARD_RANGES[1][0] and T.SHARD_RANGES[1][0] % REGIME_BLOCK != 0
    # a padding-only tile under AQ_TT = 2: three trait tiles in groups of two
    assert all(i[0][2] == 40 for i, e, x in cases.values() if e.get("AQ_TT") == "2")


def test_committed_measurements_admit_every_input():
    """MEASURED has every sweep count and field; every input's own reference-side deviation is at most CAP / 10 in every capped
    field (the condition under which a case may stay in the GPU file); and no bar exceeds its cap."""
    fields = set(T.CAP)
    noanneal = next(i for i, _ in INPUTS if i[4] is None)
    for s in T.SWEEPS:
        assert set(T.MEASURED[s]) >= fields - {"elbo"} and (s in (1, 3) or "elbo" in T.MEASURED[s]), s
        assert set(T.MEASURED_NOANNEAL[s]) == fields, s            # without a ladder every sweep evaluates the ELBO
        for f in T.MEASURED[s]:
            assert T.bar(s, f) <= T.CAP[f]
        for f in fields:
            assert T.bar(s, f, noanneal) <= T.CAP[f]
    assert set(T.WORST_OF_INPUT) == {_iid(i) for i, _ in INPUTS} >= {i for i, s in T.EXCLUDED_RUNS}
    over = {n: {f: v for f, v in w.items() if not v <= 0.1} for n, w in T.WORST_OF_INPUT.items()}
    assert not {n: w for n, w in over.items() if w}, over
