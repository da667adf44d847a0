"""CPU: what tests/test_gpu_shard_schemes.py claims about its inputs, cuts and kernel mix -- on the data, the planner and the
oracle alone, so that the coverage of the sharded runs cannot shrink unnoticed.

  * the missing counts of every shard of tests.util.make_shard_problem("hetero"): none | 1 ... AQ_MIS_MMAX | more;
  * the plan of every shard (aq_plan_query, 256 CUs, the missing counts of the shard's own columns, the rank's own hooks) is the
    instance the GPU case asserts from its handle -- or, for aq_vb_run_multi, which reports no per-rank status, relies on;
  * the cuts: 16 / 16 / 16, 16 / 32, 16 + 1, 16 + 16 + 1 from aq_vb_partition, and VbRun ranks that start inside a trait tile;
  * the oracle converges in fewer than 150 sweeps on every (input, scheme) the GPU file runs;
  * a shard slip -- a shard's own q where the whole problem's belongs -- moves the oracle's theta_vb, gam_vb and ELBO by more than
    1000 times their bars under the global scheme, df = 1 and df = 3: the cases can see one."""
import numpy as np
import pytest

from atlasqtl_amd.core import plan_query, vb_partition
from tests import test_gpu_shard_schemes as T
from tests.util import SHARD_HETERO_NA, SHARD_HETERO_SHAPE, SHARD_HETERO_TRAIT

MEM = 288 * 10**9          # device memory of the planned cases: more than any of them needs
NCU = 256
TILE = 16


def _missing(prob, k0, k1):
    m = np.isnan(prob["Y"][:, k0:k1]).sum(axis=0)
    return m, int(m.max()), int(np.minimum(m, prob["Y"].shape[0] - m).max())


def _plan(prob, k0, k1, hooks, fields):
    _, mm, ms = _missing(prob, k0, k1)
    st = plan_query(prob["Y"].shape[0], prob["p"], k1 - k0, mm, ms, ncu=NCU, total_bytes=MEM, overrides=dict(hooks))
    return {k: st[k] for k in fields}


def test_scheme_list_is_the_one_the_sharded_runs_are_held_to():
    assert list(T.SCHEMES.values()) == [("global_local", 1, (1, 2, 10)), ("global", 1, (1, 2, 10)), ("global", 1, None),
                                        ("global_local", 3, (1, 2, 10)), ("global_local", 3, None), ("global_local", 5, None),
                                        ("global_local", 7, (2, 3, 5))]
    assert {s for n, s in T.MULTI_HETERO if n == 3} == set(T.SCHEMES) and len(T.MULTI_HETERO) == len(T.SCHEMES) + 2
    assert {T.SCHEMES[s][:2] for n, s in T.MULTI_HETERO if n == 2} == {("global", 1), ("global_local", 3)}
    assert {T.SCHEMES[s][:2] for s in T.RANK_SCHEMES} == {("global_local", 1), ("global", 1), ("global_local", 3), ("global_local", 5)}
    for group in (T.EDGE_SCHEMES, T.ONE_RANK_SCHEMES, T.STATE_SCHEMES, T.NCCL_SCHEMES):
        assert "global-anneal" in group and len(group) == 2
    assert set(T.STATE_SCHEMES) <= set(T.RANK_SCHEMES) and all(T.STATE_SWEEPS < T.SCHEMES[s][2][2] for s in T.STATE_SCHEMES)


def test_hetero_input_holds_three_kinds_of_shard():
    prob = T.problem(T.HETERO)
    n, p, q = SHARD_HETERO_SHAPE
    assert (prob["Y"].shape, prob["X"].shape, prob["p"], prob["q"]) == ((n, q), (n, p), p, q), "prepare_xy removed a column"
    m, _, _ = _missing(prob, 0, q)
    k0, k1, frac = SHARD_HETERO_NA
    kt, mt = SHARD_HETERO_TRAIT
    assert (k0, k1) == (16, 32) and 32 <= kt < 48 and mt > T.MIS_MMAX
    assert np.all(m[:k0] == 0) and np.all(np.delete(m[k1:], kt - k1) == 0) and m[kt] == mt
    assert np.all(m[k0:k1] >= 1) and m[k0:k1].max() <= T.MIS_MMAX and 0.03 * n <= m[k0:k1].mean() <= 0.07 * n
    np.testing.assert_allclose(np.nanmean(prob["Y"], axis=0), 0.0, atol=1e-12)        # re-centred over the observed rows
    # ... so per shard of three: complete | 1 ... AQ_MIS_MMAX | beyond; of two (16 + 32 traits): complete | beyond
    for n_parts, want in ((3, [(0, 0), (1, T.MIS_MMAX), (T.MIS_MMAX + 1, n)]), (2, [(0, 0), (T.MIS_MMAX + 1, n)])):
        for ((a, b), _), (lo, hi) in zip(T.HETERO_PLANS[n_parts], want):
            assert lo <= _missing(prob, a, b)[1] <= hi, (n_parts, a, b)


@pytest.mark.parametrize("n_parts", sorted(T.HETERO_PLANS))
def test_hetero_shards_are_cut_and_planned_as_the_gpu_cases_rely_on(n_parts, hiplib):
    prob = T.problem(T.HETERO)
    rows = T.HETERO_PLANS[n_parts]
    assert vb_partition(prob["q"], n_parts) == [cut for cut, _ in rows]
    assert [cut for cut, _ in rows] == {3: [(0, 16), (16, 32), (32, 48)], 2: [(0, 16), (16, 48)]}[n_parts]
    for (k0, k1), want in rows:
        assert _plan(prob, k0, k1, {}, want) == want, (k0, k1)
    kinds = [(w["core_kernel"], w["instance_flags"]) for _, w in rows]
    assert kinds == {3: [(0, 0), (0, T.MASK), (2, 0)], 2: [(0, 0), (2, 0)]}[n_parts]
    # the single handle the shards are compared with is another kernel than two of them: the generic one on all 48 traits
    assert _plan(prob, 0, prob["q"], {}, ("core_kernel",)) == {"core_kernel": 2}


@pytest.mark.parametrize("q", sorted(T.EDGE_CUTS))
def test_partition_edges_end_in_a_shard_of_one_trait(q, hiplib):
    prob = T.problem(("small", q, T.SMALL_NA))
    cuts = T.EDGE_CUTS[q]
    assert vb_partition(q, len(cuts)) == cuts
    assert [b - a for a, b in cuts] == {17: [16, 1], 33: [16, 16, 1]}[q]
    for k0, k1 in cuts:
        assert 1 <= _missing(prob, k0, k1)[1] <= T.MIS_MMAX, (k0, k1)        # every shard, the single trait too, has NA
        assert _plan(prob, k0, k1, {}, T.EDGE_PLAN) == T.EDGE_PLAN, (k0, k1)


def test_rank_cuts_hold_a_ragged_tile_and_two_starts_inside_a_tile():
    cuts = T.RANK_CUTS
    assert cuts[0][0] == 0 and cuts[-1][1] == 40 and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    assert cuts[0][1] < TILE                                                   # the first shard: one ragged tile
    assert all(k0 % TILE != 0 for k0, k1 in cuts[1:])                          # [9, 24) and [24, 40) start inside a tile
    assert len(cuts) + 1 <= 4                                                  # the workers and the test process on one GPU
    for key, hooks, plans in T.ASSIGNMENTS.values():
        assert key[:2] == ("small", 40) and len(hooks) == len(plans) == len(cuts)


@pytest.mark.parametrize("assignment", sorted(T.ASSIGNMENTS))
def test_every_rank_is_planned_the_instance_it_asserts(assignment, hiplib):
    """Each rank's own hooks on its own columns: the fields the worker asserts from aq_vb_status before it runs."""
    key, hooks, plans = T.ASSIGNMENTS[assignment]
    prob = T.problem(key)
    for (k0, k1), h, want in zip(T.RANK_CUTS, hooks, plans):
        _, mm, _ = _missing(prob, k0, k1)
        assert (1 <= mm <= T.MIS_MMAX) if key[2] else mm == 0
        assert _plan(prob, k0, k1, h, want) == want, (assignment, k0, k1, h)
    kinds = [(w["core_kernel"], w["instance_flags"], w["split_parts"], w["chain_segments"]) for w in plans]
    assert len(set(kinds)) == len(kinds)                                       # no two ranks run the same kernel form
    if assignment == "mask":
        assert kinds == [(0, T.MASK, 2, 0), (0, T.MASK | T.SEG, 1, 3), (3, 0, 3, 0)]
    else:
        assert kinds == [(0, T.WIDE, 9, 0), (2, 0, 1, 0), (0, 0, 1, 0)]
    # the hooks are what makes the mix: left alone every rank gets the same instance
    own = [_plan(prob, k0, k1, {}, ("core_kernel", "instance_flags", "split_parts", "chain_segments")) for k0, k1 in T.RANK_CUTS]
    assert all(o == own[0] for o in own)


@pytest.mark.parametrize("key,name", T.runs(), ids=[f"{'-'.join(str(v) for v in k)}-{s}" for k, s in T.runs()])
def test_oracle_converges_on_every_input_and_scheme_of_the_gpu_file(key, name):
    ref, lref = T.reference(key, name)
    assert ref["converged"] and ref["it"] < 150 and lref.size >= 2
    for f in ("theta_vb", "zeta_vb", "mu_beta_vb", "gam_vb", "tau_vb", "sig2_theta_vb", "lam2_inv_vb"):
        assert np.all(np.isfinite(ref[f])), f


@pytest.mark.parametrize("name", ["global-anneal", "local-df1-anneal", "df3-anneal"])
def test_a_shard_slip_is_seen(name):
    """shr_fac_inv = 16, a shard's own q, in place of 48 (what q_total carries into sig2_theta, the p-vector update and the
    ELBO), 12 sweeps: theta_vb, gam_vb and the ELBO move by more than 1000 times their bars."""
    slip_q = T.HETERO_PLANS[3][0][0][1] - T.HETERO_PLANS[3][0][0][0]
    assert slip_q == 16 != T.problem(T.HETERO)["q"]
    ref, lref = T.reference(T.HETERO, name, maxit=12, thinned=False)
    alt, lalt = T.reference(T.HETERO, name, maxit=12, shr_fac_inv=slip_q, thinned=False)
    assert ref["it"] == alt["it"] == 12 and lref.shape == lalt.shape and lref.size >= 2
    theta = T._bar(alt["theta_vb"], ref["theta_vb"], 1e-6, 1e-10)
    gam = float(np.max(np.abs(alt["gam_vb"] - ref["gam_vb"])))
    elbo = T._rel(lalt, lref)
    print(f"\nSLIP scheme={name} theta_bar={theta:.3e} gam_abs={gam:.3e} elbo_rel={elbo:.3e}")
    assert theta > 1000.0 and gam > 1000.0 * 1e-9 and elbo > 1000.0 * 1e-9
