"""GPU: trait-sharded runs under every scheme and with a different kernel on every shard, against the CPU oracle on the whole
problem and against the single-handle run.

Every multi-GPU configuration is a run sharded over traits, and the shards on one GPU are the only evidence for it.  Until this
file every sharded test ran the horseshoe with df = 1 and gave all its shards the same kind of kernel.  Here:
  A  aq_vb_run_multi in 3 and 2 shards on tests.util.make_shard_problem("hetero"): shard 0 complete (look-ahead kernel), shard 1
     with NA (its MASK instance), shard 2 with a trait of 1030 missing samples (generic kernel) -- all seven SCHEMES;
  B  partition edges: a last shard of ONE trait (16 + 1, 16 + 16 + 1);
  C  aq_vb_run_multi with one rank through RCCL, global scheme and df = 3;
  D  three VbRun ranks over [0, 9), [9, 24), [24, 40) -- a ragged single tile, two shards that start inside a tile -- every rank
     with launch hooks of its own, so that the ranks run different kernels by construction (each asserts its instance from
     aq_vb_status before it runs);
  E  get_state / set_state inside a shard, mid-ladder, all ranks in step;
  F  a one-rank nccl group: RankGroup.allreduce_device reduces the payload where it lies on the device.
The global scheme, df = 3, 5, 7 and the annealed Kummer update take branches of the p-vector and ELBO kernels in which q_total,
the replicated p-sum of the ELBO and the tail of the all-reduce payload enter; with one handle q_total == q, so only a sharded run
can see a slip there.  tests/test_shard_coverage_host.py asserts on the CPU what the inputs, cuts and plans below claim.

Bars: against the oracle those of tests/test_gpu_schemes.py::_compare (plus tau_vb as tests/test_gpu_split_instances.py::_check),
against the single handle tests/test_gpu_multi.py::_same.  Observed on an MI355X, worst of each family (ELBO relative /
mu_beta_vb as a fraction of its bar / gam_vb absolute): see DESIGN.md section 3."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MASK, WIDE, SEG = 1, 2, 4        # aq_vb_status.instance_flags
LADDER = (1, 2, 10)
MAXIT = 1000
MIS_MMAX = 1024                  # AQ_MIS_MMAX: more missing samples in a trait hand the handle to the generic kernel

# name -> (scheme, df, anneal)
SCHEMES = {
    "local-df1-anneal": ("global_local", 1, LADDER),
    "global-anneal": ("global", 1, LADDER),
    "global": ("global", 1, None),
    "df3-anneal": ("global_local", 3, LADDER),
    "df3": ("global_local", 3, None),
    "df5": ("global_local", 5, None),
    "df7-anneal": ("global_local", 7, (2, 3, 5)),
}

HETERO = ("hetero",)
SMALL_NA = 0.04

# --- A. aq_vb_run_multi on "hetero": (shards, scheme)
MULTI_HETERO = [(3, s) for s in SCHEMES] + [(2, "global-anneal"), (2, "df3-anneal")]
# the plan of every shard at 256 CUs (aq_vb_run_multi reports no per-rank status: tests/test_shard_coverage_host.py proves these
# from aq_plan_query with the missing counts of the shard's own columns): shards -> [(cut, plan fields)]
HETERO_PLANS = {
    3: [((0, 16), dict(core_kernel=0, instance_flags=0, split_parts=2, tiles_matrix=7, tiles_matrix2=7, chain_segments=0, n_pad=1344)),
        ((16, 32), dict(core_kernel=0, instance_flags=MASK, split_parts=2, tiles_matrix=7, tiles_matrix2=7, chain_segments=0, n_pad=1344)),
        ((32, 48), dict(core_kernel=2, instance_flags=0, split_parts=1, tiles_matrix=0, tiles_matrix2=0, chain_segments=0, n_pad=2048))],
    # (aq_vb_partition deals out whole 16-trait tiles: three tiles in two parts are 16 + 32 traits, not 24 + 24)
    2: [((0, 16), dict(core_kernel=0, instance_flags=0, split_parts=2, tiles_matrix=7, tiles_matrix2=7, chain_segments=0, n_pad=1344)),
        ((16, 48), dict(core_kernel=2, instance_flags=0, split_parts=1, tiles_matrix=0, tiles_matrix2=0, chain_segments=0, n_pad=2048))],
}

# --- B. partition edges through aq_vb_run_multi, "small" with 4 % NA: q -> the cuts of aq_vb_partition
EDGE_CUTS = {17: [(0, 16), (16, 17)], 33: [(0, 16), (16, 32), (32, 33)]}
EDGE_SCHEMES = ("global-anneal", "df5")
EDGE_PLAN = dict(core_kernel=0, instance_flags=MASK, split_parts=1, tiles_matrix=4, tiles_matrix2=3, chain_segments=0, n_pad=336)   # every shard

# --- C. one rank through RCCL
ONE_RANK_INPUT = ("small", 40, SMALL_NA)
ONE_RANK_SCHEMES = ("global-anneal", "df3-anneal")

# --- D. VbRun ranks with hooks of their own: assignment -> (input, per-rank hooks, per-rank plan fields)
RANK_CUTS = ((0, 9), (9, 24), (24, 40))
RANK_SCHEMES = ("local-df1-anneal", "global-anneal", "df3-anneal", "df5")
ASSIGNMENTS = {
    "mask": (("small", 40, SMALL_NA),
             ({"AQ_LA_C": "2", "AQ_LA_XHELPER": "1"}, {"AQ_CHAIN": "3"}, {"AQ_KERNEL": "3", "AQ_MIS_C": "3"}),
             (dict(core_kernel=0, instance_flags=MASK, split_parts=2, tiles_matrix=2, tiles_matrix2=2, chain_segments=0, n_pad=384),
              dict(core_kernel=0, instance_flags=MASK | SEG, split_parts=1, tiles_matrix=4, tiles_matrix2=3, chain_segments=3, n_pad=336),
              dict(core_kernel=3, instance_flags=0, split_parts=3, tiles_matrix=1, tiles_matrix2=0, chain_segments=0, n_pad=384))),
    "complete": (("small", 40, 0.0),
                 ({"AQ_LA_C": "9"}, {"AQ_KERNEL": "2"}, {}),
                 (dict(core_kernel=0, instance_flags=WIDE, split_parts=9, tiles_matrix=1, tiles_matrix2=1, chain_segments=0, n_pad=864),
                  dict(core_kernel=2, instance_flags=0, split_parts=1, tiles_matrix=0, tiles_matrix2=0, chain_segments=0, n_pad=512),
                  dict(core_kernel=0, instance_flags=0, split_parts=1, tiles_matrix=4, tiles_matrix2=3, chain_segments=0, n_pad=336))),
}

# --- E. state inside a shard: within the spawn of assignment "mask"
STATE_ASSIGNMENT = "mask"
STATE_SCHEMES = ("global-anneal", "df3-anneal")
STATE_SWEEPS = 6                 # mid-ladder: the ladders have 10 rungs

# --- F. one-rank nccl group
NCCL_INPUT = ("small", 40, SMALL_NA)
NCCL_SCHEMES = ("local-df1-anneal", "global-anneal")

RESULT_FIELDS = ("beta_vb", "gam_vb", "mu_beta_vb", "theta_vb", "zeta_vb", "lam2_inv_vb", "sig2_theta_vb", "tau_vb", "sig2_beta_vb")
Q_FIELDS = ("beta_vb", "gam_vb", "mu_beta_vb", "zeta_vb", "tau_vb", "sig2_beta_vb")      # a rank holds its own traits of these


def runs():
    """Every (input, scheme) this file runs, for tests/test_shard_coverage_host.py."""
    out = {(HETERO, s) for _, s in MULTI_HETERO}
    out |= {(("small", q, SMALL_NA), s) for q in EDGE_CUTS for s in EDGE_SCHEMES}
    out |= {(ONE_RANK_INPUT, s) for s in ONE_RANK_SCHEMES} | {(NCCL_INPUT, s) for s in NCCL_SCHEMES}
    out |= {(inp, s) for inp, _, _ in ASSIGNMENTS.values() for s in RANK_SCHEMES}
    return sorted(out, key=str)


@functools.lru_cache(maxsize=None)
def problem(key):
    from tests.util import make_shard_problem
    return make_shard_problem(*key)


@functools.lru_cache(maxsize=None)
def reference(key, name, maxit=MAXIT, shr_fac_inv=None, thinned=True):
    """The oracle's run of the WHOLE problem: (result, ELBO trace).  Computed once per (input, scheme); left unchanged."""
    from oracle import atlasqtl_oracle as O
    scheme, df, anneal = SCHEMES[name]
    prob = problem(key)
    li = prob["list_init"]
    if scheme == "global":           # that core has no local scales
        li = dict({k: v for k, v in li.items() if k != "sig2_theta_vb"}, sig2_theta_vb=np.ones(prob["p"]))
    tr = []
    ref = O.atlasqtl_global_local_core_(prob["Y"], prob["X"], prob["q"] if shr_fac_inv is None else shr_fac_inv, anneal, df, 0.1, maxit,
                                        prob["list_hyper"], li, thinned_elbo_eval=thinned, trace=tr, full_output=True, scheme=scheme)
    return ref, np.array([r["lb"] for r in tr if r["lb"] is not None])


@functools.lru_cache(maxsize=None)
def single(key, name):
    """The single-handle GPU run of the whole problem (what the other GPU tests hold to the oracle)."""
    import atlasqtl_amd as A
    scheme, df, anneal = SCHEMES[name]
    prob = problem(key)
    return A.atlasqtl_global_local_core_(prob["Y"], prob["X"], prob["q"], anneal, df, 0.1, MAXIT, 0, prob["list_hyper"],
                                         prob["list_init"], full_output=True, debug=True, scheme=scheme)


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _bar(a, b, rtol, atol):
    """Largest |a - b| as a fraction of the bar atol + rtol |b| of assert_allclose."""
    return float(np.max(np.abs(a - b) / (atol + rtol * np.abs(b))))


def hold(family, label, name, ref, lref, got):
    """got (the fields of atlasqtl_global_local_core_ with full_output) against the oracle at the bars of
    tests/test_gpu_schemes.py::_compare; the observed deviations are printed before they are asserted."""
    scheme, df, anneal = SCHEMES[name]
    rtol_scale = 1e-9 if df in (1, 3) else 1e-7      # df = 5, 7: the reason is recorded in tests/test_gpu_schemes.py
    lgot = got["elbo_trace"][1]
    assert got["it"] == ref["it"] and bool(got["converged"]) == bool(ref["converged"]), (got["it"], ref["it"])
    assert lgot.shape == lref.shape
    print(f"\nDEV family={family} case={label} scheme={name} it={got['it']} elbo_rel={_rel(lgot, lref):.3e} "
          f"mu_bar={_bar(got['mu_beta_vb'], ref['mu_beta_vb'], 1e-6, 1e-10):.3e} "
          f"gam_abs={np.max(np.abs(got['gam_vb'] - ref['gam_vb'])):.3e} "
          f"theta_bar={_bar(got['theta_vb'], ref['theta_vb'], 1e-6, 1e-10):.3e} "
          f"zeta_bar={_bar(got['zeta_vb'], ref['zeta_vb'], 1e-6, 1e-10):.3e} tau_rel={_rel(got['tau_vb'], ref['tau_vb']):.3e} "
          f"sig2_theta_rel={_rel(got['sig2_theta_vb'], ref['sig2_theta_vb']):.3e} "
          f"sig02_inv_rel={abs(got['sig02_inv_vb'] - ref['sig02_inv_vb']) / abs(ref['sig02_inv_vb']):.3e} "
          f"lam2_inv_rel={_rel(got['lam2_inv_vb'], ref['lam2_inv_vb']):.3e}")
    np.testing.assert_allclose(lgot, lref, rtol=1e-9)
    assert np.all(np.diff(lgot) > -1.5e-8)
    np.testing.assert_allclose(got["mu_beta_vb"], ref["mu_beta_vb"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(got["gam_vb"], ref["gam_vb"], atol=1e-9)
    np.testing.assert_allclose(got["theta_vb"], ref["theta_vb"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(got["zeta_vb"], ref["zeta_vb"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(got["tau_vb"], ref["tau_vb"], rtol=1e-8)
    np.testing.assert_allclose(got["sig2_theta_vb"], ref["sig2_theta_vb"], rtol=rtol_scale)
    np.testing.assert_allclose(got["sig02_inv_vb"], ref["sig02_inv_vb"], rtol=rtol_scale)
    if scheme == "global":
        np.testing.assert_array_equal(got["lam2_inv_vb"], 1.0)
    else:
        np.testing.assert_allclose(got["lam2_inv_vb"], ref["lam2_inv_vb"], rtol=1e-6)


def _multi(key, name, n_parts, transport=1):
    from atlasqtl_amd.core import run_multi
    scheme, df, anneal = SCHEMES[name]
    prob = problem(key)
    return run_multi(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], anneal, 0.1, MAXIT, n_gpus=n_parts,
                     devices=[0] * n_parts if transport == 1 else None, transport=transport, scheme=scheme, df=df)


# ------------------------------------------------------------------------------------------------------------------------------
# A. three kernel families side by side, every scheme

@pytest.mark.parametrize("n_parts,name", MULTI_HETERO, ids=[f"{n}-{s}" for n, s in MULTI_HETERO])
def test_run_multi_heterogeneous_shards_match_oracle_and_single_handle(n_parts, name, monkeypatch):
    """Look-ahead, MASK and generic shards (16 + 32 traits with two: look-ahead and generic) put their p + 8 and 8 doubles into
    one all-reduce: whole runs of every scheme against the oracle and the single handle (which runs the generic kernel on all 48
    traits)."""
    from atlasqtl_amd.core import vb_partition
    from tests.test_gpu_multi import _same
    from tests.test_gpu_split_instances import _pin_256_cus
    _pin_256_cus(monkeypatch)
    assert vb_partition(problem(HETERO)["q"], n_parts) == [cut for cut, _ in HETERO_PLANS[n_parts]]
    ref, lref = reference(HETERO, name)
    got = _multi(HETERO, name, n_parts)
    hold("A", f"hetero-{n_parts}", name, ref, lref, got)
    _same(got, single(HETERO, name))


# ------------------------------------------------------------------------------------------------------------------------------
# B. a shard of one trait

@pytest.mark.parametrize("name", EDGE_SCHEMES)
@pytest.mark.parametrize("q", sorted(EDGE_CUTS))
def test_run_multi_last_shard_of_one_trait_matches_oracle_and_single_handle(q, name, monkeypatch):
    """q = 17 in 16 + 1 and q = 33 in 16 + 16 + 1 traits, 4 % NA: what aq_vb_partition produces for them."""
    from atlasqtl_amd.core import vb_partition
    from tests.test_gpu_multi import _same
    from tests.test_gpu_split_instances import _pin_256_cus
    _pin_256_cus(monkeypatch)
    key = ("small", q, SMALL_NA)
    cuts = EDGE_CUTS[q]
    assert vb_partition(q, len(cuts)) == cuts and cuts[-1][1] - cuts[-1][0] == 1
    ref, lref = reference(key, name)
    got = _multi(key, name, len(cuts))
    hold("B", f"small-q{q}-{len(cuts)}", name, ref, lref, got)
    _same(got, single(key, name))


# ------------------------------------------------------------------------------------------------------------------------------
# C. one rank through RCCL

@pytest.mark.parametrize("name", ONE_RANK_SCHEMES)
def test_run_multi_one_rank_through_rccl_equals_single_handle(name):
    """The threads, barriers, collectives and gather of eight ranks with one: the same kernels, so the same result to 1e-13."""
    from tests.test_gpu_multi import _same
    ref, lref = reference(ONE_RANK_INPUT, name)
    got = _multi(ONE_RANK_INPUT, name, 1, transport=0)
    hold("C", "small-q40-rccl1", name, ref, lref, got)
    _same(got, single(ONE_RANK_INPUT, name), tol_mu=1e-13)


# ------------------------------------------------------------------------------------------------------------------------------
# D, E. VbRun ranks, each with its own kernel

def _snapshot(run):
    st = run.status()
    its, lbs = run.elbo_trace()
    return dict(run.result(full_output=True), it=st["it"], converged=st["converged"], sig02_inv_vb=st["sig02_inv_vb"],
                elbo_it=its, elbo_lb=lbs)


def _load(path):
    z = np.load(path)
    out = {k: z[k] for k in z.files}
    out.update(it=int(z["it"]), converged=bool(z["converged"]), sig02_inv_vb=float(z["sig02_inv_vb"]),
               elbo_trace=(z["elbo_it"], z["elbo_lb"]))
    return out


def _assert_plan(st, want):
    got = {k: st[k] for k in want}
    assert got == want, f"planned {got}, the case is written for {want} (hooks in effect: {st['overrides']!r})"


def _rank_worker(rank, world, port, outdir, assignment):
    """One rank of assignment: its own hooks in its own environment before any handle exists; every scheme of RANK_SCHEMES as a
    whole run, one .npz each; for STATE_SCHEMES of STATE_ASSIGNMENT also the run interrupted after STATE_SWEEPS sweeps and
    continued on a new handle.  Every step is a collective: all ranks take the same ones in the same order."""
    key, hooks, plans = ASSIGNMENTS[assignment]
    for k, v in hooks[rank].items():
        os.environ[k] = v
    from tests.util import gloo_rank, shard_lists
    dist = gloo_rank(rank, world, port)
    import torch
    from atlasqtl_amd.core import VbRun
    if torch.cuda.get_device_properties(0).multi_processor_count > 256:     # the plans above are those of 256 CUs
        os.environ["AQ_NCU"] = "256"
    prob = problem(key)
    k0, k1 = RANK_CUTS[rank]
    lh, li = shard_lists(prob["list_hyper"], prob["list_init"], k0, k1)
    Y = np.asfortranarray(prob["Y"][:, k0:k1])
    for name in RANK_SCHEMES:
        scheme, df, anneal = SCHEMES[name]

        def handle():
            return VbRun(Y, prob["X"], lh, li, anneal, 0.1, MAXIT, True, True, q_total=prob["q"], process_group=dist.group.WORLD,
                         trait_offset=k0, scheme=scheme, df=df)
        run = handle()
        try:
            _assert_plan(run.status(), plans[rank])
            assert run.ranks.host_staged and run.world == world
            run.run()
            np.savez(os.path.join(outdir, f"{name}-rank{rank}.npz"), **_snapshot(run))
        finally:
            run.close()
        if assignment == STATE_ASSIGNMENT and name in STATE_SCHEMES:
            run = handle()
            try:
                run.run_sweeps(STATE_SWEEPS)
                assert run.status()["it"] == STATE_SWEEPS < anneal[2]
                blob = run.get_state()
            finally:
                run.close()
            run = handle()
            try:
                run.set_state(blob)
                assert run.status()["it"] == STATE_SWEEPS
                run.run()
                np.savez(os.path.join(outdir, f"{name}-rank{rank}-resumed.npz"), **_snapshot(run))
            finally:
                run.close()
    dist.destroy_process_group()


def _spawn(tmp_path_factory, assignment):
    from tests.util import spawn_ranks
    out = tmp_path_factory.mktemp(f"ranks-{assignment}")
    spawn_ranks(_rank_worker, len(RANK_CUTS), str(out), assignment)      # three workers and this process hold the GPU
    return out


@pytest.fixture(scope="module")
def ranks_mask(tmp_path_factory):
    return _spawn(tmp_path_factory, "mask")


@pytest.fixture(scope="module")
def ranks_complete(tmp_path_factory):
    return _spawn(tmp_path_factory, "complete")


def _hold_ranks(outdir, assignment, name):
    key = ASSIGNMENTS[assignment][0]
    r = [_load(outdir / f"{name}-rank{i}.npz") for i in range(len(RANK_CUTS))]
    for other in r[1:]:
        assert other["it"] == r[0]["it"] and other["converged"] == r[0]["converged"]
        np.testing.assert_array_equal(other["elbo_trace"][0], r[0]["elbo_trace"][0])
        for f in ("theta_vb", "lam2_inv_vb", "sig2_theta_vb"):
            np.testing.assert_array_equal(other[f], r[0][f], err_msg=f)
        np.testing.assert_array_equal(other["elbo_trace"][1], r[0]["elbo_trace"][1])
        assert other["sig02_inv_vb"] == r[0]["sig02_inv_vb"]
    for (k0, k1), part in zip(RANK_CUTS, r):
        assert part["gam_vb"].shape == (problem(key)["p"], k1 - k0)
    got = dict(r[0])
    got.update({f: np.concatenate([part[f] for part in r], axis=-1) for f in Q_FIELDS})
    ref, lref = reference(key, name)
    hold("D", f"ranks-{assignment}", name, ref, lref, got)
    return got


@pytest.mark.parametrize("name", RANK_SCHEMES)
def test_ranks_with_masked_kernels_of_three_kinds_match_oracle(name, ranks_mask):
    """4 % NA: MASK 2/2 in two parts with the exchange on the helper wave | MASK 4/3 in three chained segments | the masked
    two-barrier kernel in three parts."""
    from tests.test_gpu_multi import _same
    got = _hold_ranks(ranks_mask, "mask", name)
    _same(got, single(ASSIGNMENTS["mask"][0], name))


@pytest.mark.parametrize("name", RANK_SCHEMES)
def test_ranks_with_wide_split_generic_and_plain_kernels_match_oracle(name, ranks_complete):
    """Complete Y: the wide split 1/1 in nine parts | the generic kernel | the look-ahead kernel 4/3 as planned."""
    from tests.test_gpu_multi import _same
    got = _hold_ranks(ranks_complete, "complete", name)
    _same(got, single(ASSIGNMENTS["complete"][0], name))


@pytest.mark.parametrize("name", STATE_SCHEMES)
def test_state_saved_and_restored_inside_a_shard_continues_bit_identically(name, ranks_mask):
    """Six sweeps (mid-ladder), get_state, a new handle, set_state, run on -- on every rank in step: every result field and the
    ELBO trace as the uninterrupted run of the same rank."""
    for rank in range(len(RANK_CUTS)):
        a, b = _load(ranks_mask / f"{name}-rank{rank}.npz"), _load(ranks_mask / f"{name}-rank{rank}-resumed.npz")
        assert (a["it"], a["converged"], a["sig02_inv_vb"]) == (b["it"], b["converged"], b["sig02_inv_vb"]) and a["it"] > STATE_SWEEPS
        np.testing.assert_array_equal(a["elbo_trace"][0], b["elbo_trace"][0])
        np.testing.assert_array_equal(a["elbo_trace"][1], b["elbo_trace"][1])
        for f in RESULT_FIELDS:
            np.testing.assert_array_equal(a[f], b[f], err_msg=f"rank {rank} {f}")


# ------------------------------------------------------------------------------------------------------------------------------
# F. the payload reduced where it lies on the device

def _nccl_worker(rank, world, port, outdir):
    """One rank in an nccl group: VbRun with the group, then without, on the same device in the same process."""
    import torch
    from tests.util import gloo_rank
    torch.cuda.set_device(0)
    dist = gloo_rank(rank, world, port, backend="nccl")
    from atlasqtl_amd.core import VbRun
    prob = problem(NCCL_INPUT)
    for name in NCCL_SCHEMES:
        scheme, df, anneal = SCHEMES[name]
        for tag, group in (("group", dist.group.WORLD), ("plain", None)):
            run = VbRun(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], anneal, 0.1, MAXIT, True, True, q_total=prob["q"],
                        process_group=group, trait_offset=0, scheme=scheme, df=df)
            try:
                staged = -1 if group is None else int(run.ranks.host_staged)
                run.run()
                np.savez(os.path.join(outdir, f"{name}-{tag}.npz"), host_staged=staged, **_snapshot(run))
            finally:
                run.close()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def nccl_rank(tmp_path_factory):
    import torch.distributed as dist
    if not dist.is_nccl_available():
        pytest.skip("torch.distributed has no nccl backend in this build")
    from tests.util import spawn_ranks
    out = tmp_path_factory.mktemp("nccl-one-rank")
    spawn_ranks(_nccl_worker, 1, str(out))
    return out


@pytest.mark.parametrize("name", NCCL_SCHEMES)
def test_one_rank_nccl_group_reduces_on_the_device_and_equals_the_plain_run(name, nccl_rank):
    """RankGroup.allreduce_device's non-gloo branch: host_staged is False, the all-reduce runs on the payload buffer the library
    was given; with one rank the sum is the payload itself, so the run equals the one without a group."""
    from tests.test_gpu_multi import _same
    with_group, plain = _load(nccl_rank / f"{name}-group.npz"), _load(nccl_rank / f"{name}-plain.npz")
    assert int(with_group["host_staged"]) == 0
    ref, lref = reference(NCCL_INPUT, name)
    hold("F", "small-q40-nccl1", name, ref, lref, with_group)
    _same(with_group, plain, tol_mu=1e-13)
