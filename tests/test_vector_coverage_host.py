"""CPU: what tests/test_gpu_vector_edges.py claims about its tables -- on the tables, the sources, the planner and the oracle
alone, so that the coverage of the p- and q-vector kernels cannot shrink unnoticed.

  * the tables put a run on either side of every edge of the launch geometry, under every kernel form that owns the edge;
  * the geometry restated there (256, 1024, 64 x 4 quarters, 2048 rows per chunk, pblk) is that of aq_vb_create.hip, of the
    launch lines of aq_vb_sweep.hip and of aq_k_reduce_rows, so a geometry change fails here instead of going unnoticed;
  * no input loses a column to the duplicate filter; every case's plan comes out of aq_plan_query at 256 CUs as written;
  * the oracle's two forms (the Gram-space driver and oracle/sharded_oracle.py) agree on every df = 1 run within a tenth of
    every bar (a run that does not would go to EXCLUDED_RUNS with its figure and out of the GPU tables);
  * a slip is visible: eta, kappa or n0 rolled by one trait, S_gam and T2 short of the last trait, the p-sum of the ELBO short
    of the last predictor, the slowest Lentz element evaluated at the fast elements' count -- each more than 1000 x its bar."""
import os
import re

import numpy as np
import pytest

from atlasqtl_amd.core import plan_query
from tests import test_gpu_vector_edges as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "atlasqtl_amd", "csrc")
MEM = 288 * 10**9          # device memory of the planned cases: more than any of them needs
NCU = 256

# df = 1 runs on which the oracle's two forms disagree by more than a tenth of a bar: (input key, scheme, maxit, field, value)
EXCLUDED_RUNS = []


def _pad(x):
    return V.TILE * -(-x // V.TILE)


def geometry(case):
    """What a case's shape means to the kernels: blocks of q-threads, strides over q, strides over the Hpart entries, blocks
    of aq_k_reduce_rows, trait tiles, blocks of p-threads (pblk), strides over p, chunks of the pre-pass."""
    n, p, q, na, form = case
    ntile, nchunk = _pad(q) // V.TILE, -(-_pad(p) // V.CHUNK)
    return dict(qblocks=-(-_pad(q) // V.QBLOCK), qstrides=-(-q // V.STRIDE), hstrides=-(-(ntile * nchunk) // V.STRIDE),
                rowblocks=-(-_pad(p) // V.ROWS), ntile=ntile, pblk=-(-p // V.PBLOCK), pstrides=-(-p // V.STRIDE), chunks=nchunk)


def _reached(cases, field):
    return {geometry(c)[field] for c in cases}


def _df1_cases():
    return V.Q_CASES + V.P_CASES + V.T_CASES


def test_every_edge_has_a_run_on_both_sides_under_every_form_that_owns_it():
    df1 = _df1_cases()
    for na in (False, True):         # the complete-Y forms and the v.na forms of the look-ahead kernel
        own = [c for c in df1 if c[4] == "plain" and (c[3] > 0) == na and c[0] == V.Q_N]
        assert _reached(own, "qblocks") >= {1, 2, 5}, na             # q = 256 | 257 (aq_k_qpre, aq_k_qpost), 1025
        assert {c[2] for c in own} >= {256, 257, 1024, 1025, 2049}
        assert _reached(own, "qstrides") >= {1, 2, 3}                # q = 1024 | 1025, 2049 (aq_k_reduce_q_scalars, aq_k_elbo_q)
        assert {c[1] for c in own} >= {64, 65, 256, 257, 513, 1024, 1025, 2048, 2049}
        assert _reached(own, "rowblocks") >= {1, 2}                  # p = 64 | 65 (aq_k_reduce_rows: p_pad = 64 | 80)
        assert _reached(own, "pblk") >= {1, 2, 3, 4, 5, 8, 9}        # p = 256 | 257, 513 (aq_k_pvec_L, aq_k_pvec_finish)
        assert _reached(own, "pstrides") >= {1, 2, 3}                # p = 1024 | 1025, 2049 (aq_k_elbo_C)
        assert _reached(own, "chunks") >= {1, 2}                     # p = 2048 | 2049 (aq_k_prepass, the ELBO-only form)
    # the combine kernels (complete and NA), aq_k_sum_parts, the generic and the masked kernel: a second block of q-threads
    # and a second stride (one block and one stride is what the rest of the suite runs them with, q <= 100)
    for form, nas in V.Q_FORM_NA.items():
        for na in nas:
            own = [c for c in V.Q_CASES if c[4] == form and c[3] == na]
            assert {c[2] for c in own} == {257, 1025}, (form, na)
            assert _reached(own, "qblocks") == {2, 5} and _reached(own, "qstrides") == {1, 2}
    assert set(V.Q_FORM_NA) == {"chain3", "parts2", "generic", "masked"} and V.Q_FORM_NA["chain3"] == (0.0, V.NA)
    # the Hpart stride
    assert geometry(V.Q_HPART)["hstrides"] == 2 and geometry(V.Q_HPART)["ntile"] == 1025
    assert all(geometry(c)["hstrides"] == 1 for c in df1 if c != V.Q_HPART)
    # the write_AB pre-pass in one and two chunks, colApart summed over chunks in aq_k_qpost
    for form in ("generic", "masked"):
        own = [c for c in V.P_CASES if c[4] == form]
        assert _reached(own, "chunks") == {1, 2} and all(c[3] > 0 for c in own), form
        assert {c[1] for c in own} == {1025, 2049}
    # the quarters of aq_k_reduce_rows: t = c, c + 4, ... over 1 ... 5 and 8 | 9 tiles; gb_rows = 2, 4 with a second tile per quarter
    assert _reached([c for c in V.T_CASES if c[4] == "plain"], "ntile") == {1, 2, 3, 4, 5, 8, 9}
    for form in ("wpt2", "wpt4"):
        assert _reached([c for c in V.T_CASES if c[4] == form], "ntile") == {5, 9}, form
    assert V.T_WHOLE == [c for c in V.T_CASES if c[4] == "plain"]
    # the schemes: a second block of p-threads, a second stride over p, a second block of q-threads -- each of the six
    assert set(V.S_SCHEMES) == set(V.SCHEMES) - {V.DF1, "local-df1"}
    for name in V.S_SCHEMES:
        own = [c for c, s in V.S_CASES if s == name]
        assert _reached(own, "pblk") == {1, 2, 5} and _reached(own, "pstrides") == {1, 2} and _reached(own, "qblocks") == {1, 2}, name
    assert [V.SCHEMES[s] for s in V.S_SCHEMES] == [("global", 1, (1, 2, 10)), ("global", 1, None), ("global_local", 3, (1, 2, 10)),
                                                  ("global_local", 3, None), ("global_local", 5, None), ("global_local", 7, (2, 3, 5))]
    # the Lentz count: one block and a lone element in the second (257), three blocks (600); every placement, df = 1 and 3
    assert set(V.L_CASES) == {(p, pl, df) for p in (257, 600) for pl in V.L_PLACEMENTS for df in (1, 3)} and len(V.L_PLACEMENTS) == 5
    # the shards
    assert V.H_SHAPE[:3] == (300, 600, 300) and set(V.H_CASES) == {(n, s) for n in (2, 3) for s in (V.DF1, "global-anneal")}
    # the second handle for equal bits: one case of every (input, maxit), fixed by the tables
    rows = [(c, V.DF1, V.SWEEPS) for c in df1] + [(c, V.DF1, V.WHOLE) for c in V.T_WHOLE] + [(c, s, V.SWEEPS) for c, s in V.S_CASES]
    assert V.TWICE <= set(rows)
    assert sorted((c[:4], m) for c, _, m in V.TWICE) == sorted({(c[:4], m) for c, _, m in rows})


def _launches(text):
    """{kernel: [(grid expression, block size)]} of a source's hipLaunchKernelGGL lines."""
    out = {}
    for name, grid, block in re.findall(r"hipLaunchKernelGGL\((aq_k_\w+), dim3\((.+?)\), dim3\((\d+)\), 0, 0", text):
        out.setdefault(name, []).append((grid.replace(" ", ""), int(block)))
    return out


def test_geometry_constants_are_those_of_the_sources():
    create = open(os.path.join(CSRC, "aq_vb_create.hip")).read()
    assert f"s->pblk = (s->p + {V.PBLOCK - 1}) / {V.PBLOCK};" in create
    assert f"s->rows_per_chunk = {V.CHUNK};" in create
    assert "s->nHchunk = (s->p_pad + s->rows_per_chunk - 1) / s->rows_per_chunk;" in create
    assert "s->ppart.alloc_zeroed((size_t)3 * s->pblk)" in create
    assert "s->Hpart.alloc_zeroed((size_t)s->ntile * s->nHchunk)" in create and "s->colApart.alloc_zeroed((size_t)s->nHchunk * s->q_pad)" in create
    got = _launches(open(os.path.join(CSRC, "aq_vb_sweep.hip")).read())
    qgrid = (f"(s->q_pad+{V.QBLOCK - 1})/{V.QBLOCK}", V.QBLOCK)
    one = ("1", V.STRIDE)
    pgrid = ("s->pblk", V.PBLOCK)
    want = {"aq_k_qpre": {qgrid}, "aq_k_qpost": {qgrid}, "aq_k_combine_segment_sums": {qgrid}, "aq_k_combine_segment_sums6": {qgrid},
            "aq_k_sum_parts": {qgrid}, "aq_k_reduce_q_scalars": {one}, "aq_k_elbo_q": {one}, "aq_k_elbo_C": {one},
            "aq_k_scalars_post": {one}, "aq_k_scalars_post_global": {one}, "aq_k_elbo_C_global": {("1", 1)},     # (one thread: no stride)
            "aq_k_reduce_rows": {(f"(s->p_pad+{V.ROWS - 1})/{V.ROWS}", V.ROWS * V.QUARTERS)},
            "aq_k_pvec_L": {pgrid}, "aq_k_pvec_finish": {pgrid}, "aq_k_pvec_global": {pgrid},
            "aq_k_prepass": {("s->nHchunk,s->ntile", 256)}}
    for name, launches in want.items():
        assert set(got.get(name, [])) == launches, (name, got.get(name))
    sweep = open(os.path.join(CSRC, "aq_vb_sweep.hip")).read()
    assert "s->Hpart.get(), s->ntile * s->nHchunk, s->ered" in sweep and "s->ntile, s->p_pad, s->WPT);" in sweep
    kernels = open(os.path.join(CSRC, "aq_sweep_kernels.h")).read()
    rows = kernels[kernels.index("void aq_k_reduce_rows("):kernels.index("__global__ void aq_k_combine_segment_sums(")]
    for piece in (f"part[{V.QUARTERS}][{V.ROWS}]", f"threadIdx.x & {V.ROWS - 1}", f"blockIdx.x * {V.ROWS} + jl", f"t += {V.QUARTERS}"):
        assert piece in rows, piece
    strided = kernels[kernels.index("void aq_k_elbo_q("):kernels.index("struct AqElboConst")]
    assert "i < nHpart; i += blockDim.x" in strided and "k < v.q; k += blockDim.x" in strided
    assert "for (int j = threadIdx.x; j < v.p; j += blockDim.x)" in kernels[kernels.index("void aq_k_elbo_C("):]
    assert "for (int ch = 0; ch < v.nchunk; ch++) sZ += v.colApart[(size_t)ch * v.q_pad + k];" in kernels


def _keys():
    return sorted({k for k, _, _ in V.inputs()}, key=str)


@pytest.mark.parametrize("key", _keys(), ids=lambda k: "-".join(str(v) for v in k))
def test_no_input_loses_a_column_and_every_trait_differs_from_its_neighbour(key):
    prob = V.problem(key)
    want = {"vec": lambda: key[2:4], "lentz": lambda: (key[1], V.L_Q), "natural": lambda: (75, 20)}[key[0]]()
    assert (prob["p"], prob["q"]) == tuple(want) and prob["X"].shape[1] == prob["p"], "prepare_xy removed a column"
    if key[0] == "natural":
        return
    lh, li = prob["list_hyper"], prob["list_init"]
    sd = V.trait_sd(prob)
    for v in (lh["eta"], lh["kappa"], lh["n0"], li["tau_vb"], sd):
        v = np.asarray(v)
        assert v.shape == (prob["q"],) and np.all(np.abs(np.diff(v)) > 1e-6 * np.abs(v[1:])), "neighbouring traits share a value"
    assert sd.max() / sd.min() > 1e4 if prob["q"] >= 24 else sd.max() / sd.min() > 10
    if key[0] == "vec" and key[4] > 0:
        m = np.isnan(prob["Y"]).sum(axis=0)
        assert m.min() >= 1 and m.max() <= 1024 and abs(m.mean() / prob["n"] - key[4]) < 0.02      # MASK, not the generic kernel
    else:
        assert not np.isnan(prob["Y"]).any()


def _all_cases():
    return sorted(set(_df1_cases() + [c for c, _ in V.S_CASES] + [(V.L_N, p, V.L_Q, 0.0, "plain") for p in V.L_P]))


@pytest.mark.parametrize("case", _all_cases(), ids=V._id)
def test_every_case_is_planned_the_instance_it_asserts(case, hiplib):
    n, p, q, na, form = case
    m = np.isnan(V.problem(("vec", n, p, q, na))["Y"]).sum(axis=0) if na else np.zeros(1, dtype=np.int64)
    st = plan_query(n, p, q, int(m.max()), int(np.minimum(m, n - m).max()), ncu=NCU, total_bytes=MEM, overrides=dict(V.FORMS[form]))
    assert tuple(st[f] for f in V.PLAN_FIELDS) == V.plan_of(case)
    kind = {"plain": (0, 1, 0), "chain3": (0, 1, 3), "parts2": (0, 2, 0), "generic": (2, 1, 0), "masked": (3, 2, 0), "wpt2": (2, 1, 0),
            "wpt4": (2, 1, 0)}[form]
    assert (st["core_kernel"], st["split_parts"], st["chain_segments"]) == kind
    assert bool(st["instance_flags"] & V.MASK) == (na > 0 and st["core_kernel"] == 0)
    if form.startswith("wpt"):       # the forcing rows are TW_FORCED's
        from tests.test_gpu_fallback_instances import TW_FORCED
        assert (n, int(form[3:]), 2048) in {(r[2], r[3], r[4]) for r in TW_FORCED}


@pytest.mark.parametrize("n_parts", sorted(V.H_CUTS))
def test_shards_are_cut_and_planned_as_the_gpu_cases_rely_on(n_parts, hiplib):
    """aq_vb_run_multi reports no per-rank status: the cuts of aq_vb_partition and every shard's plan, from the planner."""
    from atlasqtl_amd.core import vb_partition
    n, p, q, na, form = V.H_SHAPE
    assert not np.isnan(V.problem(("vec", n, p, q, na))["Y"]).any()
    cuts = vb_partition(q, n_parts)
    assert cuts == V.H_CUTS[n_parts]
    assert [(b - a) // V.TILE + ((b - a) % V.TILE > 0) for a, b in cuts] == {2: [9, 10], 3: [6, 6, 7]}[n_parts]      # 19 trait tiles
    for a, b in cuts:
        st = plan_query(n, p, b - a, 0, 0, ncu=NCU, total_bytes=MEM)
        assert tuple(st[f] for f in V.PLAN_FIELDS) == V.H_PLAN == V.plan_of((n, p, b - a, 0.0, "plain")), (a, b)
        assert -(-p // V.PBLOCK) == 3 and b - a < q


def test_natural_lentz_run_is_planned_as_written(hiplib):
    n, p, q = V.L_NATURAL_ARGS
    prob = V.problem(("natural",))
    assert (prob["n"], prob["p"], prob["q"]) == (n, p, q) and V.L_NATURAL_KW == dict(p_act=10, prob_assoc=1.0)
    st = plan_query(n, p, q, 0, 0, ncu=NCU, total_bytes=MEM)
    assert tuple(st[f] for f in V.PLAN_FIELDS) == V.L_NATURAL_PLAN


# ------------------------------------------------------------------------------------------------------------------------------
# the oracle's two forms

def _sharded(key, name, maxit, allreduce=None):
    from oracle import sharded_oracle as S
    scheme, df, anneal = V.SCHEMES[name]
    assert (scheme, df) == ("global_local", 1)
    prob = V.problem(key)
    tr = []
    kw = {} if allreduce is None else dict(allreduce=allreduce)
    out = S.run_sharded(prob["Y"], prob["X"], prob["q"], anneal, 0.1, maxit, prob["list_hyper"], prob["list_init"],
                        thinned_elbo_eval=maxit == V.WHOLE, trace=tr, threads=min(16, os.cpu_count() or 1), **kw)
    return out, np.array([r["lb"] for r in tr if r["lb"] is not None])


DF1_RUNS = [(k, s, m) for k, s, m in V.inputs() if V.SCHEMES[s][:2] == ("global_local", 1)]


def two_form_deviations(key, name, maxit):
    """Every compared quantity of the run as a fraction of its bar, the sharded form against the Gram-space driver."""
    prob = V.problem(key)
    ref, lref, _, _ = V.reference(key, name, maxit, key[0] != "vec")
    alt, lalt = _sharded(key, name, maxit)
    assert alt["it"] == ref["it"] and bool(alt["converged"]) == bool(ref["converged"]) and lalt.shape == lref.shape
    mu_atol = 1e-10 * V.trait_sd(prob)[None, :]
    return dict(elbo=V._rel(lalt, lref) / 1e-9,
                mu_beta_vb=float(np.max(np.abs(alt["mu_beta_vb"] - ref["mu_beta_vb"]) / (mu_atol + 1e-6 * np.abs(ref["mu_beta_vb"])))),
                gam_vb=float(np.max(np.abs(alt["gam_vb"] - ref["gam_vb"]))) / 1e-9,
                theta_vb=V._bar(alt["theta_vb"], ref["theta_vb"], 1e-6, 1e-10), zeta_vb=V._bar(alt["zeta_vb"], ref["zeta_vb"], 1e-6, 1e-10),
                tau_vb=V._rel(alt["tau_vb"], ref["tau_vb"]) / 1e-8, lam2_inv_vb=V._rel(alt["lam2_inv_vb"], ref["lam2_inv_vb"]) / 1e-6)


@pytest.mark.parametrize("key,name,maxit", DF1_RUNS, ids=[f"{'-'.join(str(v) for v in k)}-{s}-{m}" for k, s, m in DF1_RUNS])
def test_the_two_forms_of_the_oracle_agree_within_a_tenth_of_every_bar(key, name, maxit):
    dev = two_form_deviations(key, name, maxit)
    print("\nTWOFORMS", key, name, maxit, " ".join(f"{k}={v:.3e}" for k, v in dev.items()))
    excluded = {(k, s, m) for k, s, m, _, _ in EXCLUDED_RUNS}
    assert (key, name, maxit) not in excluded, "an excluded run is still in the tables of tests/test_gpu_vector_edges.py"
    assert max(dev.values()) <= 0.1, dev


def test_no_row_of_the_edge_table_lost_all_its_runs():
    assert EXCLUDED_RUNS == []      # (nothing to weigh: no run was excluded)


# ------------------------------------------------------------------------------------------------------------------------------
# a slip is visible

def _rolled(key, which):
    from oracle import atlasqtl_oracle as O
    prob = V.problem(key)
    lh = dict(prob["list_hyper"])
    lh[which] = np.roll(np.asarray(lh[which]), 1)
    scheme, df, anneal = V.SCHEMES[V.DF1]
    return O.atlasqtl_global_local_core_(prob["Y"], prob["X"], prob["q"], anneal, df, 0.1, V.SWEEPS, lh, prob["list_init"],
                                         thinned_elbo_eval=False, full_output=True)


@pytest.mark.parametrize("q", V.Q_FORM_Q)
@pytest.mark.parametrize("which", ["eta", "kappa", "n0"])
def test_a_trait_index_that_slips_by_one_is_seen(which, q):
    """eta, kappa or n0 read one trait to the side -- what a q-thread past a block or stride border would do -- moves tau_vb (eta,
    kappa) or zeta_vb (n0) by more than 1000 times its bar after the 14 sweeps of a case."""
    key = ("vec", V.Q_N, V.Q_P, q, 0.0)
    ref = V.reference(key, V.DF1)[0]
    alt = _rolled(key, which)
    tau, zeta = V._rel(alt["tau_vb"], ref["tau_vb"]) / 1e-8, V._bar(alt["zeta_vb"], ref["zeta_vb"], 1e-6, 1e-10)
    # ... and in the traits next to the borders themselves, not only somewhere
    edge = [k for k in (255, 256, 1023, 1024) if k < q]
    tau_e = float(np.max(np.abs(alt["tau_vb"][edge] - ref["tau_vb"][edge]) / np.abs(ref["tau_vb"][edge]))) / 1e-8
    zeta_e = V._bar(alt["zeta_vb"][edge], ref["zeta_vb"][edge], 1e-6, 1e-10)
    print(f"\nSLIP {which} q={q} tau_bar={tau:.3e} zeta_bar={zeta:.3e} at_edges tau_bar={tau_e:.3e} zeta_bar={zeta_e:.3e}")
    assert (zeta_e if which == "n0" else tau_e) > 1000.0 and max(tau, zeta) > 1000.0


@pytest.mark.parametrize("q", V.Q_FORM_Q)
def test_sums_short_of_the_last_trait_or_predictor_are_seen(q):
    """S_gam and T2 short of the last trait's share (what a stride that stops one short leaves out of aq_k_reduce_q_scalars) in
    every sweep of the sharded form moves the ELBO by more than 1000 x 1e-9; so does the last trait left out of the q-sums of the
    ELBO (e_tau_) and the last predictor left out of its p-sum (e_theta_hs_)."""
    from oracle import atlasqtl_oracle as O
    key = ("vec", V.Q_N, V.Q_P, q, 0.0)
    prob = V.problem(key)
    p = prob["p"]
    ref, lref, _, _ = V.reference(key, V.DF1)
    m2 = (ref["mu_beta_vb"] ** 2 + ref["sig2_beta_vb"][None, :]) * ref["gam_vb"]
    share_g = ref["gam_vb"][:, -1].sum() / ref["gam_vb"].sum()
    t2 = ref["tau_vb"] * m2.sum(axis=0)
    share_t = t2[-1] / t2.sum()

    def short(v):
        v = v.copy()
        if v.size == p + 3:
            v[p] *= 1.0 - share_g
            v[p + 1] *= 1.0 - share_t
        return v

    base, lbase = _sharded(key, V.DF1, V.SWEEPS)
    alt, lalt = _sharded(key, V.DF1, V.SWEEPS, allreduce=short)
    moved = V._rel(lalt, lbase)
    lh = prob["list_hyper"]
    e_tau = abs(O.e_tau_(lh["eta"][-1:], ref["eta_vb"][-1:], lh["kappa"][-1:], ref["kappa_vb"][-1:],
                         O.update_log_tau_vb_(ref["eta_vb"][-1:], ref["kappa_vb"][-1:]), ref["tau_vb"][-1:])) / abs(lref[-1])
    Q_app = O.Q_approx_vec(ref["L_vb"][-1:])
    l_s02 = O.update_log_sig2_inv_vb_(ref["nu_s0_vb"], ref["rho_s0_vb"]) + np.log(prob["q"])
    e_theta = abs(O.e_theta_hs_(ref["lam2_inv_vb"][-1:], ref["L_vb"][-1:], l_s02, 0.0, ref["theta_vb"][-1:], Q_app,
                                ref["sig02_inv_vb"] * prob["q"], ref["sig2_theta_vb"][-1:], 1)) / abs(lref[-1])
    print(f"\nSLIP sums q={q} shares={share_g:.3e}/{share_t:.3e} elbo_rel={moved:.3e} e_tau_last={e_tau:.3e} e_theta_last={e_theta:.3e}")
    assert min(moved, e_tau, e_theta) > 1000.0 * 1e-9


# ------------------------------------------------------------------------------------------------------------------------------
# family L

def _lentz_at(x, iters):
    """Q_approx_vec's modified Lentz loop for x > 1, stopped after a given number of iterations (R/utils.R:392-419)."""
    f = C = 1e-30
    D = 0.0
    for j in range(2, iters + 2):
        D = 1.0 / (x + 2 * j - 1 - (j - 1) ** 2 * D)
        C = x + 2 * j - 1 - (j - 1) ** 2 / C
        f *= C * D
    return 1.0 / (x + 1.0 + f)


@pytest.mark.parametrize("p,placement,df", V.L_CASES, ids=[f"p{p}-{pl}-df{df}" for p, pl, df in V.L_CASES])
def test_lentz_placements_land_where_they_say(p, placement, df):
    """L of the oracle's first sweep, from the oracle: the elements above 1 sit in the waves and blocks the placement names, and
    the count is the slowest element's."""
    from oracle import atlasqtl_oracle as O
    key = ("lentz", p, placement, df)
    name = "local-df1" if df == 1 else "df3"
    ref, _, snaps, counts = V.reference(key, name, V.L_SWEEPS, True)
    L = snaps[1]["L_vb"]
    np.testing.assert_allclose(L, V.lentz_L(p, placement, df), rtol=1e-12)
    assert L.max() < 20.0 or df == 1                                # the reference's domain for df > 1
    up = np.flatnonzero(L > 1.0)
    waves, blocks = set(up // 64), set(up // V.PBLOCK)
    nwave = -(-p // 64)
    slow = min(p, 2 * V.PBLOCK) - 1
    if placement == "last":
        assert list(up) == [p - 1] and L[p - 1] == pytest.approx(V.L_SLOW, rel=1e-12)
    elif placement == "wave0":
        assert waves == {0} and up.size == 64
    elif placement == "slow-in-block1":
        assert waves == set(range(nwave)) and blocks == set(range(-(-p // V.PBLOCK)))
        assert slow // V.PBLOCK == 1 and slow // 64 == (4 if p == 257 else 7)        # block 1: its only wave | its last wave
        assert np.flatnonzero(L < 1.5).tolist() == [slow] or set(np.flatnonzero((L > 1.0) & (L < 1.5))) == {slow}
        assert np.all(L[np.setdiff1d(up, [slow])] == pytest.approx(V.L_FAST[df], rel=1e-12))
    elif placement == "none":
        assert up.size == 0 and L.min() > 0.5 and L.max() < 1.0
    else:
        assert up.size == p and L.min() == pytest.approx(V.L_SLOW, rel=1e-12)
    assert counts[0] == V.L_FIRST_COUNT[placement]
    if up.size:
        assert counts[0] == O.Q_approx_vec(np.array([L[up].min()]), return_iters=True)[1]      # the slowest element's own count
    if placement == "slow-in-block1":
        fast_count = O.Q_approx_vec(np.array([V.L_FAST[df]]), return_iters=True)[1]
        assert fast_count == {1: 4, 3: 6}[df] and counts[0] == 24
        # the slow element at the fast elements' count: its lam2_inv_vb (R/atlasqtl_global_local_core.R:254,258) moves by more
        # than 1000 x its bar
        x = float(L[slow])
        right, wrong = _lentz_at(x, 24), _lentz_at(x, fast_count)
        assert right == pytest.approx(float(O.Q_approx_vec(np.array([x]))[0]), rel=1e-14)

        def lam(Q):
            return 1 / (Q * x) - 1 if df == 1 else np.exp(-np.log(3) - np.log(x) + np.log(1 - x * Q) - np.log(Q * (1 + x) - 1)) - 1 / 3

        lam_r, lam_w = lam(right), lam(wrong)
        assert lam_r == pytest.approx(float(snaps[1]["lam2_inv_vb"][slow]), rel=1e-12)
        print(f"\nSLIP lentz p={p} df={df} lam2_inv_rel={abs(lam_w - lam_r) / abs(lam_r):.3e}")
        assert abs(lam_w - lam_r) / abs(lam_r) > 1000.0 * 1e-6


def test_lentz_counts_span_zero_to_twenty_four_and_the_natural_run_has_its_own():
    first = {V.reference(("lentz", p, pl, df), "local-df1" if df == 1 else "df3", V.L_SWEEPS, True)[3][0] for p, pl, df in V.L_CASES}
    assert first == {0, 21, 24}
    every = {c for p, pl, df in V.L_CASES for c in V.reference(("lentz", p, pl, df), "local-df1" if df == 1 else "df3", V.L_SWEEPS, True)[3]}
    natural = V.reference(("natural",), "local-df1", V.L_NATURAL_SWEEPS, True)[3]
    ladder = V.reference(("natural",), V.DF1, V.L_NATURAL_SWEEPS, True)[3]
    assert ladder[:9] == [0] * 9 and min(ladder[9:]) >= 7 and max(ladder[9:]) == 22 and len(set(ladder[9:])) >= 5
    assert min(every) == 0 and max(every | set(natural)) >= 24 and len(every | set(natural)) >= 8
    assert min(natural) > 0 and len(set(natural)) >= 5
    assert max(every | set(natural)) < 64                           # the mask's upper word (counts >= 66) is out of reach


@pytest.mark.parametrize("key,name,maxit", V.inputs(), ids=[f"{'-'.join(str(v) for v in k)}-{s}-{m}" for k, s, m in V.inputs()])
def test_oracle_stays_finite_and_runs_the_sweeps_the_gpu_case_expects(key, name, maxit):
    ref, lref, snaps, counts = V.reference(key, name, maxit, key[0] != "vec")
    for f in ("theta_vb", "zeta_vb", "mu_beta_vb", "gam_vb", "tau_vb", "sig2_theta_vb", "lam2_inv_vb"):
        assert np.all(np.isfinite(ref[f])), f
    if maxit == V.WHOLE:
        assert ref["converged"] and ref["it"] < 100
    else:
        assert ref["it"] == maxit and not ref["converged"] and lref.size >= min(4, maxit)
