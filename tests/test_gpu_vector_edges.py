"""GPU: the p- and q-vector kernels that run around the sweep in every iteration (aq_sweep_kernels.h) against the CPU oracle at
the edges of their own launch grids.

The sweep kernels' instances are walked by tests/test_gpu_unsplit_instances.py, test_gpu_split_instances.py and
test_gpu_fallback_instances.py -- all at q <= 100 (one complete-Y run at q = 1030 apart) and p <= 500 (tests/test_gpu_bigp.py
apart: look-ahead kernel, df = 1, q = 48), the schemes at p <= 208 and q <= 49.  So the kernels below had only ever had one block
of q-threads, one stride, one block of p-threads (pblk = 1) under any scheme but df = 1, and one chunk of the non-fused pre-pass:
  aq_k_qpre, aq_k_qpost, aq_k_combine_segment_sums(6), aq_k_sum_parts    ceil(q_pad / 256) blocks of 256
  aq_k_reduce_q_scalars, aq_k_elbo_q                                     one block of 1024, stride 1024 over q and over
                                                                         the ntile x nHchunk entries of Hpart
  aq_k_reduce_rows                                                       64 predictors x 4 quarters of the tiles, gb_rows = WPT
  aq_k_pvec_L, aq_k_pvec_finish, aq_k_pvec_global                        pblk = ceil(p / 256) blocks of 256, 3 pblk partial sums
  aq_k_elbo_C                                                            one block of 1024, stride 1024 over p
  aq_k_prepass (+ aq_k_qpost's sum over chunks)                          grid (nHchunk, ntile), 2048 rows per chunk
The families (tables below, plain data; tests/test_vector_coverage_host.py asserts on the CPU that they put a run on either side
of every edge under every form that owns it, that the geometry restated here is the one of aq_vb_create.hip / aq_vb_sweep.hip,
and every case's plan):
  Q  q = 256 | 257, 1024 | 1025, 2049 at p = 96, complete Y and 5 % NA, and at q = 257, 1025 chained segments, two sample parts,
     the generic and the masked kernel; q = 16 400 (1025 trait tiles) for the Hpart stride;
  P  p = 64 | 65, 256 | 257, 513, 1024 | 1025, 2048 | 2049 at q = 24, complete Y and 5 % NA, and at p = 1025, 2049 the generic
     and the masked kernel (the write_AB pre-pass in one and two chunks);
  T  1 ... 5, 8, 9 trait tiles at p = 130; 5 and 9 tiles on the generic kernel's WPT = 2 and 4 instances;
  S  the six schemes other than df = 1 with the ladder at (p, q) = (257, 24), (1025, 24), (96, 257);
  L  the shared Lentz count: five placements of L_j > 1 over the waves and blocks x p = 257, 600 x df = 1, 3, one sweep at a time,
     status()["lentz_iters"] equal to the oracle's count after every sweep; and make_problem(100, 75, 20, p_act=10,
     prob_assoc=1.0), the problem of smoke(), under the ladder and without annealing, where the counts are the run's own;
  H  aq_vb_run_multi in 2 and 3 trait shards at (300, 600, 300), df = 1 and the global scheme with the ladder.
Inputs are tests.util.make_vector_problem: every trait differs from its neighbours in scale, eta, kappa, n0 and initial tau_vb.
Every case of Q, P, T, S and L first proves from aq_vb_status the kernel and instance it was written for and the hooks in effect
(so AQ_TW_WPT, which the status fields cannot show, is known to have been read), then steps ONE handle to 1 sweep, 3 sweeps and
the end (the ladder and the ELBO after each of the sweeps 10 ... 14, thinned_elbo_eval = False; family L: every sweep) and
compares the state at each stop with the oracle's state after the same sweep (one oracle run per input and scheme, cached).  The
first case of every input in table order (TWICE) runs a second handle: the results are bit-identical.  aq_vb_run_multi (H) reports
no per-rank status and takes maxit alone: the cuts are asserted, a handle created on every shard's own columns shows the plan its
rank gets, and the stops are runs with maxit = 1, 3 and 14.

Bars: tests/test_gpu_split_instances.py::_check and tests/test_gpu_schemes.py::_compare -- ELBO 1e-9 relative; mu_beta_vb rtol
1e-6 + atol 1e-10 sd(y_k) (tests/test_gpu_regimes.py); theta_vb, zeta_vb rtol 1e-6 + atol 1e-10; gam_vb 1e-9; tau_vb 1e-8;
sig2_theta_vb and sig02_inv_vb 1e-9 (1e-7 for df = 5, 7); lam2_inv_vb 1e-6 (exactly 1 under the global scheme).  Worst observed
per family: DESIGN.md section 3."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MASK, WIDE, SEG = 1, 2, 4        # aq_vb_status.instance_flags
LADDER = (1, 2, 10)
SWEEPS = 14                      # the ladder (10) + four sweeps with an ELBO evaluation after each
STOPS = (1, 3)                   # states compared on the way to the end
WHOLE = 1000                     # maxit of a whole run (to convergence)
NA = 0.05

# the launch geometry under test (tests/test_vector_coverage_host.py holds these to the source)
QBLOCK, STRIDE, ROWS, QUARTERS, PBLOCK, CHUNK, TILE = 256, 1024, 64, 4, 256, 2048, 16

# name -> (scheme, df, anneal): "local-df1-anneal" and the six of family S (tests/test_gpu_shard_schemes.py::SCHEMES)
SCHEMES = {
    "local-df1-anneal": ("global_local", 1, LADDER),
    "global-anneal": ("global", 1, LADDER),
    "global": ("global", 1, None),
    "df3-anneal": ("global_local", 3, LADDER),
    "df3": ("global_local", 3, None),
    "df5": ("global_local", 5, None),
    "df7-anneal": ("global_local", 7, (2, 3, 5)),
    "local-df1": ("global_local", 1, None),        # family L only: the Lentz loop runs from the first sweep
}
DF1 = "local-df1-anneal"
S_SCHEMES = ("global-anneal", "global", "df3-anneal", "df3", "df5", "df7-anneal")

# hooks by form name
FORMS = {
    "plain": {},
    "chain3": {"AQ_CHAIN": 3},                       # aq_k_combine_segment_sums / _sums6
    "parts2": {"AQ_LA_C": 2},                        # aq_k_sum_parts
    "generic": {"AQ_KERNEL": 2},                     # the non-fused pre-pass: write_AB, rowA, colApart
    "masked": {"AQ_KERNEL": 3, "AQ_MIS_C": 2},       # ... and aq_k_sum_parts over misC parts
    "wpt2": {"AQ_KERNEL": 2, "AQ_TW_WPT": 2},        # gb_rows = 2, 4 (tests/test_gpu_fallback_instances.py::TW_FORCED at n = 2041)
    "wpt4": {"AQ_KERNEL": 2, "AQ_TW_WPT": 4},
}

# --- Q. q edges: (n, p, q, na, form)
Q_N, Q_P = 300, 96
Q_EDGES = (256, 257, 1024, 1025, 2049)
Q_FORM_Q = (257, 1025)
Q_FORM_NA = {"chain3": (0.0, NA), "parts2": (0.0,), "generic": (NA,), "masked": (NA,)}
Q_HPART = (60, 40, 16400, 0.0, "plain")          # 1025 trait tiles: the Hpart loop of aq_k_elbo_q takes a second stride
Q_CASES = ([(Q_N, Q_P, q, na, "plain") for q in Q_EDGES for na in (0.0, NA)]
           + [(Q_N, Q_P, q, na, form) for form, nas in Q_FORM_NA.items() for q in Q_FORM_Q for na in nas] + [Q_HPART])

# --- P. p edges
P_N, P_Q = 300, 24
P_EDGES = (64, 65, 256, 257, 513, 1024, 1025, 2048, 2049)
P_FORM_P = (1025, 2049)                          # one and two chunks of the write_AB pre-pass
P_CASES = ([(P_N, p, P_Q, na, "plain") for p in P_EDGES for na in (0.0, NA)]
           + [(P_N, p, P_Q, NA, form) for form in ("generic", "masked") for p in P_FORM_P])

# --- T. tile quarters of aq_k_reduce_rows: ntile = 1, 2, 3, 4, 5, 8, 9
T_N, T_P, T_WPT_N = 300, 130, 2041
T_Q = (16, 17, 33, 49, 65, 128, 129)
T_WPT_Q = (65, 129)
T_CASES = ([(T_N, T_P, q, 0.0, "plain") for q in T_Q]
           + [(T_WPT_N, T_P, q, NA, form) for form in ("wpt2", "wpt4") for q in T_WPT_Q])
T_WHOLE = [(T_N, T_P, q, 0.0, "plain") for q in T_Q]      # ... and to convergence

# --- S. the schemes at the p and q edges: (p, q)
S_N = 300
S_SHAPES = ((257, 24), (1025, 24), (96, 257))
S_CASES = [((S_N, p, q, 0.0, "plain"), name) for p, q in S_SHAPES for name in S_SCHEMES]

# --- L. the shared Lentz count
L_N, L_Q = 300, 24
L_P = (257, 600)
L_DF = (1, 3)
L_PLACEMENTS = ("last", "wave0", "slow-in-block1", "none", "all")
L_SLOW = 1.05                                    # the oracle's count there is 24
L_FAST = {1: 50.0, 3: 16.0}                      # count 4 | 6; df = 3 keeps L < 20 (domain limits)
L_FIRST_COUNT = {"last": 24, "wave0": 21, "slow-in-block1": 24, "none": 0, "all": 24}   # Q_approx_vec's count in the first sweep
L_SWEEPS = 3
L_CASES = [(p, pl, df) for pl in L_PLACEMENTS for p in L_P for df in L_DF]
# ... and a run whose counts are its own: make_problem(*L_NATURAL_ARGS, **L_NATURAL_KW), the problem of smoke(), for 16 sweeps under
# the ladder (the oracle's counts: 0 while annealed, 22, 7, 15, 18, 14, 16, 10 from sweep 10 on) and without annealing (9 ... 25
# in every sweep)
L_NATURAL_ARGS, L_NATURAL_KW = (100, 75, 20), dict(p_act=10, prob_assoc=1.0)
L_NATURAL_SWEEPS = 16
L_NATURAL_SCHEMES = (DF1, "local-df1")
L_NATURAL_PLAN = (0, 0, 1, 0, 2, 1, 144)

# --- H. trait shards: aq_vb_run_multi deals whole 16-trait tiles out, 19 tiles as 9 + 10 and 6 + 6 + 7.  It reports no per-rank
#        status, so tests/test_vector_coverage_host.py proves every shard's plan (H_PLAN, complete Y) from aq_plan_query; it takes
#        maxit alone, so the states after 1 and 3 sweeps are those of runs with maxit = 1 and 3
H_SHAPE = (300, 600, 300, 0.0, "plain")
H_CUTS = {2: [(0, 144), (144, 300)], 3: [(0, 96), (96, 192), (192, 300)]}
H_CASES = [(parts, name) for parts in sorted(H_CUTS) for name in (DF1, "global-anneal")]

# The plan every case asserts from aq_vb_status, at 256 CUs: (n, form) -> (core_kernel, instance_flags, split_parts,
# chain_segments, tiles_matrix, tiles_matrix2, n_pad) for complete Y; with NA the look-ahead kernel's flags gain MASK.  The same
# for every p and q of the tables (tests/test_vector_coverage_host.py asks aq_plan_query case by case).
PLANS = {
    (300, "plain"): (0, 0, 1, 0, 4, 3, 336),
    (300, "chain3"): (0, SEG, 1, 3, 4, 3, 336),
    (300, "parts2"): (0, 0, 2, 0, 2, 2, 384),
    (300, "generic"): (2, 0, 1, 0, 0, 0, 512),
    (300, "masked"): (3, 0, 2, 0, 2, 0, 512),
    (60, "plain"): (0, 0, 1, 0, 1, 1, 96),
    (2041, "wpt2"): (2, 0, 1, 0, 0, 0, 2048),      # (NE, WPT) = (16, 2) and (8, 4): aq_vb_status reports n_pad alone; the rows are
    (2041, "wpt4"): (2, 0, 1, 0, 0, 0, 2048),      # TW_FORCED's, proven by tests/test_fallback_coverage_host.py from the planner
}
H_PLAN = PLANS[(300, "plain")]                     # every shard of family H


def _first_of_each_input():
    """The cases that also run a second handle for equal bits: the first of every (input, maxit) in table order."""
    seen, out = set(), set()
    rows = [(c, DF1, SWEEPS) for c in Q_CASES + P_CASES + T_CASES] + [(c, DF1, WHOLE) for c in T_WHOLE] + [(c, s, SWEEPS) for c, s in S_CASES]
    for case, name, maxit in rows:
        if (case[:4], maxit) not in seen:
            seen.add((case[:4], maxit))
            out.add((case, name, maxit))
    return out


TWICE = _first_of_each_input()


def plan_of(case):
    n, p, q, na, form = case
    want = PLANS[(n, form)]
    return (want[0], want[1] | (MASK if na > 0 and want[0] == 0 else 0)) + want[2:]


def lentz_L(p, placement, df):
    """L_j of the first sweep for every predictor, by placement.  Waves are 64 predictors, blocks 256."""
    j = np.arange(p)
    low = 0.55 + 0.4 * ((j * 37) % 101) / 101.0              # in (0.5, 1): the series branch
    fast = L_FAST[df]
    L = low.copy()
    if placement == "last":                                   # (i) only j = p - 1, at 1.05
        L[p - 1] = L_SLOW
    elif placement == "wave0":                                # (ii) only in wave 0 of block 0
        L[:64] = np.geomspace(1.3, fast, 64)[(j[:64] * 29) % 64]
    elif placement == "slow-in-block1":                       # (iii) 1.05 in the last wave of block 1, fast ones in every other wave
        slow = min(p, 2 * PBLOCK) - 1
        for w in range(-(-p // 64)):
            if w != slow // 64:
                L[min(64 * w + 3, p - 1)] = fast
        L[slow] = L_SLOW
    elif placement == "all":                                  # (v) every L > 1
        L = np.geomspace(1.2, fast, p)[(j * 101) % p]
        L[p // 2] = L_SLOW
    elif placement != "none":                                 # (iv) every L in (0.5, 1)
        raise ValueError(placement)
    return L


@functools.lru_cache(maxsize=None)
def problem(key):
    """key: ("vec", n, p, q, na) | ("lentz", p, placement, df) | ("natural",)."""
    from tests.util import make_problem, make_vector_problem
    if key[0] == "vec":
        _, n, p, q, na = key
        return make_vector_problem(n, p, q, na_frac=na)
    if key[0] == "lentz":
        _, p, placement, df = key
        return make_vector_problem(L_N, p, L_Q, theta=(np.arange(p), lentz_L(p, placement, df)), df=df)
    if key == ("natural",):
        return make_problem(*L_NATURAL_ARGS, **L_NATURAL_KW)
    raise ValueError(key)


def inputs():
    """Every (input key, scheme, maxit) the file holds to the oracle, for tests/test_vector_coverage_host.py."""
    out = [(("vec",) + c[:4], DF1, SWEEPS) for c in Q_CASES + P_CASES + T_CASES]
    out += [(("vec",) + c[:4], DF1, WHOLE) for c in T_WHOLE]
    out += [(("vec",) + c[:4], name, SWEEPS) for c, name in S_CASES]
    out += [(("lentz", p, pl, df), "local-df1" if df == 1 else "df3", L_SWEEPS) for p, pl, df in L_CASES]
    out += [(("natural",), name, L_NATURAL_SWEEPS) for name in L_NATURAL_SCHEMES]
    out += [(("vec",) + H_SHAPE[:4], name, SWEEPS) for _, name in H_CASES]
    return sorted(set(out), key=str)


@functools.lru_cache(maxsize=None)
def reference(key, name, maxit=SWEEPS, every=False):
    """The oracle's run: (result, ELBO trace, {sweep: state after it}, per-sweep Lentz counts).  Computed once per (input,
    scheme); left unchanged.  every: a state after every sweep (family L)."""
    import os
    from oracle import atlasqtl_oracle as O
    scheme, df, anneal = SCHEMES[name]
    prob = problem(key)
    li = prob["list_init"]
    if scheme == "global":           # that core has no local scales
        li = dict({k: v for k, v in li.items() if k != "sig2_theta_vb"}, sig2_theta_vb=np.ones(prob["p"]))
    tr, snaps = [], dict.fromkeys(range(1, maxit + 1) if every else STOPS)
    ref = O.atlasqtl_global_local_core_(prob["Y"], prob["X"], prob["q"], anneal, df, 0.1, maxit, prob["list_hyper"], li,
                                        thinned_elbo_eval=maxit == WHOLE, trace=tr, full_output=True, scheme=scheme, snapshots=snaps,
                                        threads=min(16, os.cpu_count() or 1))
    return ref, np.array([r["lb"] for r in tr if r["lb"] is not None]), snaps, [r["lentz_iters"] for r in tr]


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _bar(a, b, rtol, atol):
    """Largest |a - b| as a fraction of the bar atol + rtol |b| of assert_allclose."""
    return float(np.max(np.abs(a - b) / (atol + rtol * np.abs(b))))


def trait_sd(prob):
    return np.nanstd(prob["Y"], axis=0, ddof=1)


def hold_state(tag, prob, name, ref, got):
    """The fields of a state (after any sweep) at the file's bars; the observed deviations are printed before they are asserted.
    ref, got: mu_beta_vb, gam_vb, theta_vb, zeta_vb, tau_vb, lam2_inv_vb, sig2_theta_vb, sig02_inv_vb."""
    scheme, df, anneal = SCHEMES[name]
    rtol_scale = 1e-9 if df in (1, 3) else 1e-7      # df = 5, 7: the reason is recorded in tests/test_gpu_schemes.py
    mu_atol = 1e-10 * trait_sd(prob)[None, :]
    dev = dict(mu_bar=float(np.max(np.abs(got["mu_beta_vb"] - ref["mu_beta_vb"]) / (mu_atol + 1e-6 * np.abs(ref["mu_beta_vb"])))),
               gam_abs=float(np.max(np.abs(got["gam_vb"] - ref["gam_vb"]))),
               theta_bar=_bar(got["theta_vb"], ref["theta_vb"], 1e-6, 1e-10), zeta_bar=_bar(got["zeta_vb"], ref["zeta_vb"], 1e-6, 1e-10),
               tau_rel=_rel(got["tau_vb"], ref["tau_vb"]), sig2_theta_rel=_rel(got["sig2_theta_vb"], ref["sig2_theta_vb"]),
               sig02_inv_rel=abs(got["sig02_inv_vb"] - ref["sig02_inv_vb"]) / abs(ref["sig02_inv_vb"]),
               lam2_inv_rel=_rel(got["lam2_inv_vb"], ref["lam2_inv_vb"]))
    print(f"\nDEV {tag} scheme={name} " + " ".join(f"{k}={v:.3e}" for k, v in dev.items()))
    for f in ("mu_beta_vb", "gam_vb", "theta_vb", "zeta_vb", "tau_vb", "lam2_inv_vb", "sig2_theta_vb"):
        assert np.all(np.isfinite(ref[f])) and got[f].shape == ref[f].shape, f
    assert dev["mu_bar"] <= 1.0, dev
    np.testing.assert_allclose(got["gam_vb"], ref["gam_vb"], atol=1e-9, rtol=0)
    np.testing.assert_allclose(got["theta_vb"], ref["theta_vb"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(got["zeta_vb"], ref["zeta_vb"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(got["tau_vb"], ref["tau_vb"], rtol=1e-8)
    np.testing.assert_allclose(got["sig2_theta_vb"], ref["sig2_theta_vb"], rtol=rtol_scale)
    np.testing.assert_allclose(got["sig02_inv_vb"], ref["sig02_inv_vb"], rtol=rtol_scale)
    if scheme == "global":
        np.testing.assert_array_equal(got["lam2_inv_vb"], 1.0)
    else:
        np.testing.assert_allclose(got["lam2_inv_vb"], ref["lam2_inv_vb"], rtol=1e-6)
    return dev


def hold_end(tag, prob, name, ref, lref, got, lgot):
    """The end of a run: it, converged, the ELBO trace and the state."""
    assert got["it"] == ref["it"] and bool(got["converged"]) == bool(ref["converged"]), (got["it"], ref["it"])
    assert lgot.shape == lref.shape and lref.size >= 2
    print(f"\nDEV {tag} scheme={name} it={got['it']} elbo_rel={_rel(lgot, lref):.3e}")
    np.testing.assert_allclose(lgot, lref, rtol=1e-9)
    return hold_state(tag, prob, name, ref, got)


PLAN_FIELDS = ("core_kernel", "instance_flags", "split_parts", "chain_segments", "tiles_matrix", "tiles_matrix2", "n_pad")


def assert_plan(st, want):
    got = tuple(st[k] for k in PLAN_FIELDS)
    assert got == tuple(want), f"planned {dict(zip(PLAN_FIELDS, got))}, the case is written for {dict(zip(PLAN_FIELDS, want))} " \
                               f"(hooks in effect: {st['overrides']!r})"


def hooks_in_effect(st):
    """The hooks the handle's plan consulted and found set (aq_vb_get_overrides), AQ_NCU of _pin_256_cus apart.  aq_vb_status
    cannot tell the generic kernel's (32, 1), (16, 2) and (8, 4) apart (n_pad = 2048 for all): AQ_TW_WPT = 2, 4 is proven here."""
    return {h for h in st["overrides"].split() if not h.startswith("AQ_NCU=")}


def _state(run):
    st = run.status()
    return dict(run.result(full_output=True), it=st["it"], converged=st["converged"], sig02_inv_vb=st["sig02_inv_vb"],
                lentz_iters=st["lentz_iters"])


def _handle(prob, name, maxit):
    from atlasqtl_amd.core import VbRun
    scheme, df, anneal = SCHEMES[name]
    return VbRun(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], anneal, 0.1, maxit, maxit == WHOLE, True, scheme=scheme, df=df)


def _setenv(monkeypatch, form):
    from tests.test_gpu_split_instances import _pin_256_cus
    assert _pin_256_cus(monkeypatch), "the plans of this file are those of 256 CUs"
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, str(v))


def check(family, case, name, monkeypatch, maxit=SWEEPS):
    """One case: the plan, then one handle stepped to every stop and to the end, each state against the oracle's."""
    n, p, q, na, form = case
    key = ("vec", n, p, q, na)
    prob = problem(key)
    assert (prob["p"], prob["q"]) == (p, q)
    _setenv(monkeypatch, form)
    ref, lref, snaps, _ = reference(key, name, maxit)
    tag = f"family={family} n={n} p={p} q={q} na={na} form={form}"
    run = _handle(prob, name, maxit)
    try:
        st = run.status()
        assert_plan(st, plan_of(case))
        assert hooks_in_effect(st) == {f"{k}={v}" for k, v in FORMS[form].items()}, st["overrides"]     # no hook was ignored
        done = 0
        if maxit != WHOLE:
            assert ref["it"] > STOPS[-1]
            for stop in STOPS:
                run.run_sweeps(stop - done)
                done = stop
                got = _state(run)
                assert got["it"] == stop
                hold_state(f"{tag} sweep={stop}", prob, name, snaps[stop], got)
            run.run_sweeps(maxit - done)
            assert ref["it"] == maxit and lref.size >= 4
        else:
            run.run()
            assert ref["converged"]
        end = _state(run)
        hold_end(f"{tag} end", prob, name, ref, lref, end, run.elbo_trace()[1])
    finally:
        run.close()
    if (case, name, maxit) in TWICE:            # the first case of every input: a second handle, run in one go, gives the same bits
        run = _handle(prob, name, maxit)
        try:
            run.run()
            again = _state(run)
        finally:
            run.close()
        assert again["it"] == end["it"]
        for f in ("gam_vb", "mu_beta_vb", "theta_vb", "zeta_vb", "tau_vb", "lam2_inv_vb", "sig2_theta_vb", "sig02_inv_vb"):
            np.testing.assert_array_equal(again[f], end[f], err_msg=f)
    return end


def _id(case):
    n, p, q, na, form = case
    return f"n{n}-p{p}-q{q}-na{na}-{form}"


# ------------------------------------------------------------------------------------------------------------------------------
# Q, P, T: df = 1 with the ladder

@pytest.mark.parametrize("case", Q_CASES, ids=_id)
def test_q_edges_match_oracle(case, monkeypatch):
    """A second block of aq_k_qpre / aq_k_qpost / the combine kernels at q = 257, a second and third stride of
    aq_k_reduce_q_scalars / aq_k_elbo_q at q = 1025 and 2049, in the complete-Y and the v.na forms."""
    check("Q", case, DF1, monkeypatch)


@pytest.mark.parametrize("case", P_CASES, ids=_id)
def test_p_edges_match_oracle(case, monkeypatch):
    """A second block of aq_k_reduce_rows at p = 65, of the aq_k_pvec kernels at p = 257, a third at 513, a second and third
    stride of aq_k_elbo_C at p = 1025 and 2049, a second chunk of aq_k_prepass at p = 2049."""
    check("P", case, DF1, monkeypatch)


@pytest.mark.parametrize("case", T_CASES, ids=_id)
def test_tile_quarters_match_oracle(case, monkeypatch):
    """aq_k_reduce_rows deals the trait tiles to four quarters: 1 ... 4 tiles leave quarters empty, 5 gives the first a second
    tile, 8 | 9 a second and third; with the generic kernel's WPT = 2, 4 every tile has 2, 4 rows of rowGB."""
    check("T", case, DF1, monkeypatch)


@pytest.mark.parametrize("case", T_WHOLE, ids=_id)
def test_tile_quarters_whole_run_matches_oracle(case, monkeypatch):
    check("T", case, DF1, monkeypatch, maxit=WHOLE)


# ------------------------------------------------------------------------------------------------------------------------------
# S: the other schemes

@pytest.mark.parametrize("case,name", S_CASES, ids=[f"{_id(c)}-{s}" for c, s in S_CASES])
def test_schemes_at_the_edges_match_oracle(case, name, monkeypatch):
    """aq_k_pvec_global, the df = 3, 5, 7 branches of aq_k_pvec_finish (closed form, aq_hs_integral, annealed Kummer update) and
    of aq_k_elbo_C with a second block (p = 257), a second stride (p = 1025) and a second block of q-threads (q = 257)."""
    check("S", case, name, monkeypatch)


# ------------------------------------------------------------------------------------------------------------------------------
# L: the shared Lentz count

def _lentz(key, name, sweeps, tag, monkeypatch, plan):
    prob = problem(key)
    _setenv(monkeypatch, "plain")
    ref, lref, snaps, counts = reference(key, name, sweeps, True)
    assert ref["it"] == sweeps == len(counts)
    run = _handle(prob, name, sweeps)
    got_counts = []
    try:
        st = run.status()
        assert hooks_in_effect(st) == set(), st["overrides"]
        assert_plan(st, plan)
        for it in range(1, sweeps + 1):
            run.run_sweeps(1)
            got = _state(run)
            assert got["it"] == it
            got_counts.append(got["lentz_iters"])
            print(f"\nLENTZ {tag} sweep={it} device={got['lentz_iters']} oracle={counts[it - 1]}")
            assert got["lentz_iters"] == counts[it - 1], (it, got_counts, counts)
            hold_state(f"family=L {tag} sweep={it}", prob, name, snaps[it], got)
        end = _state(run)
        hold_end(f"family=L {tag} end", prob, name, ref, lref, end, run.elbo_trace()[1])
    finally:
        run.close()
    run = _handle(prob, name, sweeps)           # a second handle, run in one go: the same count and the same bits
    try:
        run.run()
        again = _state(run)
    finally:
        run.close()
    assert (again["it"], again["lentz_iters"]) == (end["it"], end["lentz_iters"])
    for f in ("gam_vb", "mu_beta_vb", "theta_vb", "zeta_vb", "tau_vb", "lam2_inv_vb", "sig2_theta_vb", "sig02_inv_vb"):
        np.testing.assert_array_equal(again[f], end[f], err_msg=f)
    return counts


@pytest.mark.parametrize("p,placement,df", L_CASES, ids=[f"p{p}-{pl}-df{df}" for p, pl, df in L_CASES])
def test_shared_lentz_count_equals_the_oracles(p, placement, df, monkeypatch):
    """The AND over lanes, waves (one atomicAnd each) and blocks of the 128-bit convergence mask gives the iteration at which
    the SLOWEST element with L_j > 1 stops, wherever it sits: lentz_iters after each of three sweeps equals the oracle's count,
    and lam2_inv_vb, theta_vb, sig2_theta_vb (every element evaluated at that count) are within the bars."""
    key = ("lentz", p, placement, df)
    counts = _lentz(key, "local-df1" if df == 1 else "df3", L_SWEEPS, f"p={p} placement={placement} df={df}", monkeypatch,
                    plan_of((L_N, p, L_Q, 0.0, "plain")))
    assert counts[0] == L_FIRST_COUNT[placement]


@pytest.mark.parametrize("name", L_NATURAL_SCHEMES)
def test_shared_lentz_count_of_a_natural_run_equals_the_oracles(name, monkeypatch):
    """make_problem(100, 75, 20, p_act=10, prob_assoc=1.0), 16 sweeps: the counts are the run's own -- under the ladder 0 while
    annealed and 7 ... 22 from sweep 10 on, without annealing 9 ... 25 in every sweep."""
    counts = _lentz(("natural",), name, L_NATURAL_SWEEPS, f"natural {name}", monkeypatch, L_NATURAL_PLAN)
    first = SCHEMES[name][2][2] if SCHEMES[name][2] else 1        # the first sweep without annealing
    assert not any(counts[:first - 1]) and min(counts[first - 1:]) > 0 and len(set(counts[first - 1:])) >= 5


# ------------------------------------------------------------------------------------------------------------------------------
# H: trait shards

@functools.lru_cache(maxsize=None)
def _single(name):
    import atlasqtl_amd as A
    scheme, df, anneal = SCHEMES[name]
    prob = problem(("vec",) + H_SHAPE[:4])
    return A.atlasqtl_global_local_core_(prob["Y"], prob["X"], prob["q"], anneal, df, 0.1, SWEEPS, 0, prob["list_hyper"], prob["list_init"],
                                         full_output=True, debug=True, scheme=scheme, thinned_elbo_eval=False)


@pytest.mark.parametrize("n_parts,name", H_CASES, ids=[f"{n}-{s}" for n, s in H_CASES])
def test_trait_shards_at_the_edges_match_oracle_and_single_handle(n_parts, name, monkeypatch):
    """(300, 600, 300) in 2 and 3 shards: 19 trait tiles dealt out as 9 + 10 and 6 + 6 + 7, three blocks of p-threads, every shard
    with a q_total that is not its own q.  aq_vb_run_multi reports no per-rank status: a handle created on every shard's own
    columns shows the plan its rank gets (and tests/test_vector_coverage_host.py asks aq_plan_query).  It takes no sweep budget
    either: the states after 1 and 3 sweeps are those of runs with maxit = 1 and 3."""
    from atlasqtl_amd.core import VbRun, run_multi, vb_partition
    from tests.test_gpu_multi import _same
    from tests.util import shard_lists
    _setenv(monkeypatch, "plain")
    scheme, df, anneal = SCHEMES[name]
    key = ("vec",) + H_SHAPE[:4]
    prob = problem(key)
    cuts = vb_partition(prob["q"], n_parts)
    assert cuts == H_CUTS[n_parts]
    for k0, k1 in cuts:
        lh, li = shard_lists(prob["list_hyper"], prob["list_init"], k0, k1)
        run = VbRun(np.asfortranarray(prob["Y"][:, k0:k1]), prob["X"], lh, li, anneal, 0.1, SWEEPS, False, True, q_total=prob["q"],
                    trait_offset=k0, scheme=scheme, df=df)
        try:
            st = run.status()
            assert_plan(st, H_PLAN)
            assert hooks_in_effect(st) == set(), st["overrides"]
        finally:
            run.close()
    ref, lref, snaps, _ = reference(key, name)

    def sharded(maxit=SWEEPS):
        return run_multi(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], anneal, 0.1, maxit, n_gpus=n_parts,
                         devices=[0] * n_parts, transport=1, thinned_elbo_eval=False, scheme=scheme, df=df)

    for stop in STOPS:
        got = sharded(stop)
        assert got["it"] == stop and not got["converged"]
        hold_state(f"family=H parts={n_parts} sweep={stop}", prob, name, snaps[stop], got)
    got = sharded()
    hold_end(f"family=H parts={n_parts} end", prob, name, ref, lref, got, got["elbo_trace"][1])
    _same(got, _single(name))
    again = sharded()                           # the payloads are reduced in rank order: the same bits
    for f in ("gam_vb", "mu_beta_vb", "theta_vb", "zeta_vb", "tau_vb", "lam2_inv_vb", "sig2_theta_vb", "sig02_inv_vb"):
        np.testing.assert_array_equal(again[f], got[f], err_msg=f)
    np.testing.assert_array_equal(again["elbo_trace"][1], got["elbo_trace"][1])
