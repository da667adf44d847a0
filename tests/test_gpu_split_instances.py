"""GPU: every sample-split instance of the look-ahead sweep kernel and every lane layout of its wide exchange against the CPU
oracle (which works in Gram space, so its cost does not grow with n).

aq_core_sweep_la_kernel is compiled once per residual-tile geometry, each instance with a register allocation and a load
schedule of its own.  The ISA proof (tools/check_isa_operands.py) shows that no instance has a load hazard; only a run shows
that it computes the right numbers.  The families below walk
  a / b  the medium split's geometries 12/11 ... 18/18 (the split-only instances of aq_launch_la1.hip and aq_launch_la1m.hip), forced at small n
         and as the planner picks them for 8448 < n <= 10 240 and for a shard of many traits; and the split exchange inside
         the geometries 1/1 ... 11/11 (the unsplit launches' instances in the same units), forced by the same rule,
  c      the wide split's NT = 1 ... 18 (the WIDE instances of aq_launch_la1w.hip and aq_launch_la1wm.hip),
  d      every part count C = 9 ... 48 of split_exchange_wide (17 lane layouts, some with a dead last chunk),
  e      the geometric limit n = 82 944 = AQ_N_MAX: 48 parts of 18/18, no padding anywhere.
Every case first asserts, from aq_vb_get_status, that the handle launches the instance the case was written for -- a plan that
lands elsewhere fails -- and then holds the run to the parity bars of tests/test_gpu_large_n.py::_check.

The tables are plain data: tests/test_host_logic.py::test_split_instance_ledger_is_complete checks on the CPU that together
they name every compiled split instance and every part count."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MASK, WIDE, SEG = 1, 2, 4        # aq_vb_status.instance_flags
ANNEAL = (1, 2, 10)
SHORT = 12                       # sweeps of a short case: the whole ladder (10) + two sweeps, with an ELBO evaluation after each of them
WHOLE = 1000                     # maxit of a whole run (to convergence)
N_MAX = 48 * 108 * 16            # AQ_N_MAX, aq_core_sweep.h
MIS_MMAX = 1024                  # AQ_MIS_MMAX: more missing samples in a trait hand a medium-n problem to the generic kernel

# --- a. medium split forced with AQ_LA_C = 2 at n = 96 k - 5 (3 k residual tiles per part, the last sample tile ragged):
#        k -> (NT, NT2).  Each runs for complete Y and for 5 % NA.
MEDIUM_FORCED = {23: (12, 11), 24: (12, 12), 25: (13, 12), 26: (13, 13), 27: (14, 13), 28: (14, 14), 29: (15, 14),
                 30: (15, 15), 31: (16, 15), 32: (16, 16), 33: (17, 16), 34: (17, 17), 35: (18, 17), 36: (18, 18)}
MEDIUM_NA = 0.05
MEDIUM_XHELPER_BOTH = (23, 30, 36)     # these also run with the exchange on the helper wave (AQ_LA_XHELPER = 1)
# ... and the same rule below the split-only instances: the instances 1/1 ... 11/11 of the unsplit launches (which
# tests/test_gpu_unsplit_instances.py runs unsplit), here in two parts: the exchange is a runtime path inside them
MEDIUM_FORCED_SMALL = {2: (1, 1), 3: (2, 1), 4: (2, 2), 5: (3, 2), 6: (3, 3), 7: (4, 3), 8: (4, 4), 9: (5, 4), 10: (5, 5), 11: (6, 5),
                       12: (6, 6), 13: (7, 6), 14: (7, 7), 15: (8, 7), 16: (8, 8), 17: (9, 8), 18: (9, 9), 19: (10, 9), 20: (10, 10),
                       21: (11, 10), 22: (11, 11)}
MEDIUM_SMALL_WHOLE = (2, 11, 22)       # whole runs, and the short form with AQ_LA_XHELPER = 1 as well

# --- b. the planner's own choice on 256 CUs: (n, p, q, na, maxit) -> (C, NT, NT2)
MEDIUM_NATURAL = [
    ((8449, 70, 33, 0.0, WHOLE), (8, 12, 11)),
    ((9000, 70, 33, 0.0, WHOLE), (8, 12, 12)),
    ((9000, 70, 33, 0.05, WHOLE), (8, 12, 12)),
    ((9300, 70, 33, 0.0, WHOLE), (8, 13, 12)),
    ((9700, 70, 33, 0.0, WHOLE), (8, 13, 13)),
    ((10240, 70, 33, 0.0, WHOLE), (8, 14, 13)),        # the last n before the wide split
    ((10240, 70, 33, 0.05, WHOLE), (8, 14, 13)),
    ((5000, 40, 1030, 0.0, WHOLE), (3, 18, 17)),       # a shard of many traits: 65 trait tiles, 212 sweeps
]

# --- c. wide split forced with AQ_LA_C = 9 at n = 864 NT - 7 (6 NT residual tiles per part), complete Y and 5 % NA
WIDE_FORCED_C = 9
WIDE_FORCED_NT = tuple(range(1, 19))
WIDE_NA = 0.05

# --- d. every part count at n = 4000 (250 sample tiles dealt out in parts of 6 NT: the last parts of many C hold only
#        padding): NT -> the C that land on it
PARTS_N, PARTS_P, PARTS_Q = 4000, 50, 21
PARTS_NT = {5: (9, 10), 4: (11, 12, 13), 3: tuple(range(14, 21)), 2: tuple(range(21, 42)), 1: tuple(range(42, 49))}
PARTS_NA = 0.08
PARTS_NA_C = (9, 11, 13, 16, 17, 21, 22, 26, 29, 31, 32, 33, 36, 37, 41, 43, 46)   # one C of each of the 17 lane layouts
PARTS_WHOLE_C = (21, 35)          # pc = 6 with nch = 4; a dead last chunk
PARTS_TWICE_C = (10, 30, 45)      # two runs are bit-identical

# --- e. the geometric limit and the way to it: (n, na) -> (C, NT), p = 40, q = 17
LIMIT_P, LIMIT_Q = 40, 17
LIMIT = [((N_MAX, 0.0), (48, 18)), ((N_MAX, 0.03), (48, 18)), ((N_MAX - 1, 0.0), (48, 18)), ((N_MAX - 1, 0.03), (48, 18)),
         ((65000, 0.0), (38, 18))]


def _nt_of_parts(C):
    return next(nt for nt, cs in PARTS_NT.items() if C in cs)


def ledger():
    """What the tables above claim to reach: (medium instances, wide instances, part counts of the wide exchange), the
    instances as (mask, NT, NT2) and (mask, NT)."""
    medium, wide, parts = set(), set(), set()
    for nt, nt2 in list(MEDIUM_FORCED.values()) + list(MEDIUM_FORCED_SMALL.values()):
        medium |= {(0, nt, nt2), (1, nt, nt2)}
    for (n, p, q, na, maxit), (C, nt, nt2) in MEDIUM_NATURAL:
        medium.add((int(na > 0), nt, nt2))
    for nt in WIDE_FORCED_NT:
        wide |= {(0, nt), (1, nt)}
    parts.add(WIDE_FORCED_C)
    for nt, cs in PARTS_NT.items():
        for C in cs:
            wide.add((0, nt))
            parts.add(C)
    for C in PARTS_NA_C:
        wide.add((1, _nt_of_parts(C)))
    for (n, na), (C, nt) in LIMIT:
        wide.add((int(na > 0), nt))
        parts.add(C)
    return medium, wide, parts


def _problem(n, p, q, na=0.0):
    from tests.util import make_problem
    return make_problem(n, p, q, p_act=8, prob_assoc=0.3, na_frac=na, seed=123)


def _max_missing(prob):
    return int(np.isnan(prob["Y"]).sum(axis=0).max())


def _pin_256_cus(monkeypatch):
    """The natural plans of the tables assume 256 CUs.  A larger device is planned as 256 (AQ_NCU); on a smaller one the
    caller derives its expectation from the status.  Returns True when the tables' plan is the one to expect."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if ncu > 256:
        monkeypatch.setenv("AQ_NCU", "256")
    return ncu >= 256


def _assert_instance(run, flags, C, NT, NT2, n_pad=None):
    st = run.status()
    assert st["core_kernel"] == 0
    got = (st["instance_flags"], st["split_parts"], st["tiles_matrix"], st["tiles_matrix2"])
    assert got == (flags, C, NT, NT2), f"planned (flags, C, NT, NT2) = {got}, the case is written for {(flags, C, NT, NT2)}"
    assert st["tiles_per_group"] == 1 and st["chain_segments"] == 0 and st["tiles_recurrence"] == 0
    # the parts' residual tiles: 6 NT in a wide instance, 3 (NT + NT2) otherwise
    assert st["n_pad"] == 16 * 3 * (NT + NT2) * C
    if n_pad is not None:
        assert st["n_pad"] == n_pad
    return st


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _bar(a, b, rtol, atol):
    """Largest |a - b| as a fraction of the bar atol + rtol |b| of assert_allclose."""
    return float(np.max(np.abs(a - b) / (atol + rtol * np.abs(b))))


def _reference(prob, maxit=SHORT):
    """The oracle's run of the problem, as _check holds a handle to it: (result, ELBO trace)."""
    from oracle import atlasqtl_oracle as O
    tr = []
    ref = O.atlasqtl_global_local_core_(prob["Y"], prob["X"], prob["Y"].shape[1], ANNEAL, 1, 0.1, maxit, prob["list_hyper"],
                                        prob["list_init"], thinned_elbo_eval=maxit != SHORT, debug=True, trace=tr, full_output=True)
    return ref, np.array([r["lb"] for r in tr if r["lb"] is not None])


def _check(family, prob, instance, maxit=SHORT, n_pad=None, keep=False, assert_instance=None, reference=None):
    """Create the handle, assert its instance, run, and hold the result to the bars of tests/test_gpu_large_n.py::_check.
    Short cases evaluate the ELBO after every non-annealed sweep (thinned = False), whole runs as the library does by default.
    The observed deviations are printed before they are asserted.  assert_instance: what proves the instance from the handle
    (_assert_instance unless given); reference: _reference(prob, maxit) computed earlier, for cases that share one."""
    from atlasqtl_amd.core import VbRun
    thinned = maxit != SHORT
    q = prob["Y"].shape[1]
    ref, lref = reference if reference is not None else _reference(prob, maxit)
    run = VbRun(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], ANNEAL, 0.1, maxit, thinned, True)
    try:
        if instance is not None and assert_instance is not None:
            assert_instance(run, *instance)
        elif instance is not None:
            _assert_instance(run, *instance, n_pad=n_pad)
        run.run()
        st = run.status()
        got = run.result(full_output=True)
        lgot = run.elbo_trace()[1]
        assert st["it"] == ref["it"]
        if maxit == SHORT:
            assert st["it"] == SHORT and lref.size >= 2
        else:
            assert st["converged"] and ref["converged"]
        assert lgot.shape == lref.shape
        print(f"\nDEV family={family} n={prob['n']} q={q} it={st['it']} flags={st['instance_flags']} C={st['split_parts']} "
              f"NT={st['tiles_matrix']}/{st['tiles_matrix2']}/{st['tiles_recurrence']} TT={st['tiles_per_group']} "
              f"S={st['chain_segments']} elbo_rel={_rel(lgot, lref):.3e} "
              f"mu_bar={_bar(got['mu_beta_vb'], ref['mu_beta_vb'], 1e-6, 1e-10):.3e} "
              f"mu_abs={np.max(np.abs(got['mu_beta_vb'] - ref['mu_beta_vb'])):.3e} "
              f"gam_abs={np.max(np.abs(got['gam_vb'] - ref['gam_vb'])):.3e} "
              f"theta_bar={_bar(got['theta_vb'], ref['theta_vb'], 1e-6, 1e-10):.3e} tau_rel={_rel(got['tau_vb'], ref['tau_vb']):.3e}")
        np.testing.assert_allclose(lgot, lref, rtol=1e-9)
        np.testing.assert_allclose(got["mu_beta_vb"], ref["mu_beta_vb"], rtol=1e-6, atol=1e-10)
        np.testing.assert_allclose(got["gam_vb"], ref["gam_vb"], atol=1e-9)
        np.testing.assert_allclose(got["theta_vb"], ref["theta_vb"], rtol=1e-6, atol=1e-10)
        np.testing.assert_allclose(got["tau_vb"], ref["tau_vb"], rtol=1e-8)
        if keep:
            got["residual"] = run.residual()
        got["status"] = st
        return got
    finally:
        run.close()


# ------------------------------------------------------------------------------------------------------------------------------
# a. medium split, forced

@pytest.mark.parametrize("na", [0.0, MEDIUM_NA])
@pytest.mark.parametrize("k", sorted(MEDIUM_FORCED))
def test_medium_split_every_geometry_matches_oracle(k, na, monkeypatch):
    """The 14 split-only geometries 12/11 ... 18/18 in two parts, complete Y and MASK, exchange on the recurrence wave: whole run."""
    monkeypatch.setenv("AQ_LA_C", "2")
    monkeypatch.setenv("AQ_LA_XHELPER", "0")
    nt, nt2 = MEDIUM_FORCED[k]
    prob = _problem(96 * k - 5, 70, 33, na)
    assert _max_missing(prob) <= MIS_MMAX
    _check("a", prob, (MASK if na else 0, 2, nt, nt2), maxit=WHOLE)


@pytest.mark.parametrize("na", [0.0, MEDIUM_NA])
@pytest.mark.parametrize("k", MEDIUM_XHELPER_BOTH)
def test_medium_split_exchange_on_helper_wave_matches_oracle(k, na, monkeypatch):
    """12/11, 15/15 and 18/18 with the exchange a block ahead on the helper wave: the ladder and two ELBO evaluations."""
    monkeypatch.setenv("AQ_LA_C", "2")
    monkeypatch.setenv("AQ_LA_XHELPER", "1")
    nt, nt2 = MEDIUM_FORCED[k]
    prob = _problem(96 * k - 5, 61, 27, na)
    assert _max_missing(prob) <= MIS_MMAX
    _check("a", prob, (MASK if na else 0, 2, nt, nt2))


@pytest.mark.parametrize("na", [0.0, MEDIUM_NA])
@pytest.mark.parametrize("k", sorted(MEDIUM_FORCED_SMALL))
def test_medium_split_every_small_geometry_matches_oracle(k, na, monkeypatch):
    """The 21 geometries 1/1 ... 11/11 in two parts, complete Y and MASK, exchange on the recurrence wave: the ladder and
    two ELBO evaluations."""
    monkeypatch.setenv("AQ_LA_C", "2")
    monkeypatch.setenv("AQ_LA_XHELPER", "0")
    nt, nt2 = MEDIUM_FORCED_SMALL[k]
    _check("a", _problem(96 * k - 5, 70, 33, na), (MASK if na else 0, 2, nt, nt2))


@pytest.mark.parametrize("na", [0.0, MEDIUM_NA])
@pytest.mark.parametrize("k", MEDIUM_SMALL_WHOLE)
def test_medium_split_small_geometry_whole_run_matches_oracle(k, na, monkeypatch):
    """1/1, 6/5 and 11/11 in two parts to convergence."""
    monkeypatch.setenv("AQ_LA_C", "2")
    monkeypatch.setenv("AQ_LA_XHELPER", "0")
    nt, nt2 = MEDIUM_FORCED_SMALL[k]
    _check("a", _problem(96 * k - 5, 70, 33, na), (MASK if na else 0, 2, nt, nt2), maxit=WHOLE)


@pytest.mark.parametrize("na", [0.0, MEDIUM_NA])
@pytest.mark.parametrize("k", MEDIUM_SMALL_WHOLE)
def test_medium_split_small_geometry_exchange_on_helper_wave_matches_oracle(k, na, monkeypatch):
    """1/1, 6/5 and 11/11 with the exchange a block ahead on the helper wave: the ladder and two ELBO evaluations."""
    monkeypatch.setenv("AQ_LA_C", "2")
    monkeypatch.setenv("AQ_LA_XHELPER", "1")
    nt, nt2 = MEDIUM_FORCED_SMALL[k]
    _check("a", _problem(96 * k - 5, 70, 33, na), (MASK if na else 0, 2, nt, nt2))


# ------------------------------------------------------------------------------------------------------------------------------
# b. medium split, as planned

@pytest.mark.parametrize("shape,plan", MEDIUM_NATURAL, ids=[f"n{s[0]}-q{s[2]}-na{s[3]}" for s, _ in MEDIUM_NATURAL])
def test_medium_split_as_planned_matches_oracle(shape, plan, monkeypatch):
    """What a user gets by default for 8448 < n <= 10 240 (eight parts) and for many traits at moderate n (three parts):
    whole runs."""
    n, p, q, na, maxit = shape
    C, nt, nt2 = plan
    prob = _problem(n, p, q, na)
    mm = _max_missing(prob)
    assert mm <= MIS_MMAX, mm     # beyond it the host rightly plans the generic kernel
    if _pin_256_cus(monkeypatch):
        _check("b", prob, (MASK if na else 0, C, nt, nt2), maxit=maxit)
    else:   # fewer CUs than the tables assume: whatever the planner picks must still be one of the split-only instances
        got = _check("b", prob, None, maxit=maxit)
        st = got["status"]
        assert st["core_kernel"] == 0 and st["instance_flags"] == (MASK if na else 0) and st["tiles_matrix"] >= 12


# ------------------------------------------------------------------------------------------------------------------------------
# c. wide split, every instance

@pytest.mark.parametrize("na", [0.0, WIDE_NA])
@pytest.mark.parametrize("nt", WIDE_FORCED_NT)
def test_wide_split_every_instance_matches_oracle(nt, na, monkeypatch):
    """NT = 1 ... 18 of the wide split in nine parts, complete Y and MASK (from NT = 12 on nine parts are a plan the host could
    choose itself): whole run."""
    monkeypatch.setenv("AQ_LA_C", str(WIDE_FORCED_C))
    prob = _problem(864 * nt - 7, 70, 33, na)
    _check("c", prob, (WIDE | (MASK if na else 0), WIDE_FORCED_C, nt, nt), maxit=WHOLE)


# ------------------------------------------------------------------------------------------------------------------------------
# d. every part count of split_exchange_wide

@pytest.mark.parametrize("C", range(9, 49))
def test_wide_exchange_every_part_count_matches_oracle(C, monkeypatch):
    """Complete Y: the ladder and two ELBO evaluations per part count."""
    monkeypatch.setenv("AQ_LA_C", str(C))
    nt = _nt_of_parts(C)
    _check("d", _problem(PARTS_N, PARTS_P, PARTS_Q), (WIDE, C, nt, nt))


@pytest.mark.parametrize("C", PARTS_NA_C)
def test_wide_exchange_every_lane_layout_with_missing_values_matches_oracle(C, monkeypatch):
    """One part count of each layout (nch chunks of pc parts, the last chunk live or dead), Y with 8 % NA: whole run."""
    monkeypatch.setenv("AQ_LA_C", str(C))
    nt = _nt_of_parts(C)
    _check("d", _problem(PARTS_N, PARTS_P, PARTS_Q, PARTS_NA), (WIDE | MASK, C, nt, nt), maxit=WHOLE)


@pytest.mark.parametrize("C", PARTS_WHOLE_C)
def test_wide_exchange_whole_run_matches_oracle(C, monkeypatch):
    """To convergence with six parts per chunk in four chunks (C = 21) and with a last chunk wholly beyond C (C = 35)."""
    monkeypatch.setenv("AQ_LA_C", str(C))
    nt = _nt_of_parts(C)
    _check("d", _problem(PARTS_N, PARTS_P, PARTS_Q), (WIDE, C, nt, nt), maxit=WHOLE)


@pytest.mark.parametrize("C", PARTS_TWICE_C)
def test_wide_exchange_is_deterministic(C, monkeypatch):
    """Every exchange leaves the same bits in every part, so two runs of one case are bit-identical."""
    monkeypatch.setenv("AQ_LA_C", str(C))
    nt = _nt_of_parts(C)
    prob = _problem(PARTS_N, PARTS_P, PARTS_Q)
    a = _check("d", prob, (WIDE, C, nt, nt))
    b = _check("d", prob, (WIDE, C, nt, nt))
    np.testing.assert_array_equal(a["gam_vb"], b["gam_vb"])
    np.testing.assert_array_equal(a["mu_beta_vb"], b["mu_beta_vb"])


# ------------------------------------------------------------------------------------------------------------------------------
# e. the geometric limit

@pytest.mark.parametrize("maxit", [SHORT, WHOLE], ids=["short", "whole"])
@pytest.mark.parametrize("shape,plan", LIMIT, ids=[f"n{s[0]}-na{s[1]}" for s, _ in LIMIT])
def test_geometric_limit_matches_oracle(shape, plan, maxit, monkeypatch):
    """n = AQ_N_MAX: 48 parts of 18/18 with every tile slot full; one sample less; and n = 65 000 on the way there; each for the
    ladder with two ELBO evaluations and for the whole run.  With 3 % NA a trait misses more than 1024 samples: the long
    global-memory index lists of aq_k_gk_blocks_g.  The residual the handle carries is mis .* (Y - X beta_vb)."""
    n, na = shape
    C, nt = plan
    prob = _problem(n, LIMIT_P, LIMIT_Q, na)
    if na:
        assert _max_missing(prob) > MIS_MMAX
    _pin_256_cus(monkeypatch)     # (with two trait tiles the plan is the same for any count of CUs >= 2 C)
    got = _check("e", prob, (WIDE | (MASK if na else 0), C, nt, nt), n_pad=96 * nt * C, maxit=maxit, keep=True)
    if n >= N_MAX - 1:
        assert got["status"]["n_pad"] == N_MAX
    mis = ~np.isnan(prob["Y"])
    ref = np.where(mis, np.nan_to_num(prob["Y"]) - prob["X"] @ got["beta_vb"], 0.0)
    print(f"DEV family=e residual_abs={np.max(np.abs(got['residual'] - ref)):.3e}")
    np.testing.assert_allclose(got["residual"], ref, atol=1e-9, rtol=0)
