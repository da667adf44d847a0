"""GPU: the hand-over of the residual between the chained segments of the look-ahead sweep kernel (aq_core_sweep_la.h, SEG).

Workgroup s * ngroup + k of a chained launch runs SNP segment s of trait group k from the residual that segment s - 1 of the same
group left in global memory.  That residual is the only thing a segment reads that an earlier segment of the same launch wrote,
and it is passed on without a fence: agent-scope stores, each storing wave's s_waitcnt vmcnt(0), a barrier, the flag done[k]; the
consumer polls the flag and loads the residual at agent scope.  A hand-over that fails gives the consumer the residual from
BEFORE the producer's segment: the producer's updates X_b delta_b are lost from the residual the handle carries, while gam and mu
of those blocks are stored all the same.  So the check a stale hand-over breaks is the residual identity
    R in the handle  ==  mis_pat .* (Y - X beta_vb)   recomputed in numpy from the returned beta_vb,
taken after each of the first three sweeps of the annealing ladder, where the updates are largest (a lost block update is of the
size of X_b delta_b, ~1e-2 ... 1 here; rounding leaves ~1e-15).

Shapes (n = 75, the smallest geometry 1 / 1 / 0, so a case takes a fraction of a second):
  p = 38   three SNP blocks, the last of 6 SNPs;   p = 200   13 blocks (segments of 6 / 7, 4 / 5 and 1 blocks)
  chain    2, 3 and one block per segment
  AQ_TT    1 and 2 trait tiles per workgroup, q = 33 (TT = 2: two workgroups, the second with 31 padding traits; TT = 1: three)
  MASK     q = 40, 5 % NA, one tile per workgroup
  q = 128, AQ_TT = 1: eight one-tile workgroups per segment, so the consecutive segments of a group (workgroups k, k + 8, ...) land
           on ONE XCD under the round-robin placement; in every other shape they land on different ones.
Every case asserts the instance it launches from aq_vb_get_status.

Bar of the residual identity, max |R - (Y - X beta_vb)| / rms(Y_k) over all entries and the three sweeps: measured on the parent
commit's library (release / acquire fences) over all cases below, the worst was 1.005e-14 (q = 128, p = 200, chain 2 and 3;
MASK p = 200: 9.4e-15; the p = 38 shapes: 4e-15); ten times that, 1.005e-13, is the bar.  The fence-free hand-over measures the
same figure in every case (the arithmetic is unchanged)."""
import functools

import numpy as np
import pytest

from tests import test_gpu_split_instances as T
from tests.test_gpu_c1_paths import LADDER, NA, _cached_reference, _form_of_run, _segments, _short_of
from tests.test_gpu_split_instances import MASK, SEG, _check, _problem
from tests.test_gpu_unsplit_instances import _assert_unsplit_instance

pytestmark = pytest.mark.gpu

N = 75
P_SMALL, P_LARGE = 38, 200
Q, Q_MASK, Q_SAME_XCD = 33, 40, 128
PER_BLOCK = 32                                     # AQ_CHAIN beyond the block count: one SNP block per segment (the planner caps at 32)
CHAINS = (2, 3, PER_BLOCK)
SWEEPS = (1, 1, 1)                                 # the state is read after 1, 2 and 3 sweeps
PARENT_WORST = 1.005e-14                            # see the module docstring
RESIDUAL_BAR = 10 * PARENT_WORST

# (id, p, q, na, hooks without AQ_CHAIN, TT)
SHAPES = [
    ("tt2-p38", P_SMALL, Q, 0.0, {"AQ_TT": 2}, 2),
    ("tt2-p200", P_LARGE, Q, 0.0, {"AQ_TT": 2}, 2),
    ("tt1-p38", P_SMALL, Q, 0.0, {"AQ_TT": 1, "AQ_LA_NOSPLIT": 1}, 1),
    ("tt1-p200", P_LARGE, Q, 0.0, {"AQ_TT": 1, "AQ_LA_NOSPLIT": 1}, 1),
    ("mask-p38", P_SMALL, Q_MASK, NA, {}, 1),
    ("mask-p200", P_LARGE, Q_MASK, NA, {}, 1),
    ("same-xcd", P_LARGE, Q_SAME_XCD, 0.0, {"AQ_TT": 1, "AQ_LA_NOSPLIT": 1}, 1),
]
CASES = [pytest.param(s, c, id=f"{s[0]}-chain{c if c != PER_BLOCK else 'max'}") for s in SHAPES for c in CHAINS]


@functools.lru_cache(maxsize=None)
def _prob(p, q, na):
    """p = 200 at n = 75: the preparation may drop a column as collinear; the block count is taken from what is left."""
    prob = _problem(N, p, q, na)
    assert prob["q"] == q and prob["p"] > p - 16
    return prob


def _instance(prob, na, tt, chain):
    seg = _segments(prob["p"], chain)
    assert seg > 1
    return ((MASK if na else 0) | SEG, tt, 1, 1, 0, seg)


def _fresh_residual(prob, beta):
    Y = np.array(prob["Y"], dtype=np.float64)
    obs = ~np.isnan(Y)
    Y[~obs] = 0.0
    rms = np.sqrt((Y ** 2).sum(0) / np.maximum(obs.sum(0), 1))
    return obs * (Y - prob["X"] @ beta), rms


def _ladder_states(prob, hooks, instance, monkeypatch):
    """A fresh annealed handle advanced sweep by sweep: (residual, result) after each."""
    from atlasqtl_amd.core import VbRun
    for k, v in hooks.items():
        monkeypatch.setenv(k, str(v))
    run = VbRun(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], LADDER, 0.1, sum(SWEEPS), False, True)
    out = []
    try:
        st = _assert_unsplit_instance(run, *instance)
        for k in SWEEPS:
            run.run_sweeps(k)
            res = run.result(full_output=True)
            out.append(dict(R=run.residual(), beta=np.array(res["beta_vb"], copy=True), gam=np.array(res["gam_vb"], copy=True),
                            mu=np.array(res["mu_beta_vb"], copy=True), it=run.status()["it"]))
    finally:
        run.close()
    return st, out


@pytest.mark.parametrize("shape,chain", CASES)
def test_residual_is_y_minus_x_beta_after_each_ladder_sweep(shape, chain, monkeypatch):
    """The check a stale hand-over breaks, and two runs with the same bits (a stale read depends on timing)."""
    name, p, q, na, hooks, tt = shape
    prob = _prob(p, q, na)
    instance = _instance(prob, na, tt, chain)
    hooks = dict(hooks, AQ_CHAIN=chain)
    st, states = _ladder_states(prob, hooks, instance, monkeypatch)
    _, again = _ladder_states(prob, hooks, instance, monkeypatch)
    assert [s["it"] for s in states] == [1, 2, 3]
    worst = 0.0
    for s in states:
        fresh, rms = _fresh_residual(prob, s["beta"])
        assert np.all(np.isfinite(s["R"]))
        assert float(np.max(np.abs(s["beta"]))) > 1e-3          # the sweeps did move beta: the identity is not 0 == 0
        worst = max(worst, float(np.max(np.abs(s["R"] - fresh) / rms[None, :])))
    print(f"\nHANDOVER {name} chain={chain} S={st['chain_segments']} TT={st['tiles_per_group']} flags={st['instance_flags']} "
          f"residual_dev={worst:.3e} bar={RESIDUAL_BAR:.1e}")
    assert worst <= RESIDUAL_BAR
    for a, b in zip(states, again):
        for f in ("R", "beta", "gam", "mu"):
            assert a[f].tobytes() == b[f].tobytes(), f


@pytest.mark.parametrize("shape,chain", CASES)
def test_chained_run_matches_oracle(shape, chain, monkeypatch):
    """The whole ladder and two sweeps more against the CPU oracle, at the bars of tests/test_gpu_split_instances.py::_check."""
    name, p, q, na, hooks, tt = shape
    prob = _prob(p, q, na)
    for k, v in dict(hooks, AQ_CHAIN=chain).items():
        monkeypatch.setenv(k, str(v))
    reference = _oracle(p, q, na)
    with _form_of_run(LADDER):
        _check("handover-" + name, prob, _instance(prob, na, tt, chain), maxit=_short_of(LADDER),
               assert_instance=_assert_unsplit_instance, reference=reference)


@functools.lru_cache(maxsize=None)
def _oracle(p, q, na):
    """The oracle knows no chain: the chain lengths of a shape share its run.  Nothing writes to it."""
    if (p, q) in ((P_SMALL, Q), (P_SMALL, Q_MASK)):
        return _cached_reference(N, p, q, na, LADDER)          # the run tests/test_gpu_c1_paths.py computes for the same problem
    with _form_of_run(LADDER):
        return T._reference(_prob(p, q, na), _short_of(LADDER))
