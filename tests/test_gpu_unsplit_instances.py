"""GPU: every unsplit instance (n <= 1056, one workgroup per trait group) of the look-ahead sweep kernel against the CPU oracle.

aq_core_sweep_la_kernel is compiled once per residual-tile geometry NT / NT2 / NT3 (tiles of matrix waves 0-2, of matrix waves
4-6, of the recurrence wave), for one or two trait tiles per workgroup (TT), for complete Y and for Y with missing values
(MASK), each plain and chained (SEG): aq_launch_la1.hip, aq_launch_la2.hip, aq_launch_la1m.hip.  This is the kernel bench.py
measures.  The families below walk
  U1  TT = 1, complete Y, no tile on the recurrence wave: 1/1 ... 11/11,
  U2  TT = 1, complete Y, three, six or nine tiles on the recurrence wave, NT = 8 ... 11,
  U3  TT = 2: 1/1 ... 7/7, and from NT = 8 on the recurrence wave's three, six or nine tiles,
  U4  MASK: 1/1 ... 11/11,
each geometry plain (AQ_CHAIN = 0) and in three chained segments (AQ_CHAIN = 3).  Every case first asserts, from
aq_vb_get_status, that the handle launches the instance the case was written for -- a plan that lands elsewhere fails -- and
then holds the run to the parity bars of tests/test_gpu_split_instances.py::_check.

Inputs: make_problem(n, 70, 33): five SNP blocks, the last of 6 SNPs (segments of 2, 2 and 1 blocks); three trait tiles, the
last of 1 trait (with TT = 2 q is padded to 64: the second workgroup's second tile is all padding).  n follows one rule: with
T = 3 (NT + NT2) + NT3 tiles in the geometry, n = min(16 T - 5, 1051), so that every tile of every wave holds live samples and
the last live tile holds 11 of 16; a wave that drops, repeats or mis-offsets a tile changes S' and misses the ELBO bar.  At
n = 1051 (66 tiles) the geometries of 69 tiles keep their last three as padding.

The tables are plain data: tests/test_unsplit_coverage_host.py checks on the CPU that the planner gives every row the instance
it names, that together the rows name every compiled unsplit instance but the four of UNREACHABLE, and which tiles hold live
samples."""
import functools
from collections import namedtuple

import numpy as np
import pytest

from tests.test_gpu_split_instances import MASK, SEG, SHORT, WHOLE, _check, _problem, _reference

pytestmark = pytest.mark.gpu

P, Q = 70, 33
N_UNSPLIT = 1056                 # the largest n one workgroup holds
N_TOP = 1051                     # 66 tiles, the last with 11 of 16 samples
NA = 0.05                        # U4
CHAIN = (0, 3)                   # AQ_CHAIN of the plain and of the chained case

# NT + NT2 = k -> (NT, NT2): the pairs of the instance set, NT = 1 ... 11 (aq_plan_const.h)
PAIRS = {2: (1, 1), 3: (2, 1), 4: (2, 2), 5: (3, 2), 6: (3, 3), 7: (4, 3), 8: (4, 4), 9: (5, 4), 10: (5, 5), 11: (6, 5), 12: (6, 6),
         13: (7, 6), 14: (7, 7), 15: (8, 7), 16: (8, 8), 17: (9, 8), 18: (9, 9), 19: (10, 9), 20: (10, 10), 21: (11, 10), 22: (11, 11)}
# (NT, NT2, NT3) with tiles on the recurrence wave: the forms 3, 6, 9 of aq_launch_la1.hip; with TT = 2 aq_la_nt3 (three tiles for NT / NT,
# six for NT / NT - 1) and NT / NT / 9 of aq_launch_la2.hip.  AQ_NT3 = NT3 selects each.  (11/11/9 is not here: UNREACHABLE.)
RECURRENCE = [(8, 8, 3), (8, 7, 6), (8, 8, 9), (9, 9, 3), (9, 8, 6), (9, 9, 9), (10, 10, 3), (10, 9, 6), (10, 10, 9), (11, 11, 3), (11, 10, 6)]
U3_PLAIN_K = tuple(range(2, 15))     # TT = 2 without tiles on the recurrence wave: NT <= 7

# hooks of a family, AQ_CHAIN and AQ_NT3 apart.  AQ_LA_NOSPLIT: with three trait tiles the planner otherwise shares the samples
# among idle CUs from n of about 800 on.
HOOKS = {"U1": {"AQ_TT": 1, "AQ_LA_NOSPLIT": 1}, "U2": {"AQ_TT": 1, "AQ_LA_NOSPLIT": 1}, "U3": {"AQ_TT": 2}, "U4": {}}

# compiled, and out of the planner's reach: (mask, TT, NT, NT2, NT3, seg) -> why
_WHY_11_11_9 = ("11/11/9 holds 75 tiles; 10/10/9 already holds 69 and an unsplit problem has at most 66 (n <= 1056); the medium "
                "split never takes tiles on the recurrence wave (aq_la_fit with nt_max = 18) and has one trait tile per workgroup")
UNREACHABLE = {(0, 1, 11, 11, 9, 0): _WHY_11_11_9, (0, 1, 11, 11, 9, 1): _WHY_11_11_9,
               (0, 2, 11, 11, 9, 0): _WHY_11_11_9, (0, 2, 11, 11, 9, 1): _WHY_11_11_9}
# (TT, NT, NT2, NT3) whose recurrence-wave tiles start at tile 66, past the last tile an unsplit n can fill: they run all the
# same -- the padding must stay zero and add nothing to S'
RECURRENCE_TILES_ALL_PADDING = {(1, 11, 11, 3), (2, 11, 11, 3)}

# whole runs (to convergence): the smallest and the largest geometry of each family, and everything with tiles on the
# recurrence wave of a one-tile workgroup or nine of them on a two-tile one (the tightest register budgets)
U3_LARGEST = (11, 11, 3)
# two runs are bit-identical: (family, NT, NT2, NT3), chained
TWICE = [("U1", 11, 11, 0), ("U2", 10, 10, 9), ("U3", 11, 11, 3), ("U4", 11, 11, 0)]

Row = namedtuple("Row", "family mask TT NT NT2 NT3 n na hooks whole")


def n_of(NT, NT2, NT3):
    return min(16 * (3 * (NT + NT2) + NT3) - 5, N_TOP)


def rows():
    """The geometries of the four families (each runs with both AQ_CHAIN of CHAIN): 21 + 11 + 24 + 21."""
    out = []
    for k, (nt, nt2) in sorted(PAIRS.items()):
        out.append(Row("U1", 0, 1, nt, nt2, 0, n_of(nt, nt2, 0), 0.0, dict(HOOKS["U1"], AQ_NT3=0), k in (2, 22)))
    for nt, nt2, nt3 in RECURRENCE:
        out.append(Row("U2", 0, 1, nt, nt2, nt3, n_of(nt, nt2, nt3), 0.0, dict(HOOKS["U2"], AQ_NT3=nt3), True))
    for k in U3_PLAIN_K:
        nt, nt2 = PAIRS[k]
        out.append(Row("U3", 0, 2, nt, nt2, 0, n_of(nt, nt2, 0), 0.0, dict(HOOKS["U3"]), k == 2))
    for nt, nt2, nt3 in RECURRENCE:
        out.append(Row("U3", 0, 2, nt, nt2, nt3, n_of(nt, nt2, nt3), 0.0, dict(HOOKS["U3"], AQ_NT3=nt3),
                       nt3 == 9 or (nt, nt2, nt3) == U3_LARGEST))
    for k, (nt, nt2) in sorted(PAIRS.items()):
        out.append(Row("U4", 1, 1, nt, nt2, 0, n_of(nt, nt2, 0), NA, dict(HOOKS["U4"]), k in (2, 22)))
    return out


def hooks_of(row, chain):
    return dict(row.hooks, AQ_CHAIN=chain)


def instance_of(row, chain):
    """(instance_flags, tiles_per_group, tiles_matrix, tiles_matrix2, tiles_recurrence, chain_segments) of aq_vb_status."""
    return ((MASK if row.mask else 0) | (SEG if chain > 1 else 0), row.TT, row.NT, row.NT2, row.NT3, chain if chain > 1 else 0)


def n_pad_of(row):
    return 16 * (3 * (row.NT + row.NT2) + row.NT3)


def ledger():
    """What the tables claim to reach: the kernels as (mask, TT, NT, NT2, NT3, seg)."""
    return {(r.mask, r.TT, r.NT, r.NT2, r.NT3, int(c > 1)) for r in rows() for c in CHAIN}


def _id(row):
    return f"{row.family}-{row.NT}.{row.NT2}.{row.NT3}"


ROWS = rows()
WHOLE_ROWS = [r for r in ROWS if r.whole]


def _assert_unsplit_instance(run, flags, TT, NT, NT2, NT3, segments):
    st = run.status()
    assert st["core_kernel"] == 0 and st["split_parts"] == 1, st
    got = (st["instance_flags"], st["tiles_per_group"], st["tiles_matrix"], st["tiles_matrix2"], st["tiles_recurrence"], st["chain_segments"])
    want = (flags, TT, NT, NT2, NT3, segments)
    assert got == want, f"planned (flags, TT, NT, NT2, NT3, segments) = {got}, the case is written for {want}"
    assert st["n_pad"] == 16 * (3 * (NT + NT2) + NT3)
    return st


@functools.lru_cache(maxsize=None)
def _cached_problem(n, na):
    prob = _problem(n, P, Q, na)
    assert prob["p"] == P and prob["q"] == Q       # five SNP blocks, three trait tiles: nothing was dropped as constant or collinear
    return prob


@functools.lru_cache(maxsize=None)
def _cached_reference(n, na, maxit):
    """The oracle knows no geometry: the TT, NT3 and chain variants of one n share its run.  Nothing writes to it."""
    return _reference(_cached_problem(n, na), maxit)


def _run(row, chain, maxit, monkeypatch):
    for k, v in hooks_of(row, chain).items():
        monkeypatch.setenv(k, str(v))
    assert row.n <= N_UNSPLIT
    return _check(row.family, _cached_problem(row.n, row.na), instance_of(row, chain), maxit=maxit,
                  assert_instance=_assert_unsplit_instance, reference=_cached_reference(row.n, row.na, maxit))


@pytest.mark.parametrize("chain", CHAIN, ids=["plain", "chained"])
@pytest.mark.parametrize("row", ROWS, ids=_id)
def test_unsplit_instance_matches_oracle(row, chain, monkeypatch):
    """Every reachable unsplit kernel, 154 of them: the whole ladder and two sweeps, with an ELBO evaluation after each
    unannealed sweep."""
    _run(row, chain, SHORT, monkeypatch)


@pytest.mark.parametrize("chain", CHAIN, ids=["plain", "chained"])
@pytest.mark.parametrize("row", WHOLE_ROWS, ids=_id)
def test_unsplit_instance_whole_run_matches_oracle(row, chain, monkeypatch):
    """To convergence: the smallest and the largest geometry of each family, every U2 geometry and every NT/NT/9 of U3."""
    _run(row, chain, WHOLE, monkeypatch)


@pytest.mark.parametrize("key", TWICE, ids=lambda k: f"{k[0]}-{k[1]}.{k[2]}.{k[3]}")
def test_unsplit_instance_is_deterministic(key, monkeypatch):
    """Two runs of one chained case are bit-identical."""
    row, = [r for r in ROWS if (r.family, r.NT, r.NT2, r.NT3) == key]
    a = _run(row, 3, SHORT, monkeypatch)
    b = _run(row, 3, SHORT, monkeypatch)
    np.testing.assert_array_equal(a["gam_vb"], b["gam_vb"])
    np.testing.assert_array_equal(a["mu_beta_vb"], b["mu_beta_vb"])
