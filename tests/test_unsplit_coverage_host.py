"""CPU: the tables of tests/test_gpu_unsplit_instances.py (and MEDIUM_FORCED_SMALL of tests/test_gpu_split_instances.py) against
the launch planner and the compiled instance set.

  * every row is planned as written, on 256 and on 64 CUs;
  * the kernels the tables claim are the ones the library compiles (aq_instance_query), minus UNREACHABLE;
  * a sweep of the planner over n = 1 ... 1056 and its hooks reaches exactly the claimed kernels and none of UNREACHABLE;
  * every wave that owns tiles owns a live one, but for RECURRENCE_TILES_ALL_PADDING."""
import functools

import numpy as np

from atlasqtl_amd.core import plan_query
from tests import test_gpu_split_instances as T
from tests import test_gpu_unsplit_instances as U
from tests import test_plan_host as PH

MASK, WIDE, SEG = T.MASK, T.WIDE, T.SEG
MEM = PH.MEM
NCU = (256, 64)


@functools.lru_cache(maxsize=None)
def _missing_of(n, p, q, na):
    """(max_missing, max_short_list) of the case's own Y."""
    if not na:
        return 0, 0
    prob = T._problem(n, p, q, na)
    assert (prob["p"], prob["q"]) == (p, q)
    m = np.isnan(prob["Y"]).sum(axis=0)
    return int(m.max()), int(np.minimum(m, n - m).max())


def _instance(st):
    return (st["instance_flags"], st["tiles_per_group"], st["tiles_matrix"], st["tiles_matrix2"], st["tiles_recurrence"], st["chain_segments"])


def test_tables_have_the_stated_shape():
    rows = U.rows()
    fam = {f: [r for r in rows if r.family == f] for f in ("U1", "U2", "U3", "U4")}
    assert [len(fam[f]) for f in ("U1", "U2", "U3", "U4")] == [21, 11, 24, 21] and len(rows) == 77
    assert len(U.ledger()) == 154 == len(rows) * len(U.CHAIN)
    assert sorted(U.PAIRS) == list(range(2, 23)) and all(nt + nt2 == k and nt2 in (nt, nt - 1) for k, (nt, nt2) in U.PAIRS.items())
    for r in rows:
        T_ = 3 * (r.NT + r.NT2) + r.NT3
        assert r.n == min(16 * T_ - 5, 1051) <= U.N_UNSPLIT and U.n_pad_of(r) == 16 * T_ >= r.n
        assert r.na == (U.NA if r.family == "U4" else 0.0) and r.mask == int(r.family == "U4")
    assert [r.n for r in fam["U1"]] == [48 * k - 5 for k in range(2, 23)] == [r.n for r in fam["U4"]]
    assert {(r.NT, r.NT2, r.NT3) for r in fam["U2"]} == set(U.RECURRENCE) and len(U.RECURRENCE) == 11
    assert {(r.NT, r.NT2, r.NT3) for r in fam["U3"]} == set(U.RECURRENCE) | {U.PAIRS[k] + (0,) for k in range(2, 15)}
    # whole runs: the ends of each family, every U2 geometry, every NT / NT / 9
    whole = {(r.family, r.NT, r.NT2, r.NT3) for r in rows if r.whole}
    assert whole >= {(f, 1, 1, 0) for f in ("U1", "U3", "U4")} | {("U1", 11, 11, 0), ("U4", 11, 11, 0), ("U3", 11, 11, 3)}
    assert whole >= {("U2",) + g for g in U.RECURRENCE} | {("U3",) + g for g in U.RECURRENCE if g[2] == 9}
    assert set(U.TWICE) == {("U1", 11, 11, 0), ("U2", 10, 10, 9), ("U3", 11, 11, 3), ("U4", 11, 11, 0)}
    assert {(r.family, r.NT, r.NT2, r.NT3) for r in rows} >= set(U.TWICE)


def test_every_unsplit_row_is_planned_as_written(hiplib):
    for r in U.rows():
        mm, ms = _missing_of(r.n, U.P, U.Q, r.na)
        assert bool(mm) == bool(r.mask)
        for chain in U.CHAIN:
            for ncu in NCU:
                st = plan_query(r.n, U.P, U.Q, mm, ms, ncu=ncu, total_bytes=MEM, overrides=U.hooks_of(r, chain))
                assert st["core_kernel"] == 0 and st["split_parts"] == 1, (r, chain, ncu, st)
                assert _instance(st) == U.instance_of(r, chain), (r, chain, ncu, st)
                assert not st["instance_flags"] & WIDE and st["n_pad"] == U.n_pad_of(r), (r, chain, ncu, st)


def test_every_small_medium_row_is_planned_as_written(hiplib):
    for k, (nt, nt2) in T.MEDIUM_FORCED_SMALL.items():
        n = 96 * k - 5
        for na in (0.0, T.MEDIUM_NA):
            mm, ms = _missing_of(n, 70, 33, na)
            assert mm <= T.MIS_MMAX
            for xh in (0, 1):
                for ncu in NCU:
                    st = plan_query(n, 70, 33, mm, ms, ncu=ncu, total_bytes=MEM, overrides={"AQ_LA_C": 2, "AQ_LA_XHELPER": xh})
                    assert (st["core_kernel"], st["split_parts"]) == (0, 2), (k, na, xh, ncu, st)
                    assert _instance(st) == (MASK if na else 0, 1, nt, nt2, 0, 0), (k, na, xh, ncu, st)
                    assert st["n_pad"] == 16 * 3 * (nt + nt2) * 2 >= n, (k, na, xh, ncu, st)


def test_claimed_kernels_are_the_compiled_ones_but_the_unreachable():
    """An instance added to the compiled set (aq_plan_const.h) fails here until a case runs it."""
    compiled, claimed, unreachable = PH.compiled_unsplit(), U.ledger(), set(U.UNREACHABLE)
    assert len(compiled) == 158 and len(unreachable) == 4 and all(U.UNREACHABLE.values())
    assert unreachable == {(0, tt, 11, 11, 9, seg) for tt in (1, 2) for seg in (0, 1)}
    assert unreachable <= compiled and not unreachable & claimed
    assert claimed == compiled - unreachable, sorted(claimed ^ (compiled - unreachable))
    assert len(claimed) == 154


def test_planner_reaches_every_claimed_kernel_and_no_unreachable_one(hiplib):
    """n = 1 ... 1056, complete Y and Y with NA, AQ_TT, AQ_NT3, AQ_LA_NOSPLIT and AQ_CHAIN unset and at each of their values:
    what the planner launches unsplit.  Should a change to it make 11/11/9 reachable, this fails until a case is added."""
    reached = set()
    for n in range(1, U.N_UNSPLIT + 1):
        for na in (0.0, U.NA):
            mm, ms = PH._missing(n, na)
            if na and mm == 0:
                mm = ms = 1
            for tt in (None, 1, 2):
                for nt3 in (None, 0, 3, 6, 9):
                    for nosplit in (None, 1):
                        for chain in (None, 3):
                            ov = {k: v for k, v in (("AQ_TT", tt), ("AQ_NT3", nt3), ("AQ_LA_NOSPLIT", nosplit), ("AQ_CHAIN", chain))
                                  if v is not None}
                            rc, _msg, st, _ = PH._query(hiplib, n, U.P, U.Q, mm, ms, 256, MEM, ov)
                            if rc or st["core_kernel"] != 0 or st["split_parts"] != 1:
                                continue
                            f = st["instance_flags"]
                            assert not f & WIDE and bool(f & SEG) == (st["chain_segments"] > 1), (n, na, ov, st)
                            reached.add((f & MASK, st["tiles_per_group"], st["tiles_matrix"], st["tiles_matrix2"], st["tiles_recurrence"],
                                         int(bool(f & SEG))))
    assert not reached & set(U.UNREACHABLE), sorted(reached & set(U.UNREACHABLE))
    assert reached == U.ledger(), sorted(reached ^ U.ledger())
    assert len(reached) == 154 and len(PH.compiled_unsplit() - reached) == 4


def _live_tiles(NT, NT2, NT3, n):
    """Live tiles (holding at least one of the n samples) of each wave that owns tiles -- the tile map of aq_core_sweep_la.h:
    waves 0-2 take NT tiles each from tile 0, waves 4-6 NT2 each from tile 3 NT, the recurrence wave NT3 from 3 (NT + NT2)."""
    live = -(-n // 16)
    spans = {f"matrix{w}": (w * NT, NT) for w in range(3)}
    spans.update({f"matrix{4 + w}": (3 * NT + w * NT2, NT2) for w in range(3)})
    spans["recurrence"] = (3 * (NT + NT2), NT3)
    return {role: max(0, min(t0 + cnt, live) - t0) for role, (t0, cnt) in spans.items() if cnt > 0}


def test_every_wave_with_tiles_has_a_live_one():
    padding = set()
    for r in U.rows():
        live = _live_tiles(r.NT, r.NT2, r.NT3, r.n)
        assert len(live) == (7 if r.NT3 else 6) and sum(live.values()) == -(-r.n // 16), (r, live)
        assert r.n % 16 == 11                                         # the last live tile is ragged: 11 of 16
        for role, cnt in live.items():
            if cnt == 0:
                assert role == "recurrence", (r, live)
                padding.add((r.TT, r.NT, r.NT2, r.NT3))
        if U.n_pad_of(r) // 16 <= 66:                                 # nothing but the ragged end is padding
            assert sum(live.values()) == U.n_pad_of(r) // 16, (r, live)
    assert padding == U.RECURRENCE_TILES_ALL_PADDING == {(1, 11, 11, 3), (2, 11, 11, 3)}
    for k, (nt, nt2) in T.MEDIUM_FORCED_SMALL.items():               # two parts of 3 k tiles: the second one's last tile is the ragged one
        n = 96 * k - 5
        assert -(-n // 16) == 2 * 3 * k and n % 16 == 11
