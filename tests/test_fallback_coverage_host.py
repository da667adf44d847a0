"""CPU: the tables of tests/test_gpu_fallback_instances.py against the launch planner and the launch code.

  * the generic instances the tables claim are exactly those the library compiles (aq_instance_query), each for complete Y and
    for NA, and all three staging widths ns; the masked tables name every compiled NT: an instance added to the set
    (aq_plan_const.h) fails here until a case runs it;
  * every row is planned as written (aq_plan_query, 256 CUs, with the missingness counts of the case's own Y): the fields
    the GPU case asserts from its handle;
  * the (NT, C) pairs of the masked kernel that are planned for some n <= 10 240 -- all 40, by a sweep of aq_plan_query over
    every n -- are those of the M1 table;
  * aq_vb_status reports only n_pad for the generic kernel -- (16, 1), (8, 2) and (4, 4) share n_pad = 1024 -- so (NE, WPT, ns)
    of every G row comes from the planner itself: tests/tools/plan_probe.cpp, built with the host compiler."""
import functools
import os
import shutil
import subprocess

import pytest

from atlasqtl_amd.core import plan_query
from tests import test_gpu_fallback_instances as F
from tests import test_plan_host as PH

MEM = PH.MEM
NCU = 256
PLAIN = {"tiles_per_group": 1, "tiles_matrix2": 0, "tiles_recurrence": 0, "instance_flags": 0}


def _listed():
    """(generic (NE, WPT), masked NT) the library compiles: aq_instance_query over a box of requests (tests/test_plan_host.py)."""
    return PH.compiled(2), {nt for nt, in PH.compiled(3)}


@functools.lru_cache(maxsize=None)
def _missing(kind, n, p=F.P, q=F.Q, na=0.0, arg=0):
    """(max_missing, max_short_list) of the case's own Y; the problem has the stated shape (no column was dropped)."""
    prob = F.problem(kind, n, p, q, na, arg)
    assert (prob["p"], prob["q"], prob["Y"].shape[0]) == (p, q, n)
    return F.missing_of(prob)


def _plan(n, p, q, mm, ms, hooks):
    return plan_query(n, p, q, mm, ms, ncu=NCU, total_bytes=MEM, overrides=hooks)


def _generic_rows():
    """Every handle of the G families: (n, p, q, max_missing, max_short_list, hooks, (NE, WPT, ns, n_pad))."""
    rows = []
    for ne, wpt, n, hook, n_pad, ns in F.TW_FORCED:
        for na in (0.0, F.TW_NA):
            mm, ms = _missing("plain", n, na=na) if na else (0, 0)
            rows.append((n, F.P, F.Q, mm, ms, F.tw_hooks(hook), (ne, wpt, ns, n_pad)))
    for ne, wpt, n, hook, n_pad, ns in F.TW_ENDS:
        rows.append((n, F.P, F.Q, 0, 0, F.tw_hooks(hook), (ne, wpt, ns, n_pad)))
    for n, (ne, wpt, n_pad, ns) in F.TW_NATURAL.items():
        mm, ms = _missing("trait", n, na=F.TW_NATURAL_NA, arg=F.MIS_MMAX + 1)
        assert mm == F.MIS_MMAX + 1
        rows.append((n, F.P, F.Q, mm, ms, {}, (ne, wpt, ns, n_pad)))
    n, p, q, na, (ne, wpt, n_pad, ns) = F.TW_DENSE
    mm, ms = _missing("plain", n, p, q, na)
    assert mm > F.MIS_MMAX
    rows.append((n, p, q, mm, ms, {}, (ne, wpt, ns, n_pad)))
    return rows


def test_generic_tables_name_exactly_the_compiled_instances():
    """An instance added to (or taken from) the compiled set fails here until the tables follow."""
    compiled, _ = _listed()
    generic, ns, _, _ = F.ledger()
    assert len(compiled) == 14
    assert generic == {(ne, wpt, na) for ne, wpt in compiled for na in (False, True)}, \
        sorted(generic ^ {(ne, wpt, na) for ne, wpt in compiled for na in (False, True)})
    assert {(r[0], r[1]) for r in F.TW_FORCED} == compiled and len(F.TW_FORCED) == len(compiled)   # G1 alone reaches every one
    assert ns == {1, 2, 4}
    assert {r[5] for r in F.TW_FORCED} == {1, 2, 4}
    for ne, wpt, n, hook, n_pad, s in F.TW_FORCED + F.TW_ENDS + [F.TW_TWICE]:
        assert n_pad == 64 * ne * wpt >= n and s == F.tw_ns(n_pad) and hook in (None, 2, 4)
    for ne, wpt, n, hook, n_pad, s in F.TW_FORCED:
        assert n == n_pad - 7 and n % 64 == 57                       # the last 64-sample slice is ragged
    # the range ends: n without any padding, and the first n of an instance -- one more than the planner gives a smaller one
    full = [r for r in F.TW_ENDS if r[2] == r[4]]
    first = [r for r in F.TW_ENDS if r[2] < r[4]]
    assert len(full) + len(first) == len(F.TW_ENDS) and len(full) >= 3 and len(first) >= 4
    assert {r[4] for r in full} >= {2048, 5120, F.N_FALLBACK}       # the last n of WPT = 1, 2 and 4
    for ne, wpt, n, hook, n_pad, s in first:
        below = plan_query(n - 1, F.P, F.Q, overrides=F.tw_hooks(hook))
        assert below["core_kernel"] == 2 and below["n_pad"] == n - 1 < n_pad, (n, below)
    assert F.TW_TWICE in F.TW_FORCED and 64 * F.TW_TWICE[0] * F.TW_TWICE[1] == F.N_FALLBACK
    assert {v[:2] for v in F.TW_NATURAL.values()} == {(ne, wpt) for ne, wpt in compiled if 64 * ne * wpt > 1024 and ne >= 32}
    assert F.TW_BORDER_N in F.TW_NATURAL and F.TW_DENSE[0] == F.N_FALLBACK


def test_masked_tables_name_every_instance():
    _, compiled = _listed()
    _, _, masked, chained = F.ledger()
    assert compiled == set(F.MIS_NT) == {1, 2, 4, 8, 16}
    assert {nt for nt, c in masked} == compiled and {nt for nt, c in F.MIS_GRID} == compiled
    assert {c for nt, c in masked} == set(range(1, 9))
    assert chained == {(nt, s) for nt in compiled for s in F.CHAIN_S}
    assert masked == set(F.MIS_GRID) == {(nt, c) for nt in compiled for c in range(1, 9)}   # the other families add no pair of their own
    corners = {(nt, c) for nt in (min(compiled), max(compiled)) for c in (1, 8)}
    assert set(F.MIS_WHOLE) >= corners | {(16, 5)} and F.MIS_TWICE in F.MIS_WHOLE    # (16, 5): the largest without an all-padding part
    nb = -(-F.CHAIN_P // 16)
    assert max(F.CHAIN_S) == nb and min(F.CHAIN_S) == 2               # one block per segment; two segments
    assert any(len({nb * (s + 1) // S - nb * s // S for s in range(S)}) > 1 for S in F.CHAIN_S)   # uneven segments
    assert {c > 1 for n, c, nt in F.LISTS} == {False, True} and max(nt for n, c, nt in F.LISTS) == max(compiled)
    assert len({F.LIST_FULL, F.LIST_EMPTY, F.LIST_ONE}) == 3 and max(F.LIST_FULL, F.LIST_EMPTY, F.LIST_ONE) < 16   # one trait tile


def test_every_generic_row_is_planned_as_written(hiplib):
    rows = _generic_rows()
    assert len(rows) == 2 * 14 + 7 + 5 + 1
    for n, p, q, mm, ms, hooks, (ne, wpt, ns, n_pad) in rows:
        st = _plan(n, p, q, mm, ms, hooks)
        want = dict(PLAIN, core_kernel=2, split_parts=1, chain_segments=0, tiles_matrix=0, n_pad=64 * ne * wpt)
        assert st == want and n_pad == st["n_pad"], (n, hooks, st)


def test_list_border_is_planned_on_both_sides(hiplib):
    """AQ_MIS_MMAX missing samples in one trait: the look-ahead MASK instances; one more: the generic kernel."""
    n = F.TW_BORDER_N
    mm, ms = _missing("trait", n, na=F.TW_NATURAL_NA, arg=F.MIS_MMAX)
    assert mm == F.MIS_MMAX
    st = _plan(n, F.P, F.Q, mm, ms, {})
    assert st["core_kernel"] == 0 and st["instance_flags"] == F.MASK, st
    mm, ms = _missing("trait", n, na=F.TW_NATURAL_NA, arg=F.MIS_MMAX + 1)
    assert _plan(n, F.P, F.Q, mm, ms, {})["core_kernel"] == 2


def _masked_want(nt, c, chain=0):
    return dict(PLAIN, core_kernel=3, split_parts=c, chain_segments=chain, tiles_matrix=nt, n_pad=128 * nt * c)


def test_every_masked_row_is_planned_as_written(hiplib):
    for nt, c in F.MIS_GRID:
        n = F.mis_n(nt, c)
        assert n <= F.N_FALLBACK and n % 16 == 11                    # the last sample tile is ragged
        mm, ms = _missing("plain", n, na=F.MIS_NA)
        assert 1 <= mm <= F.MIS_MMAX
        for counts in ((mm, ms), (1, 1)):                              # 5 % NA; a single NaN
            assert _plan(n, F.P, F.Q, *counts, F.mis_hooks(c)) == _masked_want(nt, c), (nt, c, counts)
    for nt, c in F.MIS_WHOLE + [F.MIS_TWICE]:
        assert (nt, c) in F.MIS_GRID
    for nt in F.MIS_NT:
        mm, ms = _missing("plain", F.mis_n(nt, 1), F.CHAIN_P, F.Q, F.MIS_NA)
        for s in F.CHAIN_S:
            assert _plan(F.mis_n(nt, 1), F.CHAIN_P, F.Q, mm, ms, F.mis_hooks(1, s)) == _masked_want(nt, 1, s), (nt, s)
    for n, c, nt in F.LISTS:
        mm, ms = _missing("lists", n, na=F.MIS_NA)
        assert mm == F.MIS_MMAX
        assert _plan(n, F.P, F.Q, mm, ms, F.mis_hooks(c)) == _masked_want(nt, c), (n, c)
    for n, (c, nt) in F.MIS_NATURAL.items():
        mm, ms = _missing("plain", n, na=F.MIS_NA)
        assert mm <= F.MIS_MMAX
        assert _plan(n, F.P, F.Q, mm, ms, {"AQ_GK_MAX_GB": F.GK_MAX_GB}) == _masked_want(nt, c), (n, c, nt)
        assert _plan(n, F.P, F.Q, mm, ms, {})["core_kernel"] == 0     # ... which only the memory hook takes from the MASK instances


def _masked_pairs(hiplib, hooks_of_c, cs, q=F.Q):
    """{(NT, C): smallest n that is planned so} over every n the masked kernel serves, with the counts of the single-NaN cases.
    A forced C is swept up to the 2048 C samples its parts can hold.  (Beyond that the hook is a misuse that the planner does not
    refuse: it answers NT = 16 with n_pad = 2048 C < n.  tests/golden/plan_table_parent.json pins that answer at n = 5000,
    C = 2, so it stays; no case here and no hook-free plan goes there.)"""
    first = {}
    for c in cs:
        for n in range(2, min(2048 * (c or 8), F.N_FALLBACK) + 1):
            rc, msg, st, _ = PH._query(hiplib, n, F.P, q, 1, 1, NCU, MEM, hooks_of_c(c))
            assert rc == 0 and st["core_kernel"] == 3 and st["n_pad"] == 128 * st["tiles_matrix"] * st["split_parts"] >= n, (n, c, msg, st)
            first.setdefault((st["tiles_matrix"], st["split_parts"]), n)
    return first


def test_reachable_masked_pairs_are_the_table(hiplib):
    """What AQ_KERNEL = 3 with AQ_MIS_C = 1 ... 8 plans over every n <= 10 240: all 40 (NT, C), (16, 6 ... 8) among them, each
    from n = 64 NT C + 1 on.  A planner change that opens or closes a pair is noticed here: the M1 table must name exactly these.
    Left to itself (AQ_KERNEL = 3 alone) the planner never picks NT = 16 with C >= 6: (16, 5) fits every n and is found first."""
    first = _masked_pairs(hiplib, F.mis_hooks, range(1, 9))
    assert set(first) == set(F.MIS_GRID) and len(first) == 40, \
        f"planned pairs not in the M1 table: {sorted(set(first) - set(F.MIS_GRID))}; table pairs never planned: {sorted(set(F.MIS_GRID) - set(first))}"
    for (nt, c), n0 in first.items():
        assert n0 == (64 * nt * c + 1 if nt > 1 else 2), (nt, c, n0)
        assert n0 <= F.mis_n(nt, c) <= min(128 * nt * c, F.N_FALLBACK), (nt, c)     # the case's n lies in the pair's range
    for q in (F.Q, 5000):
        own = _masked_pairs(hiplib, lambda c: {"AQ_KERNEL": 3}, [None], q=q)
        assert own and not [(nt, c) for nt, c in own if nt == 16 and c >= 6], sorted(own)
    # beyond the kernels' n the hooks are refused: the n = 128 NT C - 5 of the other rows is no case for (16, 6 ... 8)
    for c in (6, 7, 8):
        rc, msg, _, _ = PH._query(hiplib, 128 * 16 * c - 5, F.P, F.Q, 1, 1, NCU, MEM, F.mis_hooks(c))
        assert rc == 3 and msg == "AQ_KERNEL: only the look-ahead kernel serves n > 10240", (c, rc, msg)


def test_probe_proves_ne_wpt_and_ns_of_every_generic_row(tmp_path):
    """The planner's own (use_tw, NE, WPT, tw_ns, n_pad) of every G row, from the stand-alone probe."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    exe = tmp_path / "plan_probe"
    src = os.path.join(PH.ROOT, "tests", "tools", "plan_probe.cpp")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", PH.CSRC, src, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = _generic_rows()
    text = "".join(f"{n} {p} {q} {mm} {ms} {','.join(f'{k}={v}' for k, v in hooks.items()) or '-'}\n" for n, p, q, mm, ms, hooks, _ in rows)
    r = subprocess.run([str(exe), str(NCU), str(MEM)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout.splitlines()
    assert len(out) == len(rows)
    seen = set()
    for (n, p, q, mm, ms, hooks, (ne, wpt, ns, n_pad)), line in zip(rows, out):
        assert line.split() == [str(v) for v in (1, ne, wpt, ns, n_pad)], (n, hooks, mm, line)
        seen.add((ne, wpt, bool(mm), ns))
    compiled, _ = _listed()
    assert {(ne, wpt, na) for ne, wpt, na, _ in seen} == {(ne, wpt, na) for ne, wpt in compiled for na in (False, True)}
    assert {ns for _, _, _, ns in seen} == {1, 2, 4}
    assert {(ne, wpt, ns) for ne, wpt, _, ns in seen if ns < 4} == {(40, 2, 2), (32, 4, 2), (40, 4, 1)}
