"""The launch planner (atlasqtl_amd/csrc/aq_plan.h) on the CPU, through aq_plan_query: no device, no environment.

  * tests/golden/plan_table_parent.json -- the plans of the commit before the planner was moved out of aq_vb_create (its
    "parent_commit"; "source" and "device" say how and where they were obtained) -- reproduces row by row: all nine plan
    fields, or the same error;
  * the tables of expected plans of tests/test_gpu_split_instances.py hold at 256 CUs;
  * invariants over a sweep of n from 2 to AQ_N_MAX: the plan succeeds, n_pad follows the geometry of its kernel, the parts of
    a split fit the chip, a split is never chained, and the instance is one the library compiles;
  * what the library compiles, and which kernel a request reaches: aq_instance_query (the launchers' own dispatch, run dry) over
    a box of requests that strictly contains the compiled set -- the source of every other module's "compiled" set."""
import ctypes as C
import functools
import itertools
import json
import os
import re
import shutil
import subprocess

import pytest

from atlasqtl_amd import _lib
from atlasqtl_amd.core import PLAN_KEYS, plan_query
from tests import test_gpu_split_instances as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "atlasqtl_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_table_parent.json")
MASK, WIDE, SEG = T.MASK, T.WIDE, T.SEG
N_MAX = T.N_MAX
MEM = 288 * 10**9          # device memory of the table cases: more than any of them needs


def _query(hiplib, n, p, q, mm, ms, ncu, total, overrides):
    """(rc, message, plan) of aq_plan_query, errors included."""
    st = _lib.AqVbStatus()
    ov = " ".join(f"{k}={v}" for k, v in overrides.items()) if isinstance(overrides, dict) else (overrides or "")
    rc = hiplib.aq_plan_query(n, p, q, mm, ms, ncu, total, ov.encode() if ov else None, C.byref(st))
    msg = hiplib.aq_last_error().decode() if rc else ""
    return rc, msg, ({k: getattr(st, k) for k in PLAN_KEYS} if rc == 0 else None), st


def _missing(n, na):
    """Per-trait missing count of a case with a fraction na of NA (any count <= AQ_MIS_MMAX plans alike below the wide split;
    the wide split takes any)."""
    m = int(round(na * n)) if na else 0
    return m, min(m, n - m)


# ------------------------------------------------------------------------------------------------------------------------------
# the parent's plans

def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_table_covers_the_grid():
    doc = _golden()
    rows = doc["rows"]
    assert re.fullmatch(r"[0-9a-f]{40}", doc["parent_commit"]) and doc["ncu"] > 0 and doc["total_bytes"] > 0 and doc["source"]
    assert len(rows) >= 300
    complete = {r["n"] for r in rows if r["na"] == "none" and not r["env"]}
    assert complete >= {2, 16, 17, 500, 800, 900, 1000, 1056, 1057, 1500, 2048, 2049, 5000, 5120, 8448, 8449, 10240, 10241, 16384,
                        16385, 20480, 50000, 82943, 82944, 82945}
    assert [r["rc"] for r in rows if r["n"] == 82945] == [3]
    assert any(r["max_missing"] > T.MIS_MMAX and r["n"] <= 10240 for r in rows)
    hooks = {k for r in rows for k in r["env"]}
    assert hooks >= {"AQ_NCU", "AQ_KERNEL", "AQ_TT", "AQ_NT3", "AQ_CHAIN", "AQ_LA_C", "AQ_LA_XHELPER", "AQ_LA_NOSPLIT", "AQ_MIS_C",
                     "AQ_TW_WPT", "AQ_STAGGER", "AQ_HPRIO", "AQ_MPRIO", "AQ_XTOUCH", "AQ_GK_MAX_GB"}
    assert {r["plan"]["core_kernel"] for r in rows if r["plan"]} == {0, 2, 3}
    assert {r["plan"]["instance_flags"] for r in rows if r["plan"]} >= {0, MASK, WIDE, WIDE | MASK, SEG, SEG | MASK}
    assert {r["plan"]["tiles_per_group"] for r in rows if r["plan"]} == {1, 2}
    assert sum(1 for r in rows if r["rc"]) >= 6


def test_every_parent_plan_reproduces(hiplib):
    doc = _golden()
    bad = []
    for r in doc["rows"]:
        rc, msg, plan, _ = _query(hiplib, r["n"], r["p"], r["q"], r["max_missing"], r["max_short_list"], doc["ncu"], doc["total_bytes"],
                                  r["env"])
        if (rc, msg, plan) != (r["rc"], r["error"], r["plan"]):
            bad.append((r, rc, msg, plan))
    assert not bad, f"{len(bad)} of {len(doc['rows'])} rows differ, first: {bad[0]}"


# ------------------------------------------------------------------------------------------------------------------------------
# the tables of tests/test_gpu_split_instances.py, at 256 CUs

def _instance(hiplib, n, p, q, na, env, flags, C_, NT, NT2):
    mm, ms = _missing(n, na)
    rc, msg, st, _ = _query(hiplib, n, p, q, mm, ms, 256, MEM, env)
    assert rc == 0, msg
    got = (st["core_kernel"], st["instance_flags"], st["split_parts"], st["tiles_matrix"], st["tiles_matrix2"])
    assert got == (0, flags, C_, NT, NT2), (n, q, na, env, got)
    assert st["tiles_per_group"] == 1 and st["chain_segments"] == 0 and st["tiles_recurrence"] == 0
    assert st["n_pad"] == 16 * C_ * 3 * (NT + NT2) >= n
    return st


def test_medium_natural_table(hiplib):
    for (n, p, q, na, _maxit), (C_, nt, nt2) in T.MEDIUM_NATURAL:
        _instance(hiplib, n, p, q, na, {}, MASK if na else 0, C_, nt, nt2)


def test_medium_forced_table(hiplib):
    for k, (nt, nt2) in T.MEDIUM_FORCED.items():
        for na in (0.0, T.MEDIUM_NA):
            for xh in ("0", "1"):
                _instance(hiplib, 96 * k - 5, 70, 33, na, {"AQ_LA_C": "2", "AQ_LA_XHELPER": xh}, MASK if na else 0, 2, nt, nt2)


def test_wide_forced_table(hiplib):
    for nt in T.WIDE_FORCED_NT:
        for na in (0.0, T.WIDE_NA):
            _instance(hiplib, 864 * nt - 7, 70, 33, na, {"AQ_LA_C": str(T.WIDE_FORCED_C)}, WIDE | (MASK if na else 0), T.WIDE_FORCED_C,
                      nt, nt)


def test_parts_table(hiplib):
    seen = set()
    for nt, cs in T.PARTS_NT.items():
        for C_ in cs:
            seen.add(C_)
            for na in (0.0, T.PARTS_NA):
                st = _instance(hiplib, T.PARTS_N, T.PARTS_P, T.PARTS_Q, na, {"AQ_LA_C": str(C_)}, WIDE | (MASK if na else 0), C_, nt, nt)
                assert st["n_pad"] == 96 * nt * C_
    assert seen == set(range(9, 49))


def test_limit_table(hiplib):
    for (n, na), (C_, nt) in T.LIMIT:
        st = _instance(hiplib, n, T.LIMIT_P, T.LIMIT_Q, na, {}, WIDE | (MASK if na else 0), C_, nt, nt)
        assert st["n_pad"] == 96 * nt * C_
        if n >= N_MAX - 1:
            assert st["n_pad"] == N_MAX


# ------------------------------------------------------------------------------------------------------------------------------
# invariants over n

LA_FIELDS = ("nt", "nt2", "seg", "tt", "mask", "nt3", "wide")
NO_INSTANCE = {0: "no look-ahead kernel instantiation for this n", 2: "no generic kernel instantiation for this n",
               3: "no masked MFMA kernel instantiation for this n"}


def resolve(hiplib, request, ne=0, wpt=0):
    """aq_instance_query: the launchers' own dispatch, run dry.  The resolved instance as a dict of aq_kernel_instance, or None
    when the launch path refuses the request -- which it must do as AQ_ERR_UNSUPPORTED, in the launcher's words."""
    out = _lib.AqKernelInstance()
    rc = hiplib.aq_instance_query(C.byref(request), ne, wpt, C.byref(out))
    if rc:
        assert rc == 3 and hiplib.aq_last_error().decode() == NO_INSTANCE[request.core_kernel], (rc, hiplib.aq_last_error())
        assert bytes(out) == bytes(C.sizeof(out))                   # nothing but zeroes on refusal
        return None
    return {k: getattr(out, k) for k, _t in _lib.AqKernelInstance._fields_}


def la_request(mask, wide, TT, NT, NT2, NT3, seg):
    return _lib.AqVbStatus(core_kernel=0, instance_flags=(MASK if mask else 0) | (WIDE if wide else 0) | (SEG if seg else 0),
                           tiles_per_group=TT, tiles_matrix=NT, tiles_matrix2=NT2, tiles_recurrence=NT3)


@functools.lru_cache(maxsize=None)
def instance_box():
    """Every request of a box that strictly contains the compiled set -> what it resolves to (None: refused).  Look-ahead
    kernel: (0, mask, wide, TT, NT, NT2, NT3, seg) over mask, wide, seg in 0/1, TT in 1 ... 3 (3 must be refused), NT and NT2 in
    0 ... 20, NT3 in 0, 3, 6, 9; generic kernel: (2, NE, WPT) over 1 ... 64 x 1 ... 8; masked kernel: (3, NT) over 1 ... 32."""
    hiplib = _lib.lib()
    box = {}
    for mask, wide, TT, seg in itertools.product((0, 1), (0, 1), (1, 2, 3), (0, 1)):
        for NT, NT2, NT3 in itertools.product(range(21), range(21), (0, 3, 6, 9)):
            box[(0, mask, wide, TT, NT, NT2, NT3, seg)] = resolve(hiplib, la_request(mask, wide, TT, NT, NT2, NT3, seg))
    for ne, wpt in itertools.product(range(1, 65), range(1, 9)):
        box[(2, ne, wpt)] = resolve(hiplib, _lib.AqVbStatus(core_kernel=2), ne, wpt)
    for nt in range(1, 33):
        box[(3, nt)] = resolve(hiplib, _lib.AqVbStatus(core_kernel=3, tiles_matrix=nt))
    return box


def compiled(kernel):
    """The accepted requests of one kernel, without the kernel id: what the library compiles."""
    return {k[1:] for k, v in instance_box().items() if k[0] == kernel and v is not None}


def compiled_unsplit():
    """The kernels of the unsplit launches, each plain and chained: (mask, TT, NT, NT2, NT3, seg), NT3 as aq_vb_status reports it
    (aq_la_nt3 of a two-tile workgroup) -- every compiled instance that is not WIDE and exists chained as well.  (The others are
    the split's: tests/test_host_logic.py::test_split_instance_ledger_is_complete.)"""
    la = compiled(0)
    return {(m, TT, NT, NT2, NT3, seg) for m, w, TT, NT, NT2, NT3, seg in la if not w and (m, w, TT, NT, NT2, NT3, 1) in la}


def test_every_request_resolves_to_itself_or_is_refused():
    """For every request of the box the library accepts, the template parameters of the kernel it would launch are the request's,
    one by one; what it refuses, it refuses as the launch does (resolve()).  222 + 14 + 5 are accepted."""
    box = instance_box()
    assert len(box) == 2 * 2 * 3 * 2 * 21 * 21 * 4 + 64 * 8 + 32
    wrong = []
    for key, got in box.items():
        if got is None:
            continue
        if key[0] == 0:
            _, mask, wide, TT, NT, NT2, NT3, seg = key
            want = dict(core_kernel=0, nt=NT, nt2=NT2, seg=seg, tt=TT, mask=mask, nt3=NT3, wide=wide, ne=0, wpt=0)
        elif key[0] == 2:
            want = dict(core_kernel=2, nt=0, nt2=0, seg=0, tt=0, mask=0, nt3=0, wide=0, ne=key[1], wpt=key[2])
        else:
            want = dict(core_kernel=3, nt=key[1], nt2=0, seg=0, tt=0, mask=0, nt3=0, wide=0, ne=0, wpt=0)
        if got != want:
            wrong.append((key, got))
    assert not wrong, f"{len(wrong)} requests reach another kernel, first: {wrong[:3]}"
    la = compiled(0)
    unit = {name: sum(1 for m, w, TT, *_ in la if (m, w, TT) == key)
            for name, key in (("la1", (0, 0, 1)), ("la2", (0, 0, 2)), ("la1m", (1, 0, 1)), ("la1w", (0, 1, 1)), ("la1wm", (1, 1, 1)))}
    assert unit == {"la1": 80, "la2": 50, "la1m": 56, "la1w": 18, "la1wm": 18} and len(la) == 222
    assert len(compiled(2)) == 14 and len(compiled(3)) == 5
    assert not [k for k in la if k[2] == 3]                          # TT = 3: never
    # an unknown kernel is an argument error, not a refusal
    assert _lib.lib().aq_instance_query(C.byref(_lib.AqVbStatus(core_kernel=1)), 0, 0, C.byref(_lib.AqKernelInstance())) == 1
    assert _lib.lib().aq_instance_query(None, 0, 0, C.byref(_lib.AqKernelInstance())) == 1


def _sweep_n():
    return list(range(2, 1101)) + list(range(1101, N_MAX, 97)) + [N_MAX]


@pytest.mark.parametrize("ncu", [64, 256])
@pytest.mark.parametrize("na", [0.0, 0.04], ids=["complete", "na"])
@pytest.mark.parametrize("q", [33, 5000])
def test_plan_invariants_over_n(hiplib, q, na, ncu):
    p = 48
    tw_pads = {64 * ne * w for ne, w in compiled(2)}
    kernels = set()
    for n in _sweep_n():
        mm, ms = _missing(n, na)
        if na and mm == 0:
            mm = ms = 1
        rc, msg, st, request = _query(hiplib, n, p, q, mm, ms, ncu, MEM, {})
        assert rc == 0, (n, msg)
        k, parts, NT, NT2, NT3 = st["core_kernel"], st["split_parts"], st["tiles_matrix"], st["tiles_matrix2"], st["tiles_recurrence"]
        flags, TT = st["instance_flags"], st["tiles_per_group"]
        kernels.add(k)
        assert st["n_pad"] >= n, (n, st)
        assert 1 <= parts <= 48, (n, st)
        if parts > 1:
            assert st["chain_segments"] == 0, (n, st)
        if k == 0:
            tiles = 6 * NT if flags & WIDE else 3 * (NT + NT2) + NT3
            assert st["n_pad"] == 16 * parts * tiles, (n, st)
            got = resolve(hiplib, request)                          # the instance is one the library compiles: this one
            assert got and tuple(got[f] for f in LA_FIELDS) == (NT, NT2, int(bool(flags & SEG)), TT, int(bool(flags & MASK)), NT3,
                                                                int(bool(flags & WIDE))), (n, st, got)
            assert bool(flags & SEG) == (st["chain_segments"] > 1) and bool(flags & MASK) == bool(na), (n, st)
            assert bool(flags & WIDE) == (n > 10240) and (parts >= 9) == (n > 10240), (n, st)
            if parts > 1 and n <= 1056:
                assert TT == 1 and parts * ((q + 15) // 16) <= ncu, (n, st)
        elif k == 3:
            assert st["n_pad"] == 128 * NT * parts and NT in (1, 2, 4, 8, 16) and parts <= 8, (n, st)
            assert (NT2, NT3, flags, TT) == (0, 0, 0, 1) and resolve(hiplib, request)["nt"] == NT, (n, st)
        else:
            assert k == 2 and st["n_pad"] in tw_pads and (parts, NT, NT2, NT3, flags, TT) == (1, 0, 0, 0, 0, 1), (n, st)
    assert 0 in kernels


def test_generic_and_masked_kernels_are_reached(hiplib):
    """A trait with more than AQ_MIS_MMAX missing values below the wide split, and the kernels forced by AQ_KERNEL."""
    assert plan_query(5000, 48, 33, max_missing=T.MIS_MMAX + 1, max_short_list=T.MIS_MMAX + 1, total_bytes=MEM)["core_kernel"] == 2
    assert plan_query(5000, 48, 33, max_missing=T.MIS_MMAX, max_short_list=T.MIS_MMAX, total_bytes=MEM)["core_kernel"] == 0
    assert plan_query(1000, 48, 33, max_missing=10, max_short_list=10, overrides={"AQ_KERNEL": 3})["core_kernel"] == 3
    assert plan_query(1000, 48, 33, overrides="AQ_KERNEL=2")["core_kernel"] == 2
    st = plan_query(12000, 48, 33, max_missing=11000, max_short_list=1000, total_bytes=MEM)
    assert st["core_kernel"] == 0 and st["instance_flags"] == WIDE | MASK


def test_refusals_carry_code_and_message(hiplib):
    rc, msg, _, st = _query(hiplib, N_MAX + 1, 16, 17, 0, 0, 256, MEM, {})
    assert rc == 3 and "exceeds the largest supported sample count" in msg and str(N_MAX) in msg
    assert bytes(st) == bytes(C.sizeof(st))                      # nothing but zeroes on failure
    rc, msg, _, _ = _query(hiplib, 1000, 16, 17, 0, 0, 256, MEM, {"AQ_LA_C": 49})
    assert rc == 1 and msg == "AQ_LA_C: the wide sample split takes 9 ... 48 parts"
    rc, msg, _, _ = _query(hiplib, 12000, 16, 17, 0, 0, 256, MEM, {"AQ_LA_C": 8})
    assert rc == 1 and msg == "AQ_LA_C: the wide sample split takes 9 ... 48 parts"
    rc, msg, _, _ = _query(hiplib, 12000, 16, 17, 0, 0, 256, MEM, {"AQ_KERNEL": 2})
    assert rc == 3 and msg == "AQ_KERNEL: only the look-ahead kernel serves n > 10240"
    rc, msg, _, _ = _query(hiplib, 12000, 16, 17, 0, 0, 256, -1, {})          # the wide split cannot do without the memory size
    assert rc == 1 and "total_bytes" in msg and "hip" not in msg
    rc, msg, _, _ = _query(hiplib, 1000, 16, 17, 50, 50, 256, -1, {})         # ... below it an unknown size only costs the MASK instances
    assert rc == 0
    assert hiplib.aq_plan_query(1, 16, 17, 0, 0, 256, MEM, None, C.byref(_lib.AqVbStatus())) == 1
    assert hiplib.aq_plan_query(100, 16, 17, 0, 0, 256, MEM, b"AQ_TT", C.byref(_lib.AqVbStatus())) == 1
    assert hiplib.aq_plan_query(100, 16, 17, 0, 0, 256, MEM, None, None) == 1


def test_only_plan_fields_are_filled(hiplib):
    rc, _, plan, st = _query(hiplib, 1000, 48, 5000, 0, 0, 256, MEM, {})
    assert rc == 0 and plan["n_pad"] >= 1000
    for name, _t in _lib.AqVbStatus._fields_:
        if name not in PLAN_KEYS:
            assert getattr(st, name) == 0, name
    assert plan_query(1000, 48, 5000, total_bytes=MEM) == plan


def test_process_environment_is_ignored(hiplib, monkeypatch):
    base = plan_query(1000, 48, 33)
    assert base["tiles_per_group"] == 1
    forced = plan_query(1000, 48, 33, overrides={"AQ_TT": 2})
    assert forced["tiles_per_group"] == 2 and forced != base
    monkeypatch.setenv("AQ_TT", "2")
    monkeypatch.setenv("AQ_NCU", "8")
    monkeypatch.setenv("AQ_KERNEL", "2")
    assert plan_query(1000, 48, 33) == base
    assert plan_query(1000, 48, 33, overrides="") == base


def test_planner_header_is_plain_host_cxx(tmp_path):
    """aq_plan.h (and the constants header the kernels share with it) includes no HIP header and compiles with the host compiler."""
    for name in ("aq_plan.h", "aq_plan_const.h"):
        with open(os.path.join(CSRC, name)) as f:
            incs = re.findall(r'#include\s*[<"]([^>"]+)[>"]', f.read())
        assert not [i for i in incs if "hip" in i.lower() and not i.endswith("atlasqtl_hip.h")], (name, incs)
    with open(os.path.join(ROOT, "include", "atlasqtl_hip.h")) as f:
        assert re.findall(r'#include\s*[<"]([^>"]+)[>"]', f.read()) == ["stdint.h"]
    for name in ("aq_core_sweep.h", "aq_core_sweep_mis.h"):        # one definition of the shared limits
        with open(os.path.join(CSRC, name)) as f:
            src = f.read()
        assert ('#include "aq_plan_const.h"' in src) == (name == "aq_core_sweep.h") and not re.search(r"(constexpr int|#define)\s+AQ_(LA_CMAX|N_MAX|GK_STRIDE|MIS_MMAX)\b", src)
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "aq_plan.h"\nint aq_tu_uses_it() { AqPlan pl; return aq_make_plan(AqPlanInput(), AqEnv(), &pl, nullptr); }\n')
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I", CSRC, str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
