"""The host side of the conditional cis scan, without a GPU: the ABI entries and the mirrored plan struct; the planner through
aq_ciscond_plan_query against plans computed by hand; the condition_on argument of cis_screen(); the refusals that come before
the first device call; the forward-backward loop independent_signals_ against a numpy scan; the long-double reference of
tests/ciscond_util.py against an ordinary least-squares fit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from atlasqtl_amd import _lib
from atlasqtl_amd import cis as CIS
from atlasqtl_amd import cis_condition as CC
from atlasqtl_amd import cis_lists as CL
from atlasqtl_amd.prepare import AtlasqtlError
from tests import ciscond_util as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aq_ciscond_plan_query", "aq_prep_cis_cond", "aq_prep_cis_cond_time")


def test_header_binding_and_library_agree(hiplib):
    import atlasqtl_amd as A
    txt = open(os.path.join(ROOT, "include", "atlasqtl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "aq_prep_handle": C.c_void_p, "const int32_t *": _lib.ip, "int32_t *": _lib.ip,
             "const double *": _lib.dp, "double *": _lib.dp, "int64_t *": C.POINTER(C.c_int64),
             "aq_ciscond_plan *": C.POINTER(_lib.AqCiscondPlan)}
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and hasattr(hiplib, name), name
        args = re.search(r"\bint " + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        types = [re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip() for a in args.split(",")]
        assert [ctype[t] for t in types] == list(_lib.SYMBOLS[name][1]), name
        assert _lib.SYMBOLS[name][0] is C.c_int
    body = re.search(r"typedef struct aq_ciscond_plan \{(.*?)\} aq_ciscond_plan;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            typ, names = decl.split(None, 1)
            fields += [(nm.strip(), {"int32_t": C.c_int32, "int64_t": C.c_int64, "aq_cis_plan": _lib.AqCisPlan}[typ])
                       for nm in names.split(",")]
    assert fields == list(_lib.AqCiscondPlan._fields_)
    assert C.sizeof(_lib.AqCiscondPlan) == C.sizeof(_lib.AqCisPlan) + 4 * 4 + 2 * 8
    for name in ("cis_independent", "independent_signals_"):
        assert name in A.__all__ and getattr(A, name) is getattr(CC, name)


# ---- the planner ----
def _query(hiplib, n, p1, q, lo, hi, k, ncu=256):
    lo32, hi32 = np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)
    ptr = np.concatenate([[0], np.cumsum(k)]).astype(np.int32)
    pl = _lib.AqCiscondPlan()
    rc = hiplib.aq_ciscond_plan_query(n, p1, q, ncu, _lib.as_ip(lo32), _lib.as_ip(hi32), _lib.as_ip(ptr), C.byref(pl))
    return rc, pl


def _lds(kc):
    """(2 + KC) panels of 64 rows of 18 doubles; two columns of (double, int) candidates; per trait two doubles and four ints."""
    return (2 + kc) * 64 * 18 * 8 + 2 * 64 * 12 + 64 * 32


@pytest.mark.parametrize("max_k, kc", [(0, 0), (1, 1), (2, 2), (3, 4), (4, 4)])
def test_plan_by_hand(hiplib, max_k, kc):
    n, p1, q = 1000, 5000, 130
    lo = np.arange(q) * 30
    hi = lo + 100
    k = np.arange(q) % (max_k + 1)
    rc, pl = _query(hiplib, n, p1, q, lo, hi, k)
    assert rc == 0
    assert (pl.kc, pl.max_k, pl.streams) == (kc, max_k, 1 + kc)
    assert pl.lds_bytes == (_lds(kc) if kc else pl.cis.lds_bytes) and pl.lds_bytes <= 65536
    assert _lds(4) == 58880 and pl.cis.lds_bytes == _lds(0)
    assert pl.yo_bytes == 8 * q * n and pl.qo_bytes == kc * 8 * q * n
    # the cis plan of the same windows, complete Y, no permutations
    cp = _lib.AqCisPlan()
    assert hiplib.aq_cis_plan_query(n, p1, q, 0, 256, _lib.as_ip(lo.astype(np.int32)), _lib.as_ip(hi.astype(np.int32)), 0, C.byref(cp)) == 0
    assert bytes(pl.cis) == bytes(cp) and cp.q_active == q and cp.trait_tiles == 3


def test_plan_counts_only_the_traits_with_a_window(hiplib):
    """A trait with an empty window costs no work item, no panel, and its list does not choose the instance."""
    n, p1, q = 100, 500, 6
    lo = np.array([0, 10, 50, 50, 7, 400])
    hi = np.array([40, 90, 50, 120, 7, 500])
    rc, pl = _query(hiplib, n, p1, q, lo, hi, [1, 0, 4, 2, 3, 0])
    assert rc == 0 and (pl.kc, pl.max_k) == (2, 2) and pl.cis.q_active == 4
    assert pl.yo_bytes == 8 * 4 * n and pl.qo_bytes == 2 * 8 * 4 * n
    assert pl.cis.n_items == -(-500 // 64)                    # one trait tile over [0, 500)
    rc, pl = _query(hiplib, n, p1, q, lo, lo, [1, 0, 4, 2, 3, 0])
    assert rc == 0 and (pl.kc, pl.max_k, pl.cis.n_items, pl.qo_bytes, pl.yo_bytes) == (0, 0, 0, 0, 8 * n)


def test_plan_refusals(hiplib):
    n, p1, q = 100, 500, 4
    lo, hi = np.zeros(q), np.full(q, 500)
    rc, pl = _query(hiplib, n, p1, q, lo, hi, [0, 5, 0, 0])
    assert rc == 3 and b"trait 1 conditions on 5 variants" in hiplib.aq_last_error() and pl.kc == 0 and pl.cis.tile == 0
    # 4 GiB: 1 + KC panels of 8 q_active n bytes
    n, q = 80000, 2000
    lo, hi = np.zeros(q), np.full(q, 10)
    assert 5 * 8 * q * n > 4 << 30 >= 3 * 8 * q * n
    assert _query(hiplib, n, 10, q, lo, hi, np.full(q, 2))[0] == 0
    rc, _ = _query(hiplib, n, 10, q, lo, hi, np.full(q, 3))
    assert rc == 3 and b"exceed 4 GiB" in hiplib.aq_last_error()
    # offsets and windows
    pl = _lib.AqCiscondPlan()
    lo32, hi32 = np.zeros(2, dtype=np.int32), np.full(2, 5, dtype=np.int32)
    for ptr, word in (([1, 1, 1], b"cond_ptr[0] must be 0"), ([0, 2, 1], b"decreases at trait 1")):
        ptr = np.asarray(ptr, dtype=np.int32)
        assert hiplib.aq_ciscond_plan_query(50, 10, 2, 256, _lib.as_ip(lo32), _lib.as_ip(hi32), _lib.as_ip(ptr), C.byref(pl)) == 1
        assert word in hiplib.aq_last_error()
    ptr = np.zeros(3, dtype=np.int32)
    assert hiplib.aq_ciscond_plan_query(50, 10, 2, 256, _lib.as_ip(lo32), _lib.as_ip(hi32), None, C.byref(pl)) == 1
    assert hiplib.aq_ciscond_plan_query(50, 10, 2, 256, _lib.as_ip(lo32), _lib.as_ip(hi32), _lib.as_ip(ptr), None) == 1
    assert hiplib.aq_ciscond_plan_query(50, 4, 2, 256, _lib.as_ip(lo32), _lib.as_ip(hi32), _lib.as_ip(ptr), C.byref(pl)) == 1
    assert b"outside [0, 4]" in hiplib.aq_last_error()
    # the entries refuse NULL arguments before they look at the handle
    d = C.c_double(0.0)
    assert hiplib.aq_prep_cis_cond(None, _lib.as_ip(lo32), _lib.as_ip(hi32), _lib.as_ip(ptr), _lib.as_ip(ptr), _lib.as_dp(np.zeros(2)), 0,
                                   *([None] * 9)) == 1
    assert b"aq_prep_cis_cond: NULL handle" in hiplib.aq_last_error()
    assert hiplib.aq_prep_cis_cond(None, _lib.as_ip(lo32), _lib.as_ip(hi32), _lib.as_ip(ptr), _lib.as_ip(ptr), None, 0, *([None] * 9)) == 1
    assert b"NULL r2_cut" in hiplib.aq_last_error()
    assert hiplib.aq_prep_cis_cond_time(None, _lib.as_ip(lo32), _lib.as_ip(hi32), _lib.as_ip(ptr), _lib.as_ip(ptr), 0, C.byref(d), C.byref(d),
                                        None) == 1
    assert b"reps >= 1" in hiplib.aq_last_error()


# ---- condition_on ----
def test_condition_on_parsing():
    nx, ny = [f"rs{j}" for j in range(10)], ["geneA", "geneB", "geneC"]
    f = CL.condition_lists
    assert f({"geneB": ["rs3", 7], 2: "rs0"}, nx, ny) == [[], [3, 7], [0]]
    assert f({0: 4}, nx, ny) == [[4], [], []]
    assert f([[1, 2, 3, 4], [], ["rs9"]], nx, ny) == [[1, 2, 3, 4], [], [9]]
    assert f([np.array([5, 6]), (), np.int64(2)], nx, ny) == [[5, 6], [], [2]]
    assert f({}, nx, ny) == [[], [], []]
    for bad, word in (([[0]], "one list per trait"), ({"geneZ": [1]}, "geneZ"), ({"geneA": ["rs77"]}, "rs77"), ({3: [1]}, "outside"),
                      ({0: [10]}, "outside"), ({0: [-1]}, "outside"), ({0: [1, 2, 3, 4, 5]}, "at most 4"), ({0: [1, "rs1"]}, "more than once"),
                      ({0: [1.5]}, "name or its index"), ({0: [True]}, "name or its index"), ("geneA", "one list per trait"),
                      (7, "one list per trait"), ({"geneA": [1], 0: [2]}, "twice")):
        with pytest.raises(AtlasqtlError, match=word):
            f(bad, nx, ny)


def test_condition_on_refusals_come_before_the_device():
    """permutations= and Y with NaN: refused by cis_screen() before anything is prepared (no device here: a device call would
    raise another error)."""
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((30, 8)), rng.standard_normal((30, 2))
    kw = dict(trait_chrom=["1", "1"], trait_start=[3, 4], window=10, snp_chrom=["1"] * 8, snp_pos=np.arange(8))
    with pytest.raises(AtlasqtlError, match="condition_on= together with permutations="):
        CIS.cis_screen(Y, X, condition_on=[[0], []], permutations=10, **kw)
    Yn = Y.copy()
    Yn[4, 1] = np.nan
    with pytest.raises(AtlasqtlError, match="complete Y"):
        CIS.cis_screen(Yn, X, condition_on=[[0], []], **kw)
    for bad in (0, 6, 2.5, None):
        with pytest.raises(AtlasqtlError, match="max_signals"):
            CC.cis_independent(Y, X, max_signals=bad, permutations=10, **kw)
    with pytest.raises(AtlasqtlError, match="permutations are required"):
        CC.cis_independent(Y, X, permutations=None, **kw)


# ---- the reference itself ----
def test_reference_is_the_t_statistic_of_the_joint_regression():
    """r of the definition is the partial correlation: t = r sqrt(df / (1 - r^2)) is the t statistic of x_s in the least-squares
    fit of y on (x_s, the list), with df = n - 2 - k_eff; the drop rule and the undefined pairs are as planted."""
    n, p, q = 50, 17, 5
    X, Y, cond = CU.case(n, p, q, 4)
    Xs, Yc = CU.prepared(X, Y)
    lo, hi = CU.windows("all", p, q)
    ref = CU.reference(Xs, Yc, lo, hi, cond)
    assert CU.thresholds_are_clear(ref)
    assert list(ref["k_eff"]) == [4, 2, 2, 1, 0] and cond[2] == [0, 1, CU.LINCOMB]
    assert not ref["defined"][3, 0] and not ref["defined"][CU.LINCOMB, 1] and not ref["defined"][0, 3]
    for t in range(q):
        kept = CU.basis(np.asarray(Xs, dtype=CU.LD), cond[t])[1]
        for s in np.nonzero(ref["defined"][:, t])[0]:
            A = np.column_stack([Xs[:, s]] + [Xs[:, c] for c in kept])
            beta, res = np.linalg.lstsq(A, Yc[:, t], rcond=None)[:2]
            df = n - 2 - len(kept)
            se = np.sqrt(res[0] / df * np.linalg.inv(A.T @ A)[0, 0])
            r = float(ref["r"][s, t])
            np.testing.assert_allclose(r * np.sqrt(df / (1 - r * r)), beta[0] / se, rtol=1e-9)
    assert float(np.nanmax(np.asarray(ref["bound"], dtype=np.float64))) < 1e-10


# ---- the forward-backward loop against a numpy scan ----
def _toy(seed=4):
    """n = 400, p = 40, six genes with every window [0, 40), on independent predictors but for two proxies:
      gene 0: y = 0.6 x_5 + 0.5 x_20            two signals
      gene 1: y = 0.6 x_10, x_11 and x_12 proxies of x_10 at r^2 ~ 0.8   one signal
      gene 3: y = 0.5 x_1 + 0.5 x_2 + 0.5 x_3 + 0.5 x_4     four signals, cut by max_signals
      genes 2, 4: noise, no eGenes (the test gives them the threshold NaN)
      gene 5: noise, but handed a threshold: an eGene whose lead stays alone."""
    rng = np.random.default_rng(seed)
    n, p, q = 400, 40, 6
    X = rng.standard_normal((n, p))
    for j in (11, 12):
        X[:, j] = np.sqrt(0.8) * X[:, 10] + np.sqrt(0.2) * X[:, j]
    Y = rng.standard_normal((n, q))
    Y[:, 0] += 0.6 * X[:, 5] + 0.5 * X[:, 20]
    Y[:, 1] += 0.6 * X[:, 10]
    Y[:, 3] += 0.5 * (X[:, 1] + X[:, 2] + X[:, 3] + X[:, 4])
    return CU.prepared(X, Y)


def _primary(Xs, Yc, lo, hi):
    q = Yc.shape[1]
    out = CU.numpy_scan(Xs, Yc, lo, hi)([[] for _ in range(q)], np.ones(q, dtype=bool))
    return out["best_snp"], out["best_pvalue"]


def test_independent_signals_loop():
    Xs, Yc = _toy()
    n, p = Xs.shape
    q = Yc.shape[1]
    lo, hi = np.zeros(q, dtype=int), np.full(q, p)
    bs, bp = _primary(Xs, Yc, lo, hi)
    thr = np.full(q, 1e-5)
    thr[[2, 4]] = np.nan
    log = []
    out = CC.independent_signals_(CU.numpy_scan(Xs, Yc, lo, hi, 0, log), bs, bp, thr, 5)
    assert CU.decisions_are_clear(log, np.where(np.isnan(thr), 1.0, thr))
    assert sorted(out["forward"][0]) == [5, 20] and [s["snp"] for s in out["signals"][0]] == out["forward"][0]
    assert out["forward"][1] == [10] and out["n_signals"][1] == 1                      # the proxies add nothing
    assert sorted(out["forward"][3]) == [1, 2, 3, 4] and out["n_signals"][3] == 4
    assert out["forward"][4] == [] and out["signals"][4] == [] and out["forward"][5] == [int(bs[5])] and out["n_signals"][5] == 1
    assert [s["rank"] for s in out["signals"][3]] == [1, 2, 3, 4]
    # every scan passes the inactive genes with an empty list and marks them inactive; gene 4 is never active
    for cond, active, _, _ in log:
        assert not active[4] and all(not c for c, a in zip(cond, active) if not a)
    # forward rounds: all active genes together, each conditioned on its own variants so far
    assert [sorted(len(c) for c in cond if c) for cond, _, _, _ in log[:2]] == [[1, 1, 1, 1], [2, 2]]
    assert list(log[0][1]) == [True, True, False, True, False, True] and list(log[1][1]) == [True, False, False, True, False, False]
    # backward rounds: genes with at least two signals, the forward set minus signal i
    back = log[-4:]
    for i, (cond, active, _, _) in enumerate(back):
        assert cond[3] == out["forward"][3][:i] + out["forward"][3][i + 1:]
        assert bool(active[0]) == (i < 2) and not active[1] and not active[5]
    # the cap: with max_signals = 2 gene 3 stops at two signals, and no scan conditions on more than one variant
    log2 = []
    capped = CC.independent_signals_(CU.numpy_scan(Xs, Yc, lo, hi, 0, log2), bs, bp, thr, 2)
    assert capped["n_signals"][3] == 2 and capped["forward"][3] == out["forward"][3][:2]
    assert max(len(c) for cond, _, _, _ in log2 for c in cond) == 1
    one = CC.independent_signals_(lambda cond, active: pytest.fail("no scan with max_signals = 1"), bs, bp, thr, 1)
    assert list(one["n_signals"]) == [1, 1, 0, 1, 0, 1]
    for bad in (0, 6, 1.5):
        with pytest.raises(AtlasqtlError, match="max_signals"):
            CC.independent_signals_(None, bs, bp, thr, bad)


def test_backward_pass_drops_and_replaces():
    """A scripted scan: the forward pass gives gene 0 the variants [7, 3, 9]; in the backward pass signal 0 is confirmed with
    another lead (8 in the place of 7), signal 1 fails its threshold and is dropped, signal 2 stays.  Gene 1 has one signal and
    is not scanned backward."""
    thr = np.array([1e-4, 1e-4])
    script = {((7,), 0): (3, 1e-8), ((7, 3), 0): (9, 1e-6), ((7, 3, 9), 0): (5, 0.2), ((4,), 1): (-1, np.nan),
              ((3, 9), 0): (8, 1e-9), ((7, 9), 0): (3, 1e-3)}
    calls = []

    def scan(cond, active):
        calls.append(([list(c) for c in cond], [bool(a) for a in active]))
        bs, pv = np.full(2, -1), np.full(2, np.nan)
        for t in np.nonzero(active)[0]:
            bs[t], pv[t] = script[(tuple(cond[t]), int(t))]
        return dict(best_snp=bs, best_pvalue=pv)

    out = CC.independent_signals_(scan, np.array([7, 4]), np.array([1e-12, 1e-7]), thr, 5)
    assert out["forward"] == [[7, 3, 9], [4]]
    assert [(s["rank"], s["snp"], s["forward_snp"]) for s in out["signals"][0]] == [(1, 8, 7), (3, 9, 9)]
    assert [(s["rank"], s["snp"], s["forward_snp"], s["pvalue"]) for s in out["signals"][1]] == [(1, 4, 4, 1e-7)]
    assert list(out["n_signals"]) == [2, 1]
    assert [c for c, _ in calls] == [[[7], [4]], [[7, 3], []], [[7, 3, 9], []], [[3, 9], []], [[7, 9], []], [[7, 3], []]]
    assert [a for _, a in calls] == [[True, True]] + [[True, False]] * 5
