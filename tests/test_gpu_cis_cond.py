"""GPU: the conditional cis scan (aq_prep_cis_cond, csrc/aq_ciscond_kernels.h, csrc/aq_screen_tile.h) against the long-double restatement of
tests/ciscond_util.py run on the handle's own matrices, against the plain scan of the same handle, which every trait with an
empty list must equal to the bit, and cis_independent() against the same loop run on the reference scan.

Shapes (n, p, q): (20, 5, 2) and (50, 17, 5) below one tile; (333, 257, 33) odd n, nothing a multiple of 16; (257, 130, 130) one
past 64 both ways, and under `all` two trait tiles whose longest lists differ; (130, 1000, 20) many predictor items per trait
tile.  Each with the window patterns `all` and `band` of ciscond_util.windows and with the longest list 1, 2 and 4, so that
every instance of the tile kernel runs; the lists of ciscond_util.case hold every length 0 ... max within one trait tile."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ciscond_util as CU
from tests import mscreen_util as MU

pytestmark = pytest.mark.gpu

SHAPES = [(20, 5, 2), (50, 17, 5), (333, 257, 33), (257, 130, 130), (130, 1000, 20)]
RUNS = [(s, w, k) for s in SHAPES for w in CU.PATTERNS for k in (1, 2, 4)]


def _id(run):
    (n, p, q), pattern, k = run
    return f"{n}x{p}x{q}-{pattern}-k{k}"


@functools.lru_cache(maxsize=None)
def _case(shape, max_k):
    """Once per (shape, longest list), shared and left unchanged: the raw inputs, the lists, and the handle's own matrices."""
    from atlasqtl_amd import prepare as P
    n, p, q = shape
    X, Y, cond = CU.case(n, p, q, max_k)
    prep = P.prepare_on_device(Y, X)[0]
    try:
        assert prep.p == p
        Xs, Yc = prep.X_host(), prep.Y.copy()
    finally:
        prep.close()
    for v in (X, Y, Xs, Yc):
        v.setflags(write=False)
    return dict(X=X, Y=Y, cond=cond, Xs=Xs, Yc=Yc)


def _handle(case):
    from atlasqtl_amd import prepare as P
    return P.prepare_on_device(case["Y"], case["X"])[0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _table(out):
    return set(zip(MU.int_list(out["snp"]), MU.int_list(out["trait"]), MU.int_list(_bits(out["r"]))))


def _rows(out):
    return set(zip(MU.int_list(out["snp"]), MU.int_list(out["trait"])))


@pytest.mark.parametrize("run", RUNS, ids=[_id(r) for r in RUNS])
def test_scan_against_long_double_and_the_plain_scan(run):
    shape, pattern, max_k = run
    n, p, q = shape
    case = _case(shape, max_k)
    cond = case["cond"]
    lo, hi = CU.windows(pattern, p, q)
    ref = CU.reference(case["Xs"], case["Yc"], lo, hi, cond)
    # the reference first: no pair near the 1e-10 rule, and what ciscond_util.case plants is there
    assert CU.thresholds_are_clear(ref)
    inside, defined, r_ref, bound = ref["inside"], ref["defined"], ref["r"], ref["bound"]
    assert max(len(c) for c in cond) == max_k and lo[0] <= 3 < hi[0] and cond[0][0] == 3
    assert inside[3, 0] and not defined[3, 0] and ref["ratio"][3, 0] < 1e-13          # a conditioning variant in its own window
    if q > 1 and max_k >= 2:                                   # a linear combination of the two conditioning variants of trait 1
        assert cond[1] == [0, 1] and inside[CU.LINCOMB, 1] and not defined[CU.LINCOMB, 1] and ref["ratio"][CU.LINCOMB, 1] < 1e-13
    if q > 2 and max_k == 4:                                   # the third entry is collinear with the first two: dropped
        assert cond[2] == [0, 1, CU.LINCOMB] and ref["k_eff"][2] == 2
    if q > 3:                                                  # a conditioning variant outside the window
        assert cond[3] == [0] and inside[0, 3] == (pattern == "all") and ref["k_eff"][3] == 1
    M = int(inside.sum())
    prep = _handle(case)
    try:
        full = prep.cis_conditional(lo, hi, cond, np.zeros(q), M)
        again = prep.cis_conditional(lo, hi, cond, np.zeros(q), M)
        plain = prep.cis(lo, hi, np.zeros(q), M)
        r64 = np.asarray(r_ref, dtype=np.float64)
        cut = MU.clear_cutoffs(r64)
        assert MU.cutoffs_are_clear(r64, cut)
        sel = prep.cis_conditional(lo, hi, cond, cut, M)
        count = prep.cis_conditional(lo, hi, cond, cut, 0)
        short = prep.cis_conditional(lo, hi, cond, cut, sel["n_pairs"] - 1) if sel["n_pairs"] >= 1 else None
    finally:
        prep.close()
    # 1. cutoff 0: exactly the defined in-window pairs, every r within the bound; the undefined sets are equal
    want = set(zip(*(MU.int_list(a) for a in np.nonzero(inside & defined))))
    assert full["n_pairs"] == len(want) and _rows(full) == want
    s, t = full["snp"], full["trait"]
    err = np.abs(full["r"].astype(MU.LD) - r_ref[s, t])
    ratio = float(np.max(err / bound[s, t])) if err.size else 0.0
    print(f"{_id(run)}: {len(want)} of {M} in-window pairs defined; worst |r - reference| / bound {ratio:.2e}, worst error "
          f"{float(err.max()) if err.size else 0.0:.2e}; KC {full['plan']['kc']}, W {full['plan']['n_items']}")
    assert (err <= bound[s, t]).all()
    np.testing.assert_array_equal(full["n_undef"], (inside & ~defined).sum(axis=0))
    np.testing.assert_array_equal(full["k_eff"], ref["k_eff"])
    has_window = hi > lo
    assert full["plan"]["max_k"] == max((len(c) for c, w in zip(cond, has_window) if w), default=0)
    assert full["plan"]["kc"] == {0: 0, 1: 1, 2: 2, 3: 4, 4: 4}[full["plan"]["max_k"]] and full["plan"]["streams"] == 1 + full["plan"]["kc"]
    # 2. the best predictor, where the reference's is clear of the runner-up by the bound
    bs, clear = CU.best(ref)
    assert clear.any()
    np.testing.assert_array_equal(full["best_snp"][clear], bs[clear])
    assert (full["best_snp"][~has_window] == -1).all() and np.isnan(full["best_r"][~has_window]).all()
    got = {(int(a), int(b)): float(c) for a, b, c in zip(s, t, full["r"])}
    for tr in np.nonzero(full["best_snp"] >= 0)[0]:
        assert _bits(full["best_r"][tr]) == _bits(got[(int(full["best_snp"][tr]), int(tr))])
    # 3. clear cutoffs: the reference's selection; cap = 0 only counts; beyond cap n_pairs is still the full count
    r2 = np.where(defined, r64 * r64, -1.0)
    want_sel = set(zip(*(MU.int_list(a) for a in np.nonzero(inside & defined & (r2 >= cut[None, :])))))
    assert sel["n_pairs"] == len(want_sel) and _rows(sel) == want_sel
    assert count["n_pairs"] == len(want_sel) and count["snp"].size == 0
    if short is not None:
        assert short["n_pairs"] == len(want_sel) and short["snp"].size == len(want_sel) - 1 and _rows(short) < want_sel
    for key in ("best_snp", "best_r", "n_undef", "k_eff"):
        assert sel[key].tobytes() == full[key].tobytes() == count[key].tobytes(), key
    # 4. two calls: the same bits everywhere, the same set of rows
    for key in ("best_snp", "best_r", "n_undef", "k_eff"):
        assert full[key].tobytes() == again[key].tobytes(), key
    assert again["n_pairs"] == full["n_pairs"] and again["plan"] == full["plan"] and _table(again) == _table(full)
    # 5. a trait with an empty list: the plain scan of the same handle to the bit, whatever instance the other traits force
    empty = np.asarray([len(c) == 0 for c in cond])
    if q >= 20:
        assert (empty & has_window).any() and (~empty & has_window).any()
    assert {row for row in _table(full) if empty[row[1]]} == {row for row in _table(plain) if empty[row[1]]}
    np.testing.assert_array_equal(full["best_snp"][empty], plain["best_snp"][empty])
    assert _bits(full["best_r"][empty]).tobytes() == _bits(plain["best_r"][empty]).tobytes()
    np.testing.assert_array_equal(full["n_undef"][empty], plain["n_undef"][empty])


def test_no_list_at_all_is_the_plain_scan():
    shape = (257, 130, 130)
    n, p, q = shape
    case = _case(shape, 1)
    lo, hi = CU.windows("band", p, q)
    prep = _handle(case)
    try:
        a = prep.cis_conditional(lo, hi, [[] for _ in range(q)], np.zeros(q), n * q)
        b = prep.cis(lo, hi, np.zeros(q), n * q)
    finally:
        prep.close()
    assert a["plan"]["kc"] == 0 and a["plan"]["streams"] == 1 and not a["k_eff"].any()
    assert _table(a) == _table(b) and a["n_pairs"] == b["n_pairs"]
    for key in ("best_snp", "best_r", "n_undef"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_errors_come_before_any_launch():
    """The documented refusals, through the Python layer and through the C ABI on a real handle."""
    from atlasqtl_amd import _lib
    from atlasqtl_amd.prepare import AtlasqtlError
    shape = (50, 17, 5)
    n, p, q = shape
    case = _case(shape, 2)
    lo, hi = CU.windows("all", p, q)
    L = _lib.lib()
    outs = [None] * 9
    cut = np.zeros(q)

    def raw(prep, lists):
        ptr = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int32)
        idx = np.asarray([v for c in lists for v in c] + [0], dtype=np.int32)
        rc = L.aq_prep_cis_cond(prep.handle, _lib.as_ip(lo), _lib.as_ip(hi), _lib.as_ip(ptr), _lib.as_ip(idx), _lib.as_dp(cut), 0, *outs)
        return rc, L.aq_last_error()

    prep = _handle(case)
    try:
        live = L.aq_debug_live_device_bytes()
        for lists, word, pyword in (([[3, 4, 5, 6, 7]] + [[]] * (q - 1), b"at most 4", "at most 4"),
                                    ([[3, 4, 3]] + [[]] * (q - 1), b"more than once", "more than once"),
                                    ([[]] * (q - 1) + [[p]], b"outside [0, 17)", r"\[0, 17\)"),
                                    ([[-1]] + [[]] * (q - 1), b"outside [0, 17)", r"\[0, 17\)")):
            rc, msg = raw(prep, lists)
            assert rc == 1 and word in msg and b"aq_prep_cis_cond" in msg, msg
            with pytest.raises(AtlasqtlError, match=pyword):
                prep.cis_conditional(lo, hi, lists, cut, 0)
            assert L.aq_debug_live_device_bytes() == live          # nothing was allocated, so nothing was launched
        bad = np.array([0, 2, 1, 1, 1, 1], dtype=np.int32)         # decreasing offsets
        idx = np.zeros(4, dtype=np.int32)
        assert L.aq_prep_cis_cond(prep.handle, _lib.as_ip(lo), _lib.as_ip(hi), _lib.as_ip(bad), _lib.as_ip(idx), _lib.as_dp(cut), 0,
                                  *outs) == 1
        assert b"decreases" in L.aq_last_error()
        assert L.aq_prep_cis_cond(prep.handle, _lib.as_ip(lo), _lib.as_ip(hi), None, _lib.as_ip(idx), _lib.as_dp(cut), 0, *outs) == 1
        with pytest.raises(AtlasqtlError, match="one list per trait"):
            prep.cis_conditional(lo, hi, [[]] * (q + 1), cut, 0)
        # the timing entry on a small shape: both figures, and the plan it used
        ptr = np.concatenate([[0], np.cumsum([len(c) for c in case["cond"]])]).astype(np.int32)
        idx = np.asarray([v for c in case["cond"] for v in c] + [0], dtype=np.int32)
        ms, plan = (C.c_double(0.0), C.c_double(0.0)), _lib.AqCiscondPlan()
        _lib.check(L.aq_prep_cis_cond_time(prep.handle, _lib.as_ip(lo), _lib.as_ip(hi), _lib.as_ip(ptr), _lib.as_ip(idx), 1,
                                           C.byref(ms[0]), C.byref(ms[1]), C.byref(plan)), "aq_prep_cis_cond_time")
        assert ms[0].value > 0 and ms[1].value > 0 and plan.kc == 2 and plan.cis.n_items == 1
    finally:
        prep.close()
    # Y with missing values: refused by the Python layer, and by the library under its own name
    Y = np.array(case["Y"])
    Y[3, 1] = np.nan
    from atlasqtl_amd import prepare as P
    prep = P.prepare_on_device(Y, case["X"])[0]
    try:
        with pytest.raises(AtlasqtlError, match="missing values"):
            prep.cis_conditional(lo, hi, case["cond"], cut, 0)
        rc, msg = raw(prep, case["cond"])
        assert rc == 3 and b"aq_prep_cis_cond: Y has missing values" in msg
    finally:
        prep.close()


def test_cis_screen_with_condition_on():
    """The public entry: names and indices, the reduced df, and the table against the reference at its clear cutoffs."""
    import atlasqtl_amd as A
    shape = (50, 17, 5)
    n, p, q = shape
    case = _case(shape, 4)
    cond = case["cond"]
    chrom, pos = ["1"] * p, np.arange(p)
    plain = A.cis_screen(case["Y"], case["X"], ["1"] * q, np.full(q, 8), window=100, snp_chrom=chrom, snp_pos=pos, p_value=1.0)
    names = plain["names_x"]
    by_name = {plain["names_y"][t]: [names[v] for v in c] for t, c in enumerate(cond) if c}
    res = A.cis_screen(case["Y"], case["X"], ["1"] * q, np.full(q, 8), window=100, snp_chrom=chrom, snp_pos=pos, p_value=1.0,
                       condition_on=by_name)
    res2 = A.cis_screen(case["Y"], case["X"], ["1"] * q, np.full(q, 8), window=100, snp_chrom=chrom, snp_pos=pos, p_value=1.0,
                        condition_on=cond)
    ref = CU.reference(case["Xs"], case["Yc"], np.zeros(q, dtype=int), np.full(q, p), cond)
    assert res["condition_on"] == cond == res2["condition_on"]
    np.testing.assert_array_equal(res["k_eff"], ref["k_eff"])
    np.testing.assert_array_equal(res["df"], n - 2 - ref["k_eff"])
    assert "condition_on" not in plain and (plain["df"] == n - 2).all()
    a = res["assoc"]
    assert a["n_pairs"] == int(ref["defined"].sum()) and res2["assoc"]["r"].tobytes() == a["r"].tobytes()
    np.testing.assert_array_equal(a["df"], res["df"][a["trait"]])
    err = np.abs(a["r"].astype(MU.LD) - ref["r"][a["snp"], a["trait"]])
    assert (err <= ref["bound"][a["snp"], a["trait"]]).all()
    np.testing.assert_array_equal(res["n_undefined"], (~ref["defined"]).sum(axis=0))
    with pytest.raises(A.AtlasqtlError, match="permutations"):
        A.cis_screen(case["Y"], case["X"], ["1"] * q, np.full(q, 8), window=100, snp_chrom=chrom, snp_pos=pos, condition_on=cond,
                     permutations=10)


def test_cis_independent_on_a_planted_cohort():
    """cis_independent() returns the signal sets of the same loop run on the long-double scan of the handle's own matrices,
    with the device's eGenes and thresholds; before that, every accept / reject decision of the reference run clears its
    threshold by a factor of 10 in p (the seed of ciscond_util.COHORT was chosen, with numpy alone, so that it does)."""
    import atlasqtl_amd as A
    from atlasqtl_amd import prepare as P
    c, co = CU.COHORT, CU.cohort()
    res = A.cis_independent(co["Y"], co["X"], co["trait_chrom"], co["trait_start"], window=c["window"], snp_chrom=co["snp_chrom"],
                            snp_pos=co["snp_pos"], fdr=c["fdr"], permutations=c["permutations"], max_signals=5)
    prep = P.prepare_on_device(co["Y"], co["X"])[0]
    try:
        assert prep.p == c["p"]
        Xs, Yc = prep.X_host(), prep.Y.copy()
    finally:
        prep.close()
    prim = res["primary"]
    lo, hi = prim["window"]
    thr, egene = res["threshold"], res["egene"]
    kinds = np.asarray(co["kinds"])
    assert egene[kinds != "null"].all() and egene.sum() >= 20
    log = []
    want = A.independent_signals_(CU.numpy_scan(Xs, Yc, lo, hi, 0, log), prim["best_snp"], prim["best_pvalue"],
                                  np.where(egene, thr, np.nan), 5)
    assert len(log) >= 3 and CU.decisions_are_clear(log, thr, 10.0)
    np.testing.assert_array_equal(res["n_signals"], want["n_signals"])
    assert res["forward"] == want["forward"]
    sig = res["signals"]
    got = [[] for _ in range(c["q"])]
    for i in range(sig["trait"].size):
        got[int(sig["trait"][i])].append((int(sig["rank"][i]), int(sig["snp"][i]), int(sig["forward_snp"][i])))
    assert got == [[(s["rank"], s["snp"], s["forward_snp"]) for s in w] for w in want["signals"]]
    flat = [s for w in want["signals"] for s in w]
    np.testing.assert_allclose(sig["pvalue"], [s["pvalue"] for s in flat], rtol=1e-6)
    # what was planted is what comes out: two signals, one signal despite the proxies, none for a gene that is no eGene
    for t, kind in enumerate(kinds):
        found = sorted(s[1] for s in got[t])
        if kind == "two":
            assert found == sorted(co["planted"][t]), (t, found)
        elif kind == "proxy":
            j = co["planted"][t][0]
            assert len(found) == 1 and found[0] in (j, j - 2, j + 3, j + 11), (t, found)
        elif kind == "weak":
            assert found == co["planted"][t], (t, found)
        elif not egene[t]:
            assert found == []
    n_forward = np.asarray([len(f) for f in res["forward"]])
    assert (sig["df"] == c["n"] - 2 - (n_forward[sig["trait"]] - 1)).all()
