"""GPU: the interaction cis scan (aq_prep_cis_int, csrc/aq_cisint_kernels.h, aq_ms_tile_loop_x2 in csrc/aq_screen_tile.h) against the
long-double restatement of tests/cisint_util.py run on the handle's own matrices, and cis_screen(interaction=) against the same
reference run through the host statistics.

Shapes (n, p, q): (20, 5, 2) and (50, 17, 5) below one tile; (333, 257, 33) odd n, which takes the loads that are not 16-byte
ones and a ragged last chunk; (257, 130, 130) one past 64 both ways, two trait tiles; (130, 1000, 20) many predictor items per
trait tile.  Over them the window patterns `all` and `band` of ciscond_util.windows, d = 0 and 3 covariates and a binary and a
continuous e: every shape runs four of the eight combinations, a half fraction in which every two factors meet in all four
ways, and neighbouring shapes run complementary halves.

There is no tolerance: every r must lie within the elementwise bound that cisint_util.reference derives (first order in 2^-53,
every length-n sum in any order, the cancellations in num, Vw and S'' carried), and the worst ratio is printed."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import cisint_util as CI
from tests import mscreen_util as MU

pytestmark = pytest.mark.gpu

SHAPES = [(20, 5, 2), (50, 17, 5), (333, 257, 33), (257, 130, 130), (130, 1000, 20)]
HALVES = ([("all", 0, "binary"), ("all", 3, "continuous"), ("band", 0, "continuous"), ("band", 3, "binary")],
          [("all", 0, "continuous"), ("all", 3, "binary"), ("band", 0, "binary"), ("band", 3, "continuous")])
RUNS = [(s, w, d, k) for i, s in enumerate(SHAPES) for (w, d, k) in HALVES[i % 2]]


def _id(run):
    (n, p, q), pattern, d, kind = run
    return f"{n}x{p}x{q}-{pattern}-d{d}-{kind}"


@functools.lru_cache(maxsize=None)
def _case(shape, d, kind):
    """Once per (shape, d, e), shared and left unchanged: the raw inputs, the handle's own matrices, and the basis and the
    multiplier that the library is given."""
    from atlasqtl_amd import cis_interaction as CIS
    from atlasqtl_amd import prepare as P
    n, p, q = shape
    X, Y, Z, e = CI.case(n, p, q, d, kind)
    prep = P.prepare_on_device(Y, X, covariates=Z)[0]
    try:
        assert prep.p == p and prep.n_cov == d
        Xs, Yc = prep.X_host(), prep.Y.copy()
    finally:
        prep.close()
    B, m = CIS.interaction_basis(e, Z, n, d)
    for v in (X, Y, Xs, Yc, e, B, m) + (() if Z is None else (Z,)):
        v.setflags(write=False)
    return dict(X=X, Y=Y, Z=Z, e=e, Xs=Xs, Yc=Yc, B=B, m=m)


@functools.lru_cache(maxsize=None)
def _reference(shape, pattern, d, kind):
    n, p, q = shape
    case = _case(shape, d, kind)
    lo, hi = CI.windows(pattern, p, q)
    return CI.reference(case["Xs"], case["Yc"], lo, hi, case["B"], case["m"])


def _handle(case):
    from atlasqtl_amd import prepare as P
    return P.prepare_on_device(case["Y"], case["X"], covariates=case["Z"])[0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _table(out):
    return set(zip(MU.int_list(out["snp"]), MU.int_list(out["trait"]), MU.int_list(_bits(out["r"]))))


def _rows(out):
    return set(zip(MU.int_list(out["snp"]), MU.int_list(out["trait"])))


@pytest.mark.parametrize("run", RUNS, ids=[_id(r) for r in RUNS])
def test_scan_against_long_double(run):
    shape, pattern, d, kind = run
    n, p, q = shape
    case = _case(shape, d, kind)
    B, m = case["B"], case["m"]
    lo, hi = CI.windows(pattern, p, q)
    ref = _reference(shape, pattern, d, kind)
    # the reference first: no ratio near a 1e-10 rule, and what cisint_util.case plants is there
    assert CI.thresholds_are_clear(ref) and CI.plants_hold(ref, kind, d, lo, hi)
    inside, defined, r_ref, bound = ref["inside"], ref["defined"], ref["r"], ref["bound"]
    assert B.shape == (d + 2, n) and ref["df"] == n - 4 - d
    M = int(inside.sum())
    prep = _handle(case)
    try:
        before = prep.cis(lo, hi, np.zeros(q), M)
        full = prep.cis_interaction(lo, hi, B, m, np.zeros(q), M)
        again = prep.cis_interaction(lo, hi, B, m, np.zeros(q), M)
        after = prep.cis(lo, hi, np.zeros(q), M)
        r64 = np.asarray(r_ref, dtype=np.float64)
        cut = MU.clear_cutoffs(r64)
        assert MU.cutoffs_are_clear(r64, cut)
        sel = prep.cis_interaction(lo, hi, B, m, cut, M)
        count = prep.cis_interaction(lo, hi, B, m, cut, 0)
        short = prep.cis_interaction(lo, hi, B, m, cut, sel["n_pairs"] - 1) if sel["n_pairs"] >= 1 else None
    finally:
        prep.close()
    # 1. cutoff 0: exactly the defined in-window pairs, every r within the bound; the undefined sets are equal; int_tol
    want = set(zip(*(MU.int_list(a) for a in np.nonzero(inside & defined))))
    assert full["n_pairs"] == len(want) and _rows(full) == want
    s, t = full["snp"], full["trait"]
    err = np.abs(full["r"].astype(MU.LD) - r_ref[s, t])
    ratio = float(np.max(err / bound[s, t])) if err.size else 0.0
    tol_ok = np.asarray(ref["pred_ok"], dtype=bool)
    tol_err = np.abs(full["int_tol"][tol_ok].astype(MU.LD) - ref["int_tol"][tol_ok])
    tol_ratio = float(np.max(tol_err / ref["tol_bound"][tol_ok]))
    print(f"{_id(run)}: {len(want)} of {M} in-window pairs defined; worst |r - reference| / bound {ratio:.2e}, worst error "
          f"{float(err.max()) if err.size else 0.0:.2e}; worst |int_tol - reference| / bound {tol_ratio:.2e}; W {full['plan']['n_items']}")
    assert (err <= bound[s, t]).all()
    np.testing.assert_array_equal(full["n_undef"], (inside & ~defined).sum(axis=0))
    np.testing.assert_array_equal(np.isnan(full["int_tol"]), ~tol_ok)
    assert (tol_err <= ref["tol_bound"][tol_ok]).all()
    assert np.isnan(full["int_tol"][CI.EQ]) and not (_rows(full) & {(CI.EQ, tr) for tr in range(q)})      # the plants are undefined
    if kind == "binary" and d == 0:
        assert np.isnan(full["int_tol"][CI.ZERO]) and not (_rows(full) & {(CI.ZERO, tr) for tr in range(q)})
    pl = full["plan"]
    assert (pl["streams"], pl["n_basis"], pl["lds_bytes"], pl["mult_pad"]) == (2, d + 2, 22528, -(-n // 16) * 16)
    assert pl["masked"] == 0 and pl["window_pairs"] == M and pl["n_items"] == before["plan"]["n_items"]
    # 2. the best predictor, where the reference's is clear of the runner-up by the bound
    has_window = hi > lo
    bs, clear = CI.best(ref)
    assert clear[0] and bs[0] == CI.PLANT
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
    for key in ("best_snp", "best_r", "n_undef", "int_tol"):
        assert sel[key].tobytes() == full[key].tobytes() == count[key].tobytes(), key
    # 4. two calls: the same bits everywhere, the same set of rows
    for key in ("best_snp", "best_r", "n_undef", "int_tol"):
        assert full[key].tobytes() == again[key].tobytes(), key
    assert again["n_pairs"] == full["n_pairs"] and again["plan"] == full["plan"] and _table(again) == _table(full)
    # 5. the handle is unchanged: the plain scan before and after gives identical bytes
    assert _table(before) == _table(after) and before["n_pairs"] == after["n_pairs"] and before["plan"] == after["plan"]
    for key in ("best_snp", "best_r", "n_undef"):
        assert before[key].tobytes() == after[key].tobytes(), key


def test_errors_come_in_the_documented_order_before_any_launch():
    """The refusals of the C ABI on a real handle, two faults at a time: the one the header names first is the one reported."""
    from atlasqtl_amd import _lib
    from atlasqtl_amd import prepare as P
    from atlasqtl_amd.prepare import AtlasqtlError
    shape, d, kind = (50, 17, 5), 3, "continuous"
    n, p, q = shape
    case = _case(shape, d, kind)
    lo, hi = CI.windows("all", p, q)
    L = _lib.lib()
    outs = [None] * 9
    good = dict(lo=lo, hi=hi, B=np.array(case["B"]), nb=d + 2, m=np.array(case["m"]), cut=np.zeros(q), cap=0)

    def raw(prep, **kw):
        a = dict(good, **kw)
        rc = L.aq_prep_cis_int(prep.handle, _lib.as_ip(a["lo"]), _lib.as_ip(a["hi"]), _lib.as_dp(a["B"]), a["nb"], _lib.as_dp(a["m"]),
                               _lib.as_dp(a["cut"]), a["cap"], *outs)
        return rc, L.aq_last_error()

    def edit(v, idx, value):
        v = np.array(v)
        v[idx] = value
        return v

    B_nan, B_skew = edit(good["B"], (1, 3), np.nan), edit(good["B"], (d + 1, 0), good["B"][d + 1, 0] + 1e-3)
    m_nan, m_out = edit(good["m"], 2, np.inf), good["m"] + np.arange(n) ** 2
    hi_bad, cut_nan = edit(hi, 1, p + 1), edit(good["cut"], 2, np.nan)
    faults = [(dict(cap=-1, nb=0), 1, b"cap >= 0 required"),
              (dict(nb=0, B=B_nan), 1, b"n_basis >= 1 required"),
              (dict(nb=257, B=B_nan), 3, b"at most 256"),
              (dict(B=B_nan, m=m_nan), 1, b"basis vector 1 has a non-finite entry"),
              (dict(m=m_nan, B=B_skew), 1, b"mult[2] is not finite"),
              (dict(B=B_skew, m=m_out), 1, b"not orthonormal"),
              (dict(m=m_out, hi=hi_bad), 1, b"not in the span"),
              (dict(m=np.zeros(n), hi=hi_bad), 1, b"mult is all zero"),
              (dict(hi=hi_bad, cut=cut_nan), 1, b"the window of trait 1"),
              (dict(cut=cut_nan), 1, b"r2_cut[2] is NaN")]
    prep = _handle(case)
    try:
        live = L.aq_debug_live_device_bytes()
        for kw, code, word in faults:
            rc, msg = raw(prep, **kw)
            assert rc == code and word in msg and b"aq_prep_cis_int" in msg, (kw.keys(), rc, msg)
            assert L.aq_debug_live_device_bytes() == live          # nothing was allocated, so nothing was launched
        assert raw(prep)[0] == 0
        with pytest.raises(AtlasqtlError, match="basis must be nb x n"):
            prep.cis_interaction(lo, hi, good["B"][:, :-1], good["m"], good["cut"], 0)
        # the timing entry on a small shape: both figures, and the plan it used
        ms, plan = (C.c_double(0.0), C.c_double(0.0)), _lib.AqCisintPlan()
        _lib.check(L.aq_prep_cis_int_time(prep.handle, _lib.as_ip(lo), _lib.as_ip(hi), _lib.as_dp(good["B"]), d + 2, _lib.as_dp(good["m"]), 1,
                                          C.byref(ms[0]), C.byref(ms[1]), C.byref(plan)), "aq_prep_cis_int_time")
        assert ms[0].value > 0 and ms[1].value > 0
        assert (plan.streams, plan.n_basis, plan.cis.n_items, plan.cis.q_active) == (2, d + 2, 1, q)
    finally:
        prep.close()
    # Y with missing values: refused by the Python layer, and by the library under its own name
    Y = np.array(case["Y"])
    Y[3, 1] = np.nan
    prep = P.prepare_on_device(Y, case["X"], covariates=case["Z"])[0]
    try:
        with pytest.raises(AtlasqtlError, match="missing values"):
            prep.cis_interaction(lo, hi, good["B"], good["m"], good["cut"], 0)
        rc, msg = raw(prep)
        assert rc == 3 and b"aq_prep_cis_int: Y has missing values" in msg
    finally:
        prep.close()


def test_cis_screen_with_interaction():
    """The public entry with covariates: the table's t, df, p and q against the reference run through the host statistics, the
    planted pair first, and the fields the argument adds."""
    import atlasqtl_amd as A
    from atlasqtl_amd import marginal as MG
    shape, d, kind = (50, 17, 5), 3, "binary"
    n, p, q = shape
    case = _case(shape, d, kind)
    chrom, pos = ["1"] * p, np.arange(p)
    kw = dict(window=100, snp_chrom=chrom, snp_pos=pos, p_value=1.0, covariates=case["Z"])
    plain = A.cis_screen(case["Y"], case["X"], ["1"] * q, np.full(q, 8), **kw)
    res = A.cis_screen(case["Y"], case["X"], ["1"] * q, np.full(q, 8), interaction=case["e"], **kw)
    for key in ("interaction", "int_tol", "best_pvalue_bonferroni"):
        assert key not in plain and key in res
    assert (plain["df"] == n - 2 - d).all() and (res["df"] == n - 4 - d).all() and res["n_covariates"] == d
    lo, hi = CI.windows("all", p, q)
    ref = _reference(shape, "all", d, kind)
    assert CI.thresholds_are_clear(ref) and CI.plants_hold(ref, kind, d, lo, hi)
    assert res["interaction"].tobytes() == case["m"].tobytes()                            # e centred
    a = res["assoc"]
    defined = ref["defined"]
    assert a["n_pairs"] == int(defined.sum()) == a["snp"].size and (a["snp"][0], a["trait"][0]) == (CI.PLANT, 0)
    np.testing.assert_array_equal(res["n_undefined"], (~defined).sum(axis=0))
    np.testing.assert_array_equal(res["n_tests"], defined.sum(axis=0))
    err = np.abs(a["r"].astype(MU.LD) - ref["r"][a["snp"], a["trait"]])
    assert (err <= ref["bound"][a["snp"], a["trait"]]).all()
    # the reference through the host statistics, row by row
    sr, tr = np.nonzero(defined)
    rr = np.asarray(ref["r"], dtype=np.float64)[sr, tr]
    t_ref, p_ref = MG.t_and_pvalue(rr, float(n - 4 - d))
    order = MG.table_order(p_ref, t_ref, sr, tr, p)
    q_ref = MG.bh_qvalues(p_ref[order], int(defined.sum()))
    want = {(int(sr[i]), int(tr[i])): (t_ref[i], p_ref[i], q_ref[k]) for k, i in enumerate(order)}
    rows = np.asarray([want[(int(s), int(t))] for s, t in zip(a["snp"], a["trait"])])
    assert (a["df"] == n - 4 - d).all()
    np.testing.assert_allclose(a["t"], rows[:, 0], rtol=1e-9)
    np.testing.assert_allclose(a["pvalue"], rows[:, 1], rtol=1e-8)
    np.testing.assert_allclose(a["qvalue"], rows[:, 2], rtol=1e-8)
    np.testing.assert_allclose(a["t"], CI.t_of(a["r"], n - 4 - d), rtol=1e-12)
    tol_ok = np.asarray(ref["pred_ok"], dtype=bool)
    np.testing.assert_array_equal(np.isnan(res["int_tol"]), ~tol_ok)
    assert (np.abs(res["int_tol"][tol_ok].astype(MU.LD) - ref["int_tol"][tol_ok]) <= ref["tol_bound"][tol_ok]).all()
    np.testing.assert_array_equal(res["best_pvalue_bonferroni"], np.minimum(1.0, res["best_pvalue"] * res["n_tests"]))
    assert res["best_snp"][0] == CI.PLANT and res["best_pvalue_bonferroni"][0] < 1e-6
    assert res["plan"]["streams"] == 2 and res["plan"]["n_basis"] == d + 2
