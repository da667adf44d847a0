"""GPU: the cis scan (aq_prep_cis, aq_prep_cis_perm, csrc/aq_cis_kernels.h, csrc/aq_screen_tile.h) against the long-double restatement of
tests/mscreen_util.py run on the handle's own matrices and restricted to the windows, and against the device's own dense r of
aq_prep_marginal on the same handle, which every in-window r must equal to the bit.

Shapes (n, p, q): (20, 3, 1) and (50, 17, 5) below one tile; (333, 257, 33) odd n, nothing a multiple of 16; (257, 130, 130)
one past 64 and 128 in both directions; (130, 1000, 20) many predictor items per trait tile.  Each with Y complete, "random"
and "few", and with the window patterns
  all     every window is [0, p);
  band    seeded random windows; the first traits get, as far as q reaches, a window ending at p, one starting at 0, a
          width-1 one, an empty one and widths 63 / 64 / 65 where p allows; the last trait's window leaves out predictor 2,
          which mscreen_util.case plants as constant over that trait's observed rows: it must not be counted there;
  blocks  three disjoint "chromosomes", every trait with a window inside one of them; the last trait has the whole
          chromosome that holds predictor 2: it is counted there, as under `all`.
Permutations: B = 5 with the identity as row 0, every PB instance forced by AQ_CIS_PB (complete 1, 2, 4; masked 1, 2), the
plan's batch and a forced batch of 2.  With PB = 4 a batch of 2 is no multiple of PB, which the planner refuses: that refusal
is asserted, and PB = 4 runs with the forced batch 4 (two launches, the second one ragged) in its place."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import mscreen_util as MU

pytestmark = pytest.mark.gpu

SHAPES = [(20, 3, 1), (50, 17, 5), (333, 257, 33), (257, 130, 130), (130, 1000, 20)]
KINDS = (None, "random", "few")
PATTERNS = ("all", "band", "blocks")
B = 5
RUNS = [(s, k, w) for s in SHAPES for k in KINDS for w in PATTERNS]


def _id(run):
    (n, p, q), kind, pattern = run
    return f"{n}x{p}x{q}-{kind or 'complete'}-{pattern}"


def _set_env(monkeypatch, pb=None, batch=None):
    for name, v in (("AQ_CIS_PB", pb), ("AQ_CIS_BATCH", batch), ("AQ_MSCREEN_TILE", None), ("AQ_MSPERM_PB", None), ("AQ_MSPERM_BATCH", None)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def windows(pattern, p, q, seed=0):
    """(s_lo, s_hi) int32 of the pattern (module docstring)."""
    rng = np.random.default_rng(1000 * seed + 7 * p + q)
    lo, hi = np.zeros(q, dtype=np.int64), np.full(q, p, dtype=np.int64)
    last = q - 1
    if pattern == "all":
        pass
    elif pattern == "band":
        for t in range(q):
            a = int(rng.integers(0, p))
            lo[t], hi[t] = a, min(p, a + 1 + int(rng.integers(0, max(1, min(p, 90)))))
        special = [("end", 0), ("start", 0), ("width", 1), ("width", 0), ("width", 63), ("width", 64), ("width", 65)]
        for t, (what, w) in enumerate(special[:max(0, q - 1)]):
            if what == "end":
                lo[t], hi[t] = max(0, p - 1 - int(rng.integers(0, min(p, 40)))), p
            elif what == "start":
                lo[t], hi[t] = 0, 1 + int(rng.integers(0, min(p, 40)))
            elif w <= p:
                a = int(rng.integers(0, p - w + 1))
                lo[t], hi[t] = a, a + w
        if p > 3:                                            # the last trait: without predictor 2
            a = int(rng.integers(3, p))
            lo[last], hi[last] = a, min(p, a + 1 + int(rng.integers(0, min(p, 90))))
        else:
            lo[last], hi[last] = 0, 2
    elif pattern == "blocks":
        edges = [0, max(1, p // 3), max(2, 2 * p // 3), p]
        for t in range(q):
            c = t % 3
            a, b = edges[c], edges[c + 1]
            x, y = sorted(int(v) for v in rng.integers(a, b + 1, 2))
            lo[t], hi[t] = (x, y) if y > x else (a, b)
        c = next(c for c in range(3) if edges[c] <= 2 < edges[c + 1])
        lo[last], hi[last] = edges[c], edges[c + 1]
    else:
        raise AssertionError(pattern)
    assert np.all((0 <= lo) & (lo <= hi) & (hi <= p))
    return lo.astype(np.int32), hi.astype(np.int32)


def _inside(lo, hi, p):
    s = np.arange(p)[:, None]
    return (s >= lo[None, :]) & (s < hi[None, :])


def _perms(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.arange(n)] + [rng.permutation(n) for _ in range(B - 1)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """Once per (shape, kind), shared by every test and left unchanged: the raw inputs; of a handle prepared from them the
    long-double reference (r_ref, bound), the device's own dense r and the plain screen at cutoff 0; clear cutoffs; the
    permutations and the reference of each permuted Y."""
    from atlasqtl_amd import prepare as P
    n, p, q = shape
    X, Y = MU.case(n, p, q, kind)
    prep = P.prepare_on_device(Y, X)[0]
    try:
        assert prep.p == p
        Xs, Yc = prep.X_host(), prep.Y
        dense = prep.marginal(np.full(q, np.inf), 0, dense=True)["r_dense"]
        plain = prep.marginal(np.zeros(q), p * q)
    finally:
        prep.close()
    r_ref, bound, m, df = MU.reference(Xs, Yc, 0)
    cut = MU.clear_cutoffs(r_ref)
    assert MU.cutoffs_are_clear(r_ref, cut)
    perms = _perms(n, 100 + n)
    perm_refs = [MU.reference(Xs, Yc[perms[b]], 0)[:2] for b in range(B)]
    out = dict(X=X, Y=Y, r_ref=r_ref, bound=bound, dense=dense, plain=plain, cut=cut, perms=perms, perm_refs=perm_refs, kind=kind)
    for v in (X, Y, dense, cut, perms):
        v.setflags(write=False)
    return out


def _handle(case):
    from atlasqtl_amd import prepare as P
    return P.prepare_on_device(case["Y"], case["X"])[0]


def _rows(out):
    return set(zip(MU.int_list(out["snp"]), MU.int_list(out["trait"])))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _device_best(dense, lo, hi):
    """(best_snp, best_r) from the device's own dense r: the lowest index of the largest r^2 over the window."""
    q = dense.shape[1]
    bs, br = np.full(q, -1, dtype=np.int32), np.full(q, np.nan)
    for t in range(q):
        col = dense[lo[t]:hi[t], t]
        r2 = np.where(np.isnan(col), -1.0, col * col)
        if r2.size and r2.max() >= 0:
            bs[t] = lo[t] + int(np.argmax(r2))               # argmax: the first of equal values
            br[t] = dense[bs[t], t]
    return bs, br


@pytest.mark.parametrize("run", RUNS, ids=[_id(r) for r in RUNS])
def test_scan_against_long_double_and_the_dense_screen(run, monkeypatch):
    shape, kind, pattern = run
    n, p, q = shape
    _set_env(monkeypatch)
    case = _case(shape, kind)
    r_ref, bound, dense = case["r_ref"], case["bound"], case["dense"]
    lo, hi = windows(pattern, p, q)
    inside = _inside(lo, hi, p)
    defined = ~np.isnan(np.asarray(r_ref, dtype=np.float64))
    M = int(inside.sum())
    prep = _handle(case)
    try:
        full = prep.cis(lo, hi, np.zeros(q), M)
        again = prep.cis(lo, hi, np.zeros(q), M)
        sel = prep.cis(lo, hi, case["cut"], M)
        count = prep.cis(lo, hi, case["cut"], 0)
        short = prep.cis(lo, hi, case["cut"], sel["n_pairs"] - 1) if sel["n_pairs"] >= 1 else None
    finally:
        prep.close()
    # 1. cutoff 0: exactly the defined in-window pairs, r equal to the dense screen's to the bit and within the bound
    want = set(zip(*(MU.int_list(a) for a in np.nonzero(inside & defined))))
    assert full["n_pairs"] == len(want) and _rows(full) == want
    s, t = full["snp"], full["trait"]
    assert (_bits(full["r"]) == _bits(dense[s, t])).all()
    err = np.abs(full["r"].astype(MU.LD) - r_ref[s, t])
    ratio = float(np.max(err / bound[s, t])) if err.size else 0.0
    print(f"{_id(run)}: {len(want)} of {M} in-window pairs defined; worst |r - reference| / bound {ratio:.3f}; "
          f"fill {full['plan']['window_pairs']} / {full['plan']['staged_pairs']}, W {full['plan']['n_items']}")
    assert (err <= bound[s, t]).all()
    np.testing.assert_array_equal(full["n_undef"], (inside & ~defined).sum(axis=0))
    assert full["plan"]["window_pairs"] == M and full["plan"]["masked"] == (0 if kind is None else 1)
    if kind is not None and p > 2:                           # the planted pair: predictor 2 on the last trait
        assert not defined[2, q - 1]
        assert inside[2, q - 1] == (pattern != "band")
        assert full["n_undef"][q - 1] >= (1 if pattern != "band" else 0)
        assert full["n_undef"][q - 1] == int((~defined[lo[q - 1]:hi[q - 1], q - 1]).sum())
    # 2. the best predictor: exact against the device's own dense r
    bs, br = _device_best(dense, lo, hi)
    np.testing.assert_array_equal(full["best_snp"], bs)
    assert _bits(full["best_r"]).tobytes() == _bits(br).tobytes()
    assert (full["best_snp"][lo == hi] == -1).all()
    # 3. clear cutoffs: the reference's selection restricted to the windows; cap = 0 only counts; a short table is a subset
    r2 = np.where(defined, np.asarray(r_ref * r_ref, dtype=np.float64), -1.0)
    want_sel = set(zip(*(MU.int_list(a) for a in np.nonzero(inside & defined & (r2 >= case["cut"][None, :])))))
    assert sel["n_pairs"] == len(want_sel) and _rows(sel) == want_sel
    assert count["n_pairs"] == len(want_sel) and count["snp"].size == 0
    for key in ("best_snp", "best_r", "n_undef"):
        assert sel[key].tobytes() == full[key].tobytes() == count[key].tobytes(), key
    if short is not None:
        assert short["n_pairs"] == len(want_sel) and short["snp"].size == len(want_sel) - 1
        assert _rows(short) < want_sel and len(_rows(short)) == len(want_sel) - 1
    # 4. every window [0, p): the plain screen, to the bit
    if pattern == "all":
        plain = case["plain"]
        assert full["n_pairs"] == plain["n_pairs"]
        assert set(zip(MU.int_list(s), MU.int_list(t), MU.int_list(_bits(full["r"])))) == \
            set(zip(MU.int_list(plain["snp"]), MU.int_list(plain["trait"]), MU.int_list(_bits(plain["r"]))))
        np.testing.assert_array_equal(full["best_snp"], plain["best_snp"])
        assert _bits(full["best_r"]).tobytes() == _bits(plain["best_r"]).tobytes()
        assert int(full["n_undef"].sum()) == plain["n_undefined"]
        assert full["plan"]["n_items"] == -(-p // 64) * -(-q // 64)
    # 5. two calls: the same bytes everywhere, the same set of rows
    for key in ("best_snp", "best_r", "n_undef"):
        assert full[key].tobytes() == again[key].tobytes(), key
    assert again["n_pairs"] == full["n_pairs"] and again["plan"] == full["plan"]
    assert set(zip(MU.int_list(again["snp"]), MU.int_list(again["trait"]), MU.int_list(_bits(again["r"])))) == \
        set(zip(MU.int_list(s), MU.int_list(t), MU.int_list(_bits(full["r"]))))


def test_the_tie_and_the_windows_without_a_best():
    """Trait 0 is 3 x_0 + noise and predictor 1 is -x_0: a window holding 0 and 1 gives 0, a window holding only 1 gives 1;
    an empty window and a window whose only pair is undefined give -1 / NaN."""
    n, p, q = 50, 17, 5
    case = _case((n, p, q), "few")
    assert np.isnan(float(case["r_ref"][2, q - 1]))
    prep = _handle(case)
    try:
        a = prep.cis(np.array([0, 5, 0, 3, 2]), np.array([2, 5, 17, 9, 3]), np.zeros(q), 64)
        b = prep.cis(np.array([1, 5, 0, 3, 2]), np.array([2, 5, 17, 9, 3]), np.zeros(q), 64)
    finally:
        prep.close()
    assert a["best_snp"][0] == 0 and b["best_snp"][0] == 1
    assert a["best_r"][0] == -b["best_r"][0] and abs(a["best_r"][0]) > 0.9
    for out in (a, b):
        assert out["best_snp"][1] == -1 and np.isnan(out["best_r"][1]) and out["n_undef"][1] == 0         # empty
        assert out["best_snp"][4] == -1 and np.isnan(out["best_r"][4]) and out["n_undef"][4] == 1         # all undefined
        assert 3 <= out["best_snp"][3] < 9 and out["best_snp"][2] >= 0
        assert not any(tr in (1, 4) for tr in MU.int_list(out["trait"]))
    assert a["n_pairs"] == 2 + 17 + 6 and b["n_pairs"] == 1 + 17 + 6


def _window_max(r_ref, bound, inside):
    """Per trait over its window: (max r_ref^2, -1 where no pair is defined; max (2 |r_ref| bound + bound^2)), the form of
    tests/test_gpu_msperm.py: |r^2 - r_ref^2| = |r - r_ref| |r + r_ref| <= bound (2 |r_ref| + bound) for every pair, and the
    maximum of values that each move by at most their own tolerance moves by at most the largest tolerance."""
    ok = inside & ~np.isnan(np.asarray(r_ref, dtype=np.float64))
    r2 = np.where(ok, r_ref * r_ref, -1.0)
    tol = np.where(ok, 2 * np.abs(r_ref) * bound + bound * bound, 0.0)
    return r2.max(axis=0), tol.max(axis=0).astype(np.float64)


@pytest.mark.parametrize("run", RUNS, ids=[_id(r) for r in RUNS])
def test_permutations(run, monkeypatch):
    from atlasqtl_amd import _lib
    shape, kind, pattern = run
    n, p, q = shape
    case = _case(shape, kind)
    perms = case["perms"]
    lo, hi = windows(pattern, p, q)
    inside = _inside(lo, hi, p)
    refs = [_window_max(r_ref, bound, inside) for r_ref, bound in case["perm_refs"]]
    configs = [(pb, bt) for pb in ((1, 2, 4) if kind is None else (1, 2)) for bt in (None, 2 if pb < 4 else 4)]
    prep = _handle(case)
    worst = 0.0
    try:
        _set_env(monkeypatch)
        scan = prep.cis(lo, hi, np.full(q, np.inf), 0)
        want0 = np.where(scan["best_snp"] >= 0, scan["best_r"] * scan["best_r"], -1.0)
        plain = prep.marginal_permute(np.full(q, np.inf), perms)["max_r2"] if pattern == "all" else None
        first = None
        for pb, bt in [(None, None)] + configs:
            _set_env(monkeypatch, pb, bt)
            got = prep.cis_permute(lo, hi, perms)
            assert got.shape == (B, q)
            assert got[0].tobytes() == want0.tobytes(), (pb, bt)          # the identity: best_r^2 to the bit, -1.0 where none
            if plain is not None:
                assert got.tobytes() == plain.tobytes(), (pb, bt)
            for b in range(1, B):
                best, tol = refs[b]
                none = np.asarray(best, dtype=np.float64) < 0
                np.testing.assert_array_equal(got[b][none], -1.0)
                err = np.abs(got[b].astype(MU.LD) - best)[~none]
                if err.size:
                    worst = max(worst, float(np.max(err / tol[~none])))
                assert (err <= tol[~none]).all(), (pb, bt, b)
            if first is None:
                first = got
            assert got.tobytes() == first.tobytes(), (pb, bt)             # every instance and batch: the same bits
        if kind is None:
            _set_env(monkeypatch, 4, 2)                                     # no multiple of PB
            with pytest.raises(_lib.AtlasqtlHipError, match="AQ_CIS_BATCH"):
                prep.cis_permute(lo, hi, perms)
    finally:
        prep.close()
    assert (want0[lo == hi] == -1.0).all()
    if q > 1 and p > 3:
        assert any(not np.array_equal(first[b], first[0]) for b in range(1, B))       # the other rows are other statistics
    print(f"{_id(run)}: worst |max r^2 - reference| / tolerance over {len(configs) + 1} configurations {worst:.3f}")


def test_refusals_on_a_real_handle(monkeypatch):
    from atlasqtl_amd import _lib
    n, p, q = 50, 17, 5
    case = _case((n, p, q), None)
    _set_env(monkeypatch)
    prep = _handle(case)
    L = _lib.lib()
    i64 = C.POINTER(C.c_int64)
    outs = (None, None, None, C.cast(None, i64), None, None, C.cast(None, i64), None)
    good_lo, good_hi = windows("band", p, q)
    cut = np.full(q, 0.1)
    perms = case["perms"]

    def i32(a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        return a, _lib.as_ip(a)
    try:
        for blo, bhi, msg in (([0, 0, 18, 0, 0], [17] * 5, b"the window of trait 2, [18, 17), is outside [0, 17]"),
                              ([0] * 5, [17, 17, 17, 18, 17], b"the window of trait 3, [0, 18), is outside [0, 17]"),
                              ([0, -1, 0, 0, 0], [17] * 5, b"the window of trait 1, [-1, 17), is outside [0, 17]"),
                              ([0, 0, 0, 0, 7], [17, 17, 17, 17, 6], b"s_lo > s_hi for trait 4 (7 > 6)")):
            (klo, plo), (khi, phi) = i32(blo), i32(bhi)
            assert L.aq_prep_cis(prep.handle, plo, phi, _lib.as_dp(cut), 0, *outs) == 1
            assert b"aq_prep_cis: " + msg in L.aq_last_error(), L.aq_last_error()
            assert L.aq_prep_cis_perm(prep.handle, plo, phi, B, _lib.as_ip(perms), None) == 1
            assert b"aq_prep_cis_perm: " + msg in L.aq_last_error(), L.aq_last_error()
            ms = (C.c_double(0.0), C.c_double(0.0))
            assert L.aq_prep_cis_time(prep.handle, plo, phi, 0, 1, C.byref(ms[0]), C.byref(ms[1]), None) == 1
            assert b"aq_prep_cis_time: " + msg in L.aq_last_error(), L.aq_last_error()
        (klo, plo), (khi, phi) = i32(good_lo), i32(good_hi)
        bad = cut.copy()
        bad[3] = np.nan
        assert L.aq_prep_cis(prep.handle, plo, phi, _lib.as_dp(bad), 0, *outs) == 1
        assert b"aq_prep_cis: r2_cut[3] is NaN" in L.aq_last_error()
        rep = perms.copy()
        rep[2, 5] = rep[2, 6]
        assert L.aq_prep_cis_perm(prep.handle, plo, phi, B, _lib.as_ip(rep), None) == 1
        msg = L.aq_last_error()
        assert b"aq_prep_cis_perm: row 2 of perm" in msg and b"repeated" in msg
        far = perms.copy()
        far[1, 0] = n
        assert L.aq_prep_cis_perm(prep.handle, plo, phi, B, _lib.as_ip(far), None) == 1
        msg = L.aq_last_error()
        assert b"aq_prep_cis_perm: row 1 of perm" in msg and b"out of range" in msg
        with pytest.raises(_lib.AtlasqtlHipError, match="row 2 of perm"):
            prep.cis_permute(good_lo, good_hi, rep)
        for name, v in (("AQ_CIS_PB", "3"), ("AQ_CIS_PB", "abc"), ("AQ_CIS_BATCH", "0"), ("AQ_CIS_BATCH", "7")):
            _set_env(monkeypatch)
            monkeypatch.setenv(name, v)
            with pytest.raises(_lib.AtlasqtlHipError, match=name):
                prep.cis_permute(good_lo, good_hi, perms)
            prep.cis(good_lo, good_hi, cut, 0)                           # the scan does not read them
        _set_env(monkeypatch)
        # the timing entry on a small shape: both figures, and the plan it used
        ms, plan = (C.c_double(0.0), C.c_double(0.0)), _lib.AqCisPlan()
        _lib.check(L.aq_prep_cis_time(prep.handle, plo, phi, 3, 1, C.byref(ms[0]), C.byref(ms[1]), C.byref(plan)), "aq_prep_cis_time")
        assert ms[0].value > 0 and ms[1].value > 0 and plan.batch >= 3 and plan.launches == 1 and plan.masked == 0 and plan.pb == 2
        _lib.check(L.aq_prep_cis_time(prep.handle, plo, phi, 0, 1, C.byref(ms[0]), C.byref(ms[1]), C.byref(plan)), "aq_prep_cis_time")
        assert ms[0].value > 0 and ms[1].value == 0.0 and plan.batch == 0
        # every window empty: nothing to launch, every output says so
        zero = np.zeros(q, dtype=np.int32)
        out = prep.cis(zero, zero, cut, 8)
        assert out["n_pairs"] == 0 and (out["best_snp"] == -1).all() and np.isnan(out["best_r"]).all() and not out["n_undef"].any()
        assert out["plan"]["n_items"] == 0
        np.testing.assert_array_equal(prep.cis_permute(zero, zero, perms), -1.0)
    finally:
        prep.close()


# ---- the Python layer ----
def _fileset(tmp_path, n=60, p=40, seed=5):
    """A fileset over two chromosomes (25 and 15 variants, positions 1000 apart) and its A1 dosages."""
    from tests import bed_util
    rng = np.random.default_rng(seed)
    G = rng.binomial(2, rng.uniform(0.2, 0.8, p), size=(n, p))
    prefix = str(tmp_path / "cis")
    snp_ids, _ = bed_util.write_fileset(prefix, G)
    chrom = ["1"] * 25 + ["2"] * (p - 25)
    pos = [1000 * (j + 1) for j in range(25)] + [1000 * (j + 1) for j in range(p - 25)]
    with open(prefix + ".bim", "w") as f:
        for j, rs in enumerate(snp_ids):
            f.write(f"{chrom[j]}\t{rs}\t0\t{pos[j]}\tA\tC\n")
    return prefix, G.astype(np.float64), snp_ids, chrom, np.array(pos)


def _host_tests(res, G, Y, snp_ids):
    """scipy's Pearson test of every in-window pair of the result, on the host: {(snp, trait): (r, p-value)}."""
    from scipy.stats import pearsonr
    col = {name: j for j, name in enumerate(snp_ids)}
    out = {}
    lo, hi = res["window"]
    for t in range(Y.shape[1]):
        for s in range(lo[t], hi[t]):
            r, pv = pearsonr(G[:, col[res["names_x"][s]]], Y[:, t])
            out[(s, t)] = (float(r), float(pv))
    return out


def test_api_end_to_end(tmp_path, monkeypatch):
    import atlasqtl_amd as A
    from atlasqtl_amd import marginal as M
    _set_env(monkeypatch)
    prefix, G, snp_ids, chrom, pos = _fileset(tmp_path)
    n, p = G.shape
    rng = np.random.default_rng(9)
    tchrom = ["1", "1", "2", "2", "3", "1"]
    tstart = np.array([5000, 20000, 3000, 12000, 5000, 24000])
    tend = tstart + np.array([0, 1500, 0, 0, 0, 0])
    q = len(tchrom)
    Y = rng.standard_normal((n, q))
    Y[:, 0] += 1.5 * G[:, 4]                                  # chromosome 1, position 5000: inside the window of trait 0
    Y[:, 2] += 1.0 * G[:, 27]                                 # chromosome 2, position 3000
    Y[:, 1] += 1.5 * G[:, 30]                                 # a trans effect: on chromosome 2, outside every window of trait 1
    bed = A.PlinkBed(prefix)
    window = 4000
    res = A.cis_screen(Y, bed, tchrom, tstart, tend, window=window, p_value=0.05)
    assert res["names_x"] == [nm for nm in snp_ids if nm in set(res["names_x"])] and res["p"] == len(res["names_x"])
    kept = np.array([nm in set(res["names_x"]) for nm in snp_ids])
    lo, hi = A.cis_windows(np.array(chrom, dtype=object)[kept], pos[kept], tchrom, tstart, tend, window)
    np.testing.assert_array_equal(res["window"][0], lo)
    np.testing.assert_array_equal(res["window"][1], hi)
    np.testing.assert_array_equal(res["n_cis"], hi - lo)
    assert res["n_cis"][4] == 0 and (res["n_cis"][[0, 1, 2, 3, 5]] > 0).all()
    assert res["plan"]["window_pairs"] == int((hi - lo).sum()) <= res["plan"]["staged_pairs"]
    host = _host_tests(res, G, Y, snp_ids)
    assert len(host) == int((hi - lo).sum())
    a = res["assoc"]
    want = {k for k, (r, pv) in host.items() if pv <= 0.05}
    assert min(abs(pv - 0.05) for r, pv in host.values()) > 1e-9          # no pair sits on the threshold
    assert set(zip(MU.int_list(a["snp"]), MU.int_list(a["trait"]))) == want and a["n_pairs"] == len(want)
    np.testing.assert_allclose(a["r"], [host[k][0] for k in zip(MU.int_list(a["snp"]), MU.int_list(a["trait"]))], rtol=0, atol=1e-12)
    np.testing.assert_allclose(a["pvalue"], [host[k][1] for k in zip(MU.int_list(a["snp"]), MU.int_list(a["trait"]))], rtol=1e-8)
    assert (np.diff(a["pvalue"]) >= 0).all() and (a["df"] == n - 2).all()
    assert (0, 0) in {(int(res["names_x"][s] != snp_ids[4]), t) for s, t in want}      # the planted cis effect is found
    assert all(t != 1 or chrom[snp_ids.index(res["names_x"][s])] == "1" for s, t in want)   # the trans effect is not looked at
    # the best predictor per trait; the gene on a chromosome without variants
    for t in range(q):
        mine = {k: v for k, v in host.items() if k[1] == t}
        if not mine:
            assert res["best_snp"][t] == -1 and np.isnan(res["best_r"][t]) and np.isnan(res["best_pvalue"][t]) and res["n_tests"][t] == 0
            continue
        top = max(mine, key=lambda k: mine[k][0] ** 2)
        assert res["best_snp"][t] == top[0]
        np.testing.assert_allclose([res["best_r"][t], res["best_pvalue"][t]], mine[top], rtol=1e-8)
    assert res["best_snp"][4] == -1 and res["best_snp"][0] == res["names_x"].index(snp_ids[4])
    np.testing.assert_array_equal(res["n_tests"], res["n_cis"] - res["n_undefined"])
    # Bonferroni over the in-window tests by default
    bon = A.cis_screen(Y, bed, tchrom, tstart, tend, window=window)
    assert bon["threshold"]["mode"] == "bonferroni" and bon["threshold"]["level"] == 0.05 / len(host)
    assert set(zip(MU.int_list(bon["assoc"]["snp"]), MU.int_list(bon["assoc"]["trait"]))) == \
        {k for k, (r, pv) in host.items() if pv <= 0.05 / len(host)}
    # fdr: Benjamini-Hochberg over the in-window tests, densely on the host
    alpha = 0.2
    keys = sorted(host, key=lambda k: host[k][1])
    pv = np.array([host[k][1] for k in keys])
    below = np.nonzero(pv <= alpha * np.arange(1, pv.size + 1) / pv.size)[0]
    k_bh = int(below[-1]) + 1 if below.size else 0
    fdr = A.cis_screen(Y, bed, tchrom, tstart, tend, window=window, fdr=alpha)
    assert k_bh >= 2 and fdr["assoc"]["n_pairs"] == k_bh
    assert set(zip(MU.int_list(fdr["assoc"]["snp"]), MU.int_list(fdr["assoc"]["trait"]))) == set(keys[:k_bh])
    dense_q = np.minimum(np.minimum.accumulate((pv * pv.size / np.arange(1, pv.size + 1))[::-1])[::-1], 1.0)
    np.testing.assert_allclose(fdr["assoc"]["qvalue"], dense_q[:k_bh], rtol=1e-8)
    assert fdr["threshold"]["n_tests"] == len(host)
    # permutations: reproducible, equal to the explicit rows of the recipe, NaN for the gene without a window
    spec = {"n": 20, "seed": 3}
    pa = A.cis_screen(Y, bed, tchrom, tstart, tend, window=window, p_value=0.05, permutations=spec)
    pb = A.cis_screen(Y, bed, tchrom, tstart, tend, window=window, p_value=0.05, permutations=spec)
    rows = M.permutation_options(spec, n)["perms"]
    pc = A.cis_screen(Y, bed, tchrom, tstart, tend, window=window, p_value=0.05, permutations=rows)
    assert "permutation" not in res
    for key in ("best_snp", "best_r", "n_cis"):
        np.testing.assert_array_equal(pa[key], res[key])
    perm = pa["permutation"]
    assert set(perm) == {"n", "seed", "max_r2", "trait_pvalue", "beta_shape1", "beta_shape2", "trait_pvalue_beta", "trait_qvalue"}
    assert (perm["n"], perm["seed"]) == (20, 3) and perm["max_r2"].shape == (20, q)
    assert pc["permutation"]["seed"] is None and pc["permutation"]["n"] == 20
    for key in ("max_r2", "trait_pvalue", "beta_shape1", "beta_shape2", "trait_pvalue_beta", "trait_qvalue"):
        assert perm[key].tobytes() == pb["permutation"][key].tobytes() == pc["permutation"][key].tobytes(), key
    np.testing.assert_array_equal(perm["max_r2"][:, 4], -1.0)
    assert (perm["max_r2"][:, [0, 1, 2, 3, 5]] >= 0).all()
    for key in ("trait_pvalue", "trait_pvalue_beta", "trait_qvalue"):
        assert np.isnan(perm[key][4]) and not np.isnan(perm[key][[0, 1, 2, 3, 5]]).any(), key
    obs = res["best_r"] ** 2
    want_p = (1 + (perm["max_r2"] >= np.where(res["best_snp"] >= 0, obs, np.inf)[None, :]).sum(axis=0)) / 21
    np.testing.assert_array_equal(perm["trait_pvalue"][[0, 1, 2, 3, 5]], want_p[[0, 1, 2, 3, 5]])
    assert perm["trait_pvalue"][0] == 1 / 21 and perm["trait_pvalue_beta"][0] < 1e-3
    # the Benjamini-Hochberg step over the five traits with a window: the gene without one is not among the tests
    pbeta = perm["trait_pvalue_beta"][[0, 1, 2, 3, 5]]
    order = np.argsort(pbeta)
    want_q = np.empty(5)
    want_q[order] = M.bh_qvalues(pbeta[order], 5)
    np.testing.assert_allclose(perm["trait_qvalue"][[0, 1, 2, 3, 5]], want_q, rtol=1e-15)
    # covariates: df drops by d
    Z = np.random.default_rng(2).standard_normal((n, 3))
    cov = A.cis_screen(Y, bed, tchrom, tstart, tend, window=window, p_value=0.05, covariates=Z)
    assert (cov["df"] == n - 2 - 3).all() and cov["n_covariates"] == 3 and (cov["assoc"]["df"] == n - 5).all()
    # positions given by hand for a plain matrix give what the fileset gives
    arr = A.cis_screen(Y, G, tchrom, tstart, tend, window=window, p_value=0.05, snp_chrom=chrom, snp_pos=pos)
    np.testing.assert_array_equal(arr["window"][0], res["window"][0])
    np.testing.assert_array_equal(arr["best_snp"], res["best_snp"])
    np.testing.assert_allclose(arr["best_r"], res["best_r"], rtol=1e-10)
