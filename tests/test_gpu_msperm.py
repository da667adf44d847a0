"""GPU: permutation nulls of the marginal screen (aq_prep_marginal_perm, csrc/aq_msperm_kernels.h, csrc/aq_screen_tile.h) against the long-double
restatement of tests/mscreen_util.py run on the handle's own matrices with the rows of Y permuted on the host.  Shapes:
(37, 70, 5): odd n, q below a tile, two predictor tiles; (50, 130, 67): n no multiple of 16, both dimensions ragged, two trait
tiles; (96, 200, 150).  Each with complete Y and with the missing kinds "random" and "few", B = 5 permutations, and every
instance of the tile kernel -- complete Y at tile 64 with PB 1, 2, 4 and at tile 128 with PB 1, masked Y with PB 1, 2 -- with
the plan's own batch (one launch, a ragged last PB group where PB does not divide 5) and with AQ_MSPERM_BATCH 2 or 4 (several
launches, a ragged last one), and the plan's own choice of everything."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import mscreen_util as MU

pytestmark = pytest.mark.gpu

SHAPES = [(37, 70, 5), (50, 130, 67), (96, 200, 150)]
KINDS = (None, "random", "few")
B = 5
# (tile, PB, batch); None: the plan's choice
COMPLETE = [(None, None, None)] + [(64, pb, bt) for pb, bts in ((1, (None, 2)), (2, (None, 2, 4)), (4, (None, 4))) for bt in bts] + \
           [(128, 1, None), (128, 1, 2)]
MASKED = [(None, None, None), (None, 1, None), (None, 1, 2), (None, 2, None), (None, 2, 2), (None, 2, 4)]
RUNS = [(s, k, cfg) for s in SHAPES for k in KINDS for cfg in (COMPLETE if k is None else MASKED)]


def _id(run):
    (n, p, q), kind, (tile, pb, batch) = run
    return f"{n}x{p}x{q}-{kind or 'complete'}-tile{tile or 'plan'}-pb{pb or 'plan'}-batch{batch or 'plan'}"


def _set_env(monkeypatch, tile=None, pb=None, batch=None):
    for name, v in (("AQ_MSCREEN_TILE", tile), ("AQ_MSPERM_PB", pb), ("AQ_MSPERM_BATCH", batch)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _perms(n, b, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n) for _ in range(b)]).astype(np.int32)


def _tol(r_ref, bound):
    """Per trait: (max_s r_ref^2 in fp64, -1 where no pair is defined; max_s (2 |r_ref| bound + bound^2)).  |r^2 - r_ref^2| =
    |r - r_ref| |r + r_ref| <= bound (2 |r_ref| + bound) for every pair, and the maximum of values that each move by at most
    their own tolerance moves by at most the largest tolerance."""
    defined = ~np.isnan(np.asarray(r_ref, dtype=np.float64))
    r2 = np.where(defined, r_ref * r_ref, -1.0)
    tol = np.where(defined, 2 * np.abs(r_ref) * bound + bound * bound, 0.0)
    return r2.max(axis=0), tol.max(axis=0).astype(np.float64), defined


@functools.lru_cache(maxsize=None)
def _case(shape, kind, seed=0, n_cov=0, few_m=None):
    """(X, Y as given, perms, per permutation (max r_ref^2, tolerance, n_undefined, hs_max, n_sel), the cutoffs, covariates or
    None), once per case.  The cutoffs are clear of every permutation's reference r^2: a condition on the inputs, asserted here."""
    from atlasqtl_amd import prepare as P
    n, p, q = shape
    X, Y = MU.case(n, p, q, kind, few_m=few_m)
    Z = None if n_cov == 0 else np.asfortranarray(np.random.default_rng(5).standard_normal((n, n_cov)))
    prep = P.prepare_on_device(Y, X, covariates=Z)[0]
    Xs, Yc = prep.X_host(), prep.Y
    assert prep.p == p and prep.n_cov == n_cov
    prep.close()
    perms = _perms(n, B, 100 + seed)
    refs = [MU.reference(Xs, Yc[perms[b]], n_cov)[:2] for b in range(B)]
    stack = np.concatenate([r for r, _ in refs], axis=0)
    cut = MU.clear_cutoffs(stack)
    assert MU.cutoffs_are_clear(stack, cut)
    per = []
    for r_ref, bound in refs:
        best, tol, defined = _tol(r_ref, bound)
        rows, rs, n_undef, _ = MU.selection(r_ref, cut)
        per.append((np.asarray(best, dtype=MU.LD), tol, n_undef, int(rs.max()), len(rows)))
    for a in (X, Y, perms, cut):
        a.setflags(write=False)
    return X, Y, perms, per, cut, Z


def _check(case, label):
    """max_r2 within the tolerance, -1.0 exactly where the reference has no defined pair, the three counts exactly."""
    from atlasqtl_amd import prepare as P
    X, Y, perms, per, cut, Z = case
    prep = P.prepare_on_device(Y, X, covariates=Z)[0]
    try:
        out = prep.marginal_permute(cut, perms)
    finally:
        prep.close()
    assert out["max_r2"].shape == (B, Y.shape[1])
    worst = 0.0
    for b, (best, tol, n_undef, hs, nsel) in enumerate(per):
        got = out["max_r2"][b]
        none = np.asarray(best, dtype=np.float64) < 0
        np.testing.assert_array_equal(got[none], -1.0)
        err = np.abs(got.astype(MU.LD) - best)[~none]
        if err.size:
            worst = max(worst, float(np.max(err / tol[~none])))
        assert (err <= tol[~none]).all(), (b, float(np.max(err / tol[~none])))
        assert out["n_undef"][b] == n_undef, b
        assert out["hs_max"][b] == hs and out["n_sel"][b] == nsel, (b, out["hs_max"][b], hs, out["n_sel"][b], nsel)
    print(f"{label}: worst |max r^2 - reference| / tolerance {worst:.3f}; n_sel {[v[4] for v in per]}, hs_max {[v[3] for v in per]}, "
          f"n_undef {[v[2] for v in per]}")
    assert sum(v[4] for v in per) > 0                          # the cutoffs select something
    return out


@pytest.mark.parametrize("run", RUNS, ids=[_id(r) for r in RUNS])
def test_against_long_double(run, monkeypatch):
    shape, kind, (tile, pb, batch) = run
    _set_env(monkeypatch, tile, pb, batch)
    _check(_case(shape, kind), _id(run))


@pytest.mark.parametrize("pb", [1, 2])
def test_trait_without_a_defined_pair(pb, monkeypatch):
    """With d = 2 covariates the trait with m = 4 observed values has df = 0: undefined for every predictor under every
    permutation, max_r2 = -1.0 there, and its p pairs are counted (the case of tests/test_gpu_mscreen.py)."""
    shape, d = (50, 130, 67), 2
    case = _case(shape, "few", 0, d, 4)
    _set_env(monkeypatch, None, pb, 2)
    out = _check(case, f"covariates d={d} few pb={pb}")
    np.testing.assert_array_equal(out["max_r2"][:, -1], -1.0)
    assert (out["max_r2"][:, :-1] >= 0).all() and (out["n_undef"] >= shape[1]).all()


@pytest.mark.parametrize("kind", [None, "random"])
def test_two_calls_give_the_same_bits(kind, monkeypatch):
    from atlasqtl_amd import prepare as P
    X, Y, perms, per, cut, _ = _case((96, 200, 150), kind)
    _set_env(monkeypatch)
    prep = P.prepare_on_device(Y, X)[0]
    try:
        a = prep.marginal_permute(cut, perms)
        b = prep.marginal_permute(cut, perms)
    finally:
        prep.close()
    for key in ("max_r2", "hs_max", "n_sel", "n_undef"):
        assert a[key].tobytes() == b[key].tobytes(), key


IDENTITY = [(None, 64, 1), (None, 64, 2), (None, 64, 4), (None, 128, 1), ("random", None, 1), ("random", None, 2), ("few", None, 2)]


@pytest.mark.parametrize("kind,tile,pb", IDENTITY, ids=[f"{k or 'complete'}-tile{t or 'plan'}-pb{pb}" for k, t, pb in IDENTITY])
def test_identity_permutation_is_the_screen_itself(kind, tile, pb, monkeypatch):
    """Row 0 is the identity: its max_r2 is best_r^2 of aq_prep_marginal on the same handle to the bit (every output element
    is accumulated over the samples in the same order, whatever the tile edge and PB), and its counts are the screen's."""
    from atlasqtl_amd import prepare as P
    n, p, q = 50, 130, 67
    X, Y = MU.case(n, p, q, kind)
    perms = np.stack([np.arange(n), np.random.default_rng(8).permutation(n)]).astype(np.int32)
    cut = np.full(q, 0.05)
    _set_env(monkeypatch, tile, pb)
    prep = P.prepare_on_device(Y, X)[0]
    try:
        plain = prep.marginal(cut, 0)
        nul = prep.marginal_permute(cut, perms)
    finally:
        prep.close()
    has = plain["best_snp"] >= 0
    want = np.where(has, plain["best_r"] * plain["best_r"], -1.0)
    assert nul["max_r2"][0].tobytes() == want.tobytes()
    assert has.sum() >= q - 1 and plain["rs"].max() > 1
    assert nul["hs_max"][0] == plain["rs"].max() and nul["n_sel"][0] == plain["n_pairs"] == plain["rs"].sum()
    assert nul["n_undef"][0] == plain["n_undefined"]
    assert nul["max_r2"][1].tobytes() != want.tobytes()        # the other row is another statistic
    assert nul["max_r2"][1][0] < 0.5 < want[0]                 # trait 0 is 3 x_0 + noise: the permutation breaks the link


def test_permuting_y_by_pi_is_permuting_x_by_its_inverse():
    """Y'[i] = Y[pi[i]] pairs sample i of X with sample pi[i] of Y: the pairs of (X[inv], Y), inv = pi^-1.  The plain screen
    of a handle prepared from (X[inv], Y), raw and complete, must agree with the permutation entry on the handle of (X, Y):
    best_r^2 against max_r2 within the sum of the two tolerances, each derived on its own handle's matrices.  The two
    preparations standardise the same columns in another row order, a difference of a few 2^-53 per element, far inside
    bounds that allow (n + 2) 2^-53 per term.  A gather by pi^-1 instead of pi fails this by O(1)."""
    from atlasqtl_amd import prepare as P
    n, p, q = 50, 130, 67
    X, Y = MU.case(n, p, q, None)
    pi = np.random.default_rng(21).permutation(n).astype(np.int32)
    inv = np.argsort(pi)
    assert not np.array_equal(pi, inv)
    cut = np.full(q, np.inf)
    a = P.prepare_on_device(Y, X)[0]
    try:
        nul = a.marginal_permute(cut, pi[None, :])
        best_a, tol_a, _ = _tol(*MU.reference(a.X_host(), a.Y[pi], 0)[:2])
    finally:
        a.close()
    b = P.prepare_on_device(Y, np.asfortranarray(X[inv]))[0]
    try:
        plain = b.marginal(cut, 0)
        best_b, tol_b, _ = _tol(*MU.reference(b.X_host(), b.Y, 0)[:2])
    finally:
        b.close()
    got, want = nul["max_r2"][0], plain["best_r"] ** 2
    ratio = np.abs(got - want) / (tol_a + tol_b)
    print(f"permuting Y by pi against permuting X by its inverse: worst |difference| / (sum of the tolerances) {float(ratio.max()):.3f}")
    assert (np.abs(got - want) <= tol_a + tol_b).all()
    wrong = MU.reference(X - X.mean(axis=0), (Y - Y.mean(axis=0))[inv], 0)[0]          # what a gather by pi^-1 would give
    assert np.max(np.abs(np.nanmax(np.asarray(wrong, dtype=np.float64) ** 2, axis=0) - want)) > 1e-3


def test_bad_arguments_are_refused_before_any_launch(monkeypatch):
    from atlasqtl_amd import _lib
    from atlasqtl_amd import prepare as P
    n, p, q = 37, 70, 5
    X, Y = MU.case(n, p, q, None)
    _set_env(monkeypatch)
    prep = P.prepare_on_device(Y, X)[0]
    L = _lib.lib()
    i64 = C.POINTER(C.c_int64)
    none = (None, C.cast(None, i64), C.cast(None, i64), C.cast(None, i64))
    try:
        cut = np.full(q, 0.1)
        good = _perms(n, 3, 1)
        bad = cut.copy()
        bad[3] = np.nan
        assert L.aq_prep_marginal_perm(prep.handle, _lib.as_dp(bad), 3, _lib.as_ip(good), *none) == 1
        assert b"aq_prep_marginal_perm: r2_cut[3] is NaN" in L.aq_last_error()
        rep = good.copy()
        rep[2, 5] = rep[2, 6]
        assert L.aq_prep_marginal_perm(prep.handle, _lib.as_dp(cut), 3, _lib.as_ip(rep), *none) == 1
        msg = L.aq_last_error()
        assert b"aq_prep_marginal_perm: row 2 of perm" in msg and b"repeated" in msg
        for v in (n, -1, 2 ** 31 - 1):
            far = good.copy()
            far[1, 0] = v
            assert L.aq_prep_marginal_perm(prep.handle, _lib.as_dp(cut), 3, _lib.as_ip(far), *none) == 1
            msg = L.aq_last_error()
            assert b"aq_prep_marginal_perm: row 1 of perm" in msg and b"out of range" in msg
        with pytest.raises(_lib.AtlasqtlHipError, match="row 2 of perm"):
            prep.marginal_permute(cut, rep)
        for name, v in (("AQ_MSPERM_PB", "3"), ("AQ_MSPERM_PB", "abc"), ("AQ_MSPERM_BATCH", "0"), ("AQ_MSCREEN_TILE", "32")):
            _set_env(monkeypatch)
            monkeypatch.setenv(name, v)
            with pytest.raises(_lib.AtlasqtlHipError, match=name):
                prep.marginal_permute(cut, good)
        _set_env(monkeypatch, 128, 2)                            # no such instance
        with pytest.raises(_lib.AtlasqtlHipError, match="AQ_MSPERM_PB"):
            prep.marginal_permute(cut, good)
        _set_env(monkeypatch, 64, 2, 3)                          # no multiple of PB
        with pytest.raises(_lib.AtlasqtlHipError, match="AQ_MSPERM_BATCH"):
            prep.marginal_permute(cut, good)
        _set_env(monkeypatch)
        ms, plan = C.c_double(0.0), _lib.AqMspermPlan()
        _lib.check(L.aq_prep_marginal_perm_time(prep.handle, 3, 1, C.byref(ms), C.byref(plan)), "aq_prep_marginal_perm_time")
        assert ms.value > 0 and plan.batch >= 3 and plan.launches == 1 and plan.masked == 0
    finally:
        prep.close()


# ---- the Python layer ----
E2E = (120, 90, 40)
SPEC = {"n": 19, "seed": 3}
SUMMARY_KEYS = ("trait_pvalue", "hotspot_pvalue", "expected_null_pairs", "empirical_fdr")
ALL_KEYS = {"n", "seed", "max_r2", "hotspot_max", "n_selected", "n_undefined", "r2_cut"} | set(SUMMARY_KEYS)


def _direct(X, Y, cut, res):
    """marginal_permute with the numpy-recipe permutations on a handle of one's own, and the summary of it."""
    from atlasqtl_amd import marginal as M
    from atlasqtl_amd import prepare as P
    perms = _perms(E2E[0], SPEC["n"], SPEC["seed"])
    prep = P.prepare_on_device(Y, X)[0]
    try:
        nul = prep.marginal_permute(cut, perms)
    finally:
        prep.close()
    return nul, M.permutation_summary(nul["max_r2"], nul["hs_max"], nul["n_sel"], res["best_snp"], res["best_r"], res["rs_thres"],
                                      res["nb_pairwise"])


def _same(perm, nul, summ, cut):
    assert set(perm) == ALL_KEYS
    for key, want in (("max_r2", nul["max_r2"]), ("hotspot_max", nul["hs_max"]), ("n_selected", nul["n_sel"]),
                      ("n_undefined", nul["n_undef"]), ("r2_cut", cut)):
        np.testing.assert_array_equal(perm[key], want, err_msg=key)
    for key in SUMMARY_KEYS:
        np.testing.assert_array_equal(perm[key], summ[key], err_msg=key)


@pytest.mark.parametrize("kind", [None, "random"])
def test_api_end_to_end(kind, monkeypatch):
    import atlasqtl_amd as A
    from atlasqtl_amd import marginal as M
    _set_env(monkeypatch)
    n, p, q = E2E
    X, Y = MU.case(n, p, q, kind)
    plain = A.marginal_screen(Y, X, p_value=1e-3)
    assert "permutation" not in plain
    res = A.marginal_screen(Y, X, p_value=1e-3, permutations=SPEC)
    for key in ("rs_thres", "best_snp", "best_r", "n_obs", "df"):            # the screen itself is what it was
        np.testing.assert_array_equal(res[key], plain[key])
    perm = res["permutation"]
    assert (perm["n"], perm["seed"]) == (19, 3) and perm["max_r2"].shape == (19, q)
    np.testing.assert_array_equal(perm["r2_cut"], res["threshold"]["r2_cut"])
    nul, summ = _direct(X, Y, res["threshold"]["r2_cut"], res)
    _same(perm, nul, summ, res["threshold"]["r2_cut"])
    # what the numbers must say here: trait 0 is 3 x_0 + noise, no permutation reaches it; the p-values lie on the grid k / 20
    assert perm["trait_pvalue"][0] == 1 / 20
    k = perm["trait_pvalue"] * 20
    assert np.all((k == np.round(k)) | np.isnan(k)) and np.nanmax(perm["trait_pvalue"]) <= 1.0
    assert np.all(perm["hotspot_pvalue"][res["rs_thres"] == 0] == 1.0)
    assert perm["expected_null_pairs"] == np.mean(nul["n_sel"]) and 0.0 <= perm["empirical_fdr"] <= 1.0
    # an explicit array gives what the seed that generates it gives, and reports no seed
    explicit = A.marginal_screen(Y, X, p_value=1e-3, permutations=_perms(n, 19, 3))["permutation"]
    assert explicit["seed"] is None and explicit["n"] == 19
    _same({**explicit, "seed": 3}, nul, summ, res["threshold"]["r2_cut"])
    # Bonferroni: the device's own cutoff again
    bon = A.marginal_screen(Y, X, permutations=SPEC)
    np.testing.assert_array_equal(bon["permutation"]["r2_cut"], bon["threshold"]["r2_cut"])
    # fdr: the cutoff of the largest p-value that the Benjamini-Hochberg cut kept
    fdr = A.marginal_screen(Y, X, fdr=0.05, permutations=SPEC)
    assert fdr["assoc"]["n_pairs"] > 0 and len(fdr["assoc"]["pvalue"]) == fdr["assoc"]["n_pairs"]
    cut = M.r2_cutoff(float(np.max(fdr["assoc"]["pvalue"])), fdr["df"])
    assert np.all(cut >= fdr["threshold"]["r2_cut"])             # the kept set is a subset of the device's selection
    nul_f, summ_f = _direct(X, Y, cut, fdr)
    _same(fdr["permutation"], nul_f, summ_f, cut)
    # ... and +inf everywhere when it kept nothing
    empty = A.marginal_screen(Y, X, fdr=1e-300, permutations=SPEC)
    assert empty["assoc"]["n_pairs"] == 0
    pe = empty["permutation"]
    assert np.all(np.isinf(pe["r2_cut"])) and not pe["n_selected"].any() and not pe["hotspot_max"].any()
    assert pe["expected_null_pairs"] == 0.0 and pe["empirical_fdr"] == 0.0 and np.all(pe["hotspot_pvalue"] == 1.0)
    np.testing.assert_array_equal(pe["max_r2"], perm["max_r2"])  # the maxima do not depend on the cutoff


def test_api_with_covariates(monkeypatch):
    import atlasqtl_amd as A
    _set_env(monkeypatch)
    n, p, q = E2E
    X, Y = MU.case(n, p, q, None)
    Z = np.random.default_rng(2).standard_normal((n, 3))
    res = A.marginal_screen(Y, X, p_value=1e-3, covariates=Z, permutations=SPEC)
    assert (res["df"] == n - 2 - 3).all() and res["n_covariates"] == 3
    perm = res["permutation"]
    assert set(perm) == ALL_KEYS and perm["max_r2"].shape == (19, q) and (perm["max_r2"] >= 0).all() and (perm["max_r2"] < 1).all()
    assert not perm["n_undefined"].any() and perm["trait_pvalue"][0] == 1 / 20
