"""GPU: the marginal screen of a prepared handle (aq_prep_marginal, csrc/aq_mscreen_kernels.h, csrc/aq_screen_tile.h) against the long-double
restatement of tests/mscreen_util.py run on the handle's own matrices, at shapes chosen for the kernels' edges: below one tile
(20, 3, 1), (50, 17, 5); odd n with p and q off every multiple of 16 and of 4 (333, 257, 33); one element past 128 and 64 in
every dimension (257, 130, 130); many sample chunks (1000, 300, 70); many predictor tiles (130, 1000, 20).  Every shape runs
complete under both tile edges that AQ_MSCREEN_TILE can force (64, 128) and under the plan's own choice, and with missing
values (one tile edge exists there): 10 % NaN at random, one trait fully observed among masked ones, and one trait with very
few observed values -- m_t = 3 where the preparation accepts such a trait (n <= 120), else the fewest its guard against traits
with more than 97.5 % missing values allows, ceil(0.025 n).  At q = 1 the kind "one trait fully observed" is the complete case
and is not repeated.

The error / bound ratios these tests print on an MI355X are recorded in DESIGN.md section 9."""
import functools

import numpy as np
import pytest

from tests import mscreen_util as MU

pytestmark = pytest.mark.gpu

SHAPES = [(20, 3, 1), (50, 17, 5), (333, 257, 33), (257, 130, 130), (1000, 300, 70), (130, 1000, 20)]
RUNS = [(s, None, tile) for s in SHAPES for tile in (None, 64, 128)] + \
       [(s, kind, None) for s in SHAPES for kind in MU.MISSING_KINDS if not (kind == "one_complete" and s[2] == 1)]
IDS = [f"{n}x{p}x{q}-{kind or 'complete'}-{tile or 'plan'}" for (n, p, q), kind, tile in RUNS]


def _set_tile(monkeypatch, tile):
    if tile is None:
        monkeypatch.delenv("AQ_MSCREEN_TILE", raising=False)
    else:
        monkeypatch.setenv("AQ_MSCREEN_TILE", str(tile))


@functools.lru_cache(maxsize=None)
def _case(shape, kind, n_cov=0, few_m=None):
    """(X, Y as given, covariates or None, r_ref, bound, m, df, cutoffs, the reference's selection), once per case."""
    from atlasqtl_amd import prepare as P
    n, p, q = shape
    X, Y = MU.case(n, p, q, kind, few_m=few_m)
    Z = None if n_cov == 0 else np.asfortranarray(np.random.default_rng(5).standard_normal((n, n_cov)))
    prep = P.prepare_on_device(Y, X, covariates=Z)[0]
    Xs, Yc = prep.X_host(), prep.Y
    assert prep.p == p and prep.n_cov == n_cov                # x and -x are both kept
    prep.close()
    r_ref, B, m, df = MU.reference(Xs, Yc, n_cov)
    cut = MU.clear_cutoffs(r_ref)
    sel = MU.selection(r_ref, cut)
    for a in (X, Y, r_ref, B, cut):
        a.setflags(write=False)
    return X, Y, Z, r_ref, B, m, df, cut, sel


def _rows(out):
    return set(zip(MU.int_list(out["snp"]), MU.int_list(out["trait"])))


def _check(prep, case, label):
    """Dense r within the bound, NaN exactly where the reference is undefined, the selection equal to the reference's, two
    calls the same bits."""
    X, Y, Z, r_ref, B, m, df, cut, (rows_ref, rs_ref, nundef_ref, best_ref) = case
    assert MU.cutoffs_are_clear(r_ref, cut)                    # no reference r^2 within 1e-9 of its trait's cutoff
    p, q = r_ref.shape
    out = prep.marginal(cut, p * q, dense=True)
    out2 = prep.marginal(cut, p * q, dense=True)
    r = out["r_dense"]
    assert r.shape == (p, q) and r.flags.f_contiguous
    undef = np.isnan(np.asarray(r_ref, dtype=np.float64))
    np.testing.assert_array_equal(np.isnan(r), undef)
    err = np.abs(r.astype(MU.LD) - r_ref)[~undef]
    ratio = float(np.max(err / B[~undef])) if err.size else 0.0
    print(f"{label}: worst |error| / bound {ratio:.3f} (bound factor {MU.FACTOR}), {len(rows_ref)} selected, {nundef_ref} undefined")
    assert (err <= B[~undef]).all()
    assert r.tobytes() == out2["r_dense"].tobytes()
    for key in ("rs", "best_snp", "best_r"):
        assert out[key].tobytes() == out2[key].tobytes(), key
    assert (out["n_pairs"], out["n_undefined"]) == (out2["n_pairs"], out2["n_undefined"])
    assert _rows(out) == _rows(out2)
    # the selection
    assert out["n_pairs"] == len(rows_ref) == len(out["snp"])
    assert _rows(out) == rows_ref
    np.testing.assert_array_equal(r[out["snp"], out["trait"]], out["r"])       # a row's r is the dense one
    np.testing.assert_array_equal(out["rs"], rs_ref)
    assert out["n_undefined"] == nundef_ref
    np.testing.assert_array_equal(out["best_snp"], best_ref)
    has = best_ref >= 0
    np.testing.assert_array_equal(out["best_r"][has], r[best_ref[has], np.nonzero(has)[0]])
    assert np.isnan(out["best_r"][~has]).all()
    return out


@pytest.mark.parametrize("shape,kind,tile", RUNS, ids=IDS)
def test_screen_against_long_double(shape, kind, tile, monkeypatch):
    from atlasqtl_amd import prepare as P
    case = _case(shape, kind)
    X, Y = case[0], case[1]
    n, p, q = shape
    _set_tile(monkeypatch, tile)
    prep = P.prepare_on_device(Y, X)[0]
    try:
        out = _check(prep, case, IDS[RUNS.index((shape, kind, tile))])
        best = out["best_snp"]
        assert best[0] == 0                                    # x and -x tie exactly on trait 0: the lower index wins
        assert out["r_dense"][0, 0] == -out["r_dense"][1, 0]
        if kind is not None:                                   # predictor 2 is constant where the last trait is observed
            assert np.isnan(out["r_dense"][2, q - 1]) and out["n_undefined"] >= 1
        else:
            assert out["n_undefined"] == 0
        # cap = 0 only counts; a table shorter than the selection still reports all of it
        cnt = prep.marginal(case[7], 0)
        assert cnt["n_pairs"] == out["n_pairs"] and cnt["snp"].size == 0
        np.testing.assert_array_equal(cnt["rs"], out["rs"])
        if out["n_pairs"] > 1:
            part = prep.marginal(case[7], out["n_pairs"] - 1)
            assert part["n_pairs"] == out["n_pairs"] and part["snp"].size == out["n_pairs"] - 1
            assert _rows(part) < _rows(out)
    finally:
        prep.close()


@pytest.mark.parametrize("kind", [None, "few"])
def test_covariates_take_degrees_of_freedom(kind):
    """With d covariates df = m - 2 - d, and a trait with df < 1 is undefined for every predictor: with d = 2 the trait with
    m = 4 observed values has df = 0 (with m = 3 the preparation refuses the covariates as collinear on its rows)."""
    from atlasqtl_amd import prepare as P
    shape, d = (50, 17, 5), 2
    case = _case(shape, kind, d, 4)
    X, Y, Z, r_ref, B, m, df = case[:7]
    np.testing.assert_array_equal(df, m - 2 - d)
    prep = P.prepare_on_device(Y, X, covariates=Z)[0]
    try:
        out = _check(prep, case, f"covariates d={d} {kind or 'complete'}")
        if kind == "few":
            assert m[-1] == 4 and df[-1] == 0
            assert np.isnan(out["r_dense"][:, -1]).all() and out["best_snp"][-1] == -1 and np.isnan(out["best_r"][-1])
            assert out["n_undefined"] >= shape[1]
    finally:
        prep.close()


def test_bad_arguments_are_refused(monkeypatch):
    from atlasqtl_amd import _lib
    from atlasqtl_amd import prepare as P
    case = _case((50, 17, 5), None)
    prep = P.prepare_on_device(case[1], case[0])[0]
    try:
        bad = np.array(case[7])
        bad[2] = np.nan
        with pytest.raises(_lib.AtlasqtlHipError, match="NaN"):
            prep.marginal(bad, 4)
        with pytest.raises(_lib.AtlasqtlHipError, match="cap"):
            prep.marginal(case[7], -1)
        for tile in ("0", "32", "abc"):
            monkeypatch.setenv("AQ_MSCREEN_TILE", tile)
            with pytest.raises(_lib.AtlasqtlHipError, match="AQ_MSCREEN_TILE"):
                prep.marginal(case[7], 4)
    finally:
        prep.close()


# ---- the Python layer ----
E2E = (200, 60, 12)


@functools.lru_cache(maxsize=None)
def _e2e():
    n, p, q = E2E
    rng = np.random.default_rng(11)
    X = rng.binomial(2, 0.3, size=(n, p)).astype(np.float64)
    Y = rng.standard_normal((n, q))
    for k in range(q):
        Y[:, k] += 0.7 * X[:, 3 * k] + 0.5 * (k + 1) / q * X[:, 3 * k + 1]
    return np.asfortranarray(X), np.asfortranarray(Y)


def _pearson(X, Y):
    """scipy.stats.pearsonr per pair: (r, p-value), p x q each."""
    from scipy.stats import pearsonr
    p, q = X.shape[1], Y.shape[1]
    r, pv = np.empty((p, q)), np.empty((p, q))
    for s in range(p):
        for t in range(q):
            r[s, t], pv[s, t] = pearsonr(X[:, s], Y[:, t])
    return r, pv


def test_end_to_end_against_pearsonr():
    """marginal_screen on raw inputs, complete Y, no covariates, against scipy.stats.pearsonr per pair: r within the util's
    bound (taken in long double on the centred raw columns: r does not change with the scale of a column), the p-value to rtol
    1e-6 where |r| <= 0.9 -- the bound on r carries through to a few 1e-8 in p there."""
    import atlasqtl_amd as A
    X, Y = _e2e()
    n, p, q = E2E
    res = A.marginal_screen(Y, X, p_value=1.0, dense=True)
    assert res["p"] == p and res["assoc"]["n_pairs"] == p * q == len(res["assoc"]["snp"])
    r_sp, p_sp = _pearson(X, Y)
    B = MU.reference(X - X.mean(axis=0), Y - Y.mean(axis=0))[1]
    a = res["assoc"]
    err = np.abs(a["r"] - r_sp[a["snp"], a["trait"]])
    print(f"end to end: worst |r - pearsonr| / bound {float(np.max(err / B[a['snp'], a['trait']])):.3f}, worst |r - pearsonr| "
          f"{float(np.max(err)):.2e}")
    assert (err <= B[a["snp"], a["trait"]]).all()
    assert (a["df"] == n - 2).all() and (res["df"] == n - 2).all() and (res["n_obs"] == n).all()
    np.testing.assert_allclose(a["t"], a["r"] * np.sqrt((n - 2) / (1 - a["r"] ** 2)), rtol=1e-12)
    ok = np.abs(a["r"]) <= 0.9
    assert ok.sum() > 0.9 * p * q
    np.testing.assert_allclose(a["pvalue"][ok], p_sp[a["snp"], a["trait"]][ok], rtol=1e-6)
    np.testing.assert_array_equal(res["r"][a["snp"], a["trait"]], a["r"])
    assert (np.diff(a["pvalue"]) >= 0).all()
    np.testing.assert_array_equal(res["best_snp"], np.argmax(res["r"] ** 2, axis=0))
    np.testing.assert_array_equal(res["rs_thres"], np.full(p, q))


def _host_bh(pv_dense, alpha):
    """Benjamini-Hochberg over the dense p-values: (q-values p x q, the selected set)."""
    flat = pv_dense.ravel(order="F")
    order = np.argsort(flat, kind="stable")
    M = flat.size
    raw = flat[order] * M / np.arange(1, M + 1)
    qs = np.minimum(np.minimum.accumulate(raw[::-1])[::-1], 1.0)
    qv = np.empty(M)
    qv[order] = qs
    qv = qv.reshape(pv_dense.shape, order="F")
    return qv, set(zip(*(MU.int_list(v) for v in np.nonzero(qv <= alpha))))


def test_fdr_mode_is_benjamini_hochberg():
    import atlasqtl_amd as A
    from atlasqtl_amd import marginal as M
    X, Y = _e2e()
    n, p, q = E2E
    alpha = 0.05
    full = A.marginal_screen(Y, X, p_value=1.0, dense=True)
    pv = M.t_and_pvalue(full["r"], n - 2)[1]
    qv_ref, set_ref = _host_bh(pv, alpha)
    res = A.marginal_screen(Y, X, fdr=alpha)
    a = res["assoc"]
    assert 0 < len(set_ref) < p * q
    assert set(zip(MU.int_list(a["snp"]), MU.int_list(a["trait"]))) == set_ref
    assert a["n_pairs"] == res["nb_pairwise"] == len(set_ref)
    np.testing.assert_allclose(a["qvalue"], qv_ref[a["snp"], a["trait"]], rtol=1e-12)
    np.testing.assert_array_equal(res["rs_thres"], np.bincount(a["snp"], minlength=p))
    assert res["threshold"]["mode"] == "fdr" and res["threshold"]["n_tests"] == p * q


def test_second_call_returns_the_complete_table(monkeypatch):
    """A first table too short for the selection: the call is repeated once with cap = n_pairs, and the result is the one of
    a first table that was long enough."""
    import atlasqtl_amd as A
    from atlasqtl_amd import marginal as M
    X, Y = _e2e()
    want = A.marginal_screen(Y, X, p_value=0.01)
    assert want["assoc"]["n_pairs"] > 8
    monkeypatch.setattr(M, "INITIAL_CAP", 8)
    got = A.marginal_screen(Y, X, p_value=0.01)
    for key in ("snp", "trait", "r", "t", "pvalue", "qvalue"):
        np.testing.assert_array_equal(got["assoc"][key], want["assoc"][key])
    assert got["assoc"]["n_pairs"] == want["assoc"]["n_pairs"]
    cut = A.marginal_screen(Y, X, p_value=0.01, max_pairs=5)
    assert len(cut["assoc"]["snp"]) == 5 and cut["assoc"]["n_pairs"] == want["assoc"]["n_pairs"]
    np.testing.assert_array_equal(cut["assoc"]["snp"], want["assoc"]["snp"][:5])
    np.testing.assert_array_equal(cut["rs_thres"], want["rs_thres"])


def test_atlasqtl_runs_the_screen_on_its_own_handle():
    import atlasqtl_amd as A
    X, Y = _e2e()
    fit = A.atlasqtl(Y, X, p0=(2, 4), verbose=0, marginal_screen=True)
    alone = A.marginal_screen(Y, X)
    m = fit["marginal"]
    assert m["threshold"]["mode"] == "bonferroni" and m["threshold"]["level"] == 0.05 / (E2E[1] * E2E[2])
    for key in ("snp", "trait", "r", "t", "pvalue", "qvalue", "df"):
        np.testing.assert_array_equal(m["assoc"][key], alone["assoc"][key])
    assert list(m["assoc"]["snp_name"]) == list(alone["assoc"]["snp_name"])
    for key in ("rs_thres", "best_snp", "best_r", "best_pvalue", "n_obs", "df"):
        np.testing.assert_array_equal(m[key], alone[key])
    assert m["nb_pairwise"] == alone["nb_pairwise"] > 0 and m["n_undefined"] == alone["n_undefined"] == 0
    with_dict = A.atlasqtl(Y, X, p0=(2, 4), verbose=0, marginal_screen={"p_value": 0.01, "max_pairs": 4})
    assert len(with_dict["marginal"]["assoc"]["snp"]) == 4
    assert "marginal" not in A.atlasqtl(Y, X, p0=(2, 4), verbose=0)


def test_covariates_and_names(tmp_path):
    """df = n - 2 - d with covariates; a PlinkBed names the predictors by its .bim."""
    import atlasqtl_amd as A
    from tests.bed_util import write_fileset
    X, Y = _e2e()
    n, p, q = E2E
    Z = np.random.default_rng(2).standard_normal((n, 3))
    res = A.marginal_screen(Y, X, p_value=0.01, covariates=Z)
    assert (res["df"] == n - 2 - 3).all() and (res["assoc"]["df"] == n - 5).all() and res["n_covariates"] == 3
    G = X.astype(np.int8)
    prefix = str(tmp_path / "geno")
    ids = write_fileset(prefix, G)[0]
    got = A.marginal_screen(Y, A.PlinkBed(prefix), p_value=0.01)
    assert got["names_x"] == ids and got["assoc"]["n_pairs"] > 0
    assert list(got["assoc"]["snp_name"]) == [ids[j] for j in got["assoc"]["snp"]]
    assert list(got["assoc"]["trait_name"]) == [f"Resp_{k + 1}" for k in got["assoc"]["trait"]]
