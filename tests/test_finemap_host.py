"""Cis fine-mapping without a GPU: the two restatements of tests/finemap_util.py against each other, the ELBO of the reference,
the credible sets (atlasqtl_amd.cis_susie.credible_sets_) on hand-made rows and against the full vector, the planner
(aq_finemap_plan_query) and the argument errors of the entries."""
import ctypes as C

import numpy as np
import pytest

import atlasqtl_amd as A
from atlasqtl_amd import _lib
from atlasqtl_amd import cis_susie as CIS
from tests import finemap_util as FU

LD = FU.LD
CASES = [((50, 17, 5), "all", 1), ((50, 17, 5), "band", 3), ((60, 40, 6), "band", 10), ((20, 5, 2), "all", 3)]


def _inputs(shape, pattern):
    n, p, q = shape
    Xs, Yc = FU.prepared(*FU.case(n, p, q))
    lo, hi = FU.windows(pattern, p, q)
    return Xs, Yc, lo, hi


@pytest.mark.parametrize("shape,pattern,L", CASES)
def test_the_two_restatements_agree(shape, pattern, L):
    """alpha, mu, V, sigma2 and the ELBO trace of the sufficient-statistics form against the definition, both in long double,
    after 1, 2 and 8 iterations: within 16 x the deviation of the definition run in float64 from itself in long double."""
    Xs, Yc, lo, hi = _inputs(shape, pattern)
    assert (Xs[:, FU.ZERO_COL] == 0).all() and lo[0] <= FU.ZERO_COL < hi[0]
    if pattern == "band" and shape[2] > 4:
        assert hi[4] == lo[4]                                  # an empty window
    ref = FU.reference(Xs, Yc, lo, hi, L, 8, snapshots=(1, 2, 8))
    r64 = FU.reference(Xs, Yc, lo, hi, L, 8, dtype=np.float64, snapshots=(1, 2, 8))
    for k in (1, 2, 8):
        ss = FU.reference_ss(Xs, Yc, lo, hi, L, k)
        a, b = dict(ref["snaps"][k], elbo=ref["elbo"][:k]), dict(r64["snaps"][k], elbo=r64["elbo"][:k])
        for key in ("alpha", "mu", "V", "sigma2", "elbo"):
            e64, _ = FU.deviation(b, a, key)
            dis, _ = FU.deviation(ss, a, key)
            print(f"{shape} {pattern} L={L} after {k}: {key}: the restatements disagree by {float(dis.max()):.2e}, float64 deviates by "
                  f"{float(e64.max()):.2e}")
            assert (dis <= 16 * e64).all(), (key, k)
            assert float(e64.max()) > 0
    assert ref["n_undef"][0] == 1 and (ref["n_iter"][hi > lo] == 8).all() and (ref["n_iter"][hi == lo] == 0).all()
    assert np.isnan(ref["sigma2"][hi == lo].astype(float)).all()


@pytest.mark.parametrize("shape,pattern,L", CASES)
def test_the_elbo_of_the_reference_does_not_decrease(shape, pattern, L):
    """Every step of the ELBO trace is >= 0, but for the steps that follow an iteration whose null check set a prior variance of
    the trait to 0: that is no EM step -- the check compares the single effect's marginal likelihoods on the residual it saw,
    the effect is emptied one iteration later on another residual -- and it does lower the ELBO in these inputs (by up to 0.6
    at the GPU tests' shapes).  The steps that remain are most of them."""
    Xs, Yc, lo, hi = _inputs(shape, pattern)
    iters = 12
    ref = FU.reference(Xs, Yc, lo, hi, L, iters)
    el, Vt = ref["elbo"], ref["V_trace"]
    clean = total = 0
    for t in np.nonzero(hi > lo)[0]:
        for it in range(1, iters):
            before = Vt[it - 2, t] if it >= 2 else np.ones(L)
            zeroed = bool(np.any((Vt[it - 1, t] == 0) & (before > 0)))
            total += 1
            if not zeroed:
                clean += 1
                assert el[it, t] - el[it - 1, t] >= -LD(1e-15) * abs(el[it, t]), (t, it)
    assert clean >= total // 2


def _rows(entries):
    snp, trait, effect, alpha = zip(*entries)
    return dict(snp=np.array(snp), trait=np.array(trait), effect=np.array(effect), alpha=np.array(alpha), mu=np.ones(len(snp)))


def test_credible_sets_on_hand_made_rows():
    V = np.array([[1.0, 1.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0]])
    rows = _rows([
        # trait 0, effect 0: 0.5 + 0.3 + 0.15 = 0.95 exactly: the prefix of three reaches the coverage, not before
        (7, 0, 0, 0.15), (3, 0, 0, 0.5), (5, 0, 0, 0.3), (9, 0, 0, 0.05),
        # trait 0, effect 1: ties in alpha go to the lower predictor: 0.4, then 2 before 8 before 11
        (11, 0, 1, 0.2), (8, 0, 1, 0.2), (2, 0, 1, 0.2), (4, 0, 1, 0.4),
        # trait 0, effect 2: V = 0 gives no set
        (1, 0, 2, 1.0),
        # trait 0, effect 3: the predictors of effect 0 again: a duplicate, dropped
        (3, 0, 3, 0.6), (5, 0, 3, 0.2), (7, 0, 3, 0.19), (9, 0, 3, 0.01),
        # trait 1, effect 0: the same predictors as trait 0's effect 0, another trait: kept
        (3, 1, 0, 0.9), (5, 1, 0, 0.04), (7, 1, 0, 0.03),
    ])
    sets = CIS.credible_sets_(rows, V, 0.95)
    got = [(s["trait"], s["effect"], s["snp"].tolist()) for s in sets]
    assert got == [(0, 0, [3, 5, 7]), (0, 1, [4, 2, 8, 11]), (1, 0, [3, 5, 7])]
    assert sets[0]["alpha"].tolist() == [0.5, 0.3, 0.15] and sets[0]["mass"] == pytest.approx(0.95)
    assert CIS.credible_sets_(rows, V, 0.5)[0]["snp"].tolist() == [3]      # 0.5 is not below 0.5: one member suffices
    assert CIS.credible_sets_(rows, V, 0.51)[0]["snp"].tolist() == [3, 5]
    empty = dict(snp=np.zeros(0, int), trait=np.zeros(0, int), effect=np.zeros(0, int), alpha=np.zeros(0))
    assert CIS.credible_sets_(empty, V) == []


@pytest.mark.parametrize("coverage", [0.95, 0.5])
def test_the_row_threshold_gives_the_sets_of_the_full_vector(coverage):
    shape, L = (60, 40, 6), 4
    Xs, Yc, lo, hi = _inputs(shape, "band")
    ref = FU.reference(Xs, Yc, lo, hi, L, 8)
    alpha, V = np.asarray(ref["alpha"], dtype=np.float64), np.asarray(ref["V"], dtype=np.float64)
    P = (hi - lo) - ref["n_undef"]
    thr = CIS.row_threshold(1e-4, coverage, P)
    full, cut = [], []
    for t in np.nonzero(hi > lo)[0]:
        for l in range(L):
            for s in range(lo[t], hi[t]):
                full.append((s, t, l, alpha[t, l, s]))
                if alpha[t, l, s] >= thr[t]:
                    cut.append((s, t, l, alpha[t, l, s]))
    assert len(cut) < len(full)
    a, b = CIS.credible_sets_(_rows(full), V, coverage), CIS.credible_sets_(_rows(cut), V, coverage)
    assert len(a) == len(b) >= 2
    for x, y in zip(a, b):
        assert (x["trait"], x["effect"]) == (y["trait"], y["effect"]) and x["snp"].tolist() == y["snp"].tolist()
    lost = 1.0 - np.array([sum(r[3] for r in cut if r[1] == t and r[2] == l) for t in np.nonzero(hi > lo)[0] for l in range(L)])
    assert lost.max() < 0.1 * (1 - coverage)


def _plan(hiplib, n, p1, q, lo, hi, L):
    out = _lib.AqFinemapPlan()
    rc = hiplib.aq_finemap_plan_query(n, p1, q, 256, _lib.as_ip(lo), _lib.as_ip(hi), L, C.byref(out))
    return rc, out


def test_plan_query(hiplib, monkeypatch):
    monkeypatch.delenv("AQ_FM_BATCH_TILES", raising=False)
    n, p1, q, L = 500, 20000, 6400, 16
    centre = np.linspace(0, p1, q).astype(np.int64)
    lo = np.maximum(centre - 3200, 0).astype(np.int32)
    hi = np.minimum(centre + 3200, p1).astype(np.int32)
    rc, pl = _plan(hiplib, n, p1, q, lo, hi, L)
    assert rc == 0 and pl.L == L and pl.forced == 0
    tiles = pl.cis.trait_tiles
    assert tiles == 100 and pl.state_budget == 4 << 30
    # the batches partition the tiles: batch b is [b batch_tiles, (b + 1) batch_tiles), the last one cut at the end
    assert 1 <= pl.batch_tiles < tiles and pl.n_batches == -(-tiles // pl.batch_tiles) and pl.n_batches >= 2
    # the state of the largest batch stays within the budget, and one more tile per batch would not be known to
    assert pl.state_bytes <= pl.state_budget and pl.state_bytes > pl.state_budget // 2
    assert pl.state_bytes % (2 * L * 64 * 64 * 8) == 0 and pl.band_bytes * 2 * L == pl.state_bytes
    assert pl.fit_bytes == 8 * (L + 2) * n * 64 * pl.batch_tiles
    # a small problem is one batch
    rc, one = _plan(hiplib, 100, 300, 130, np.zeros(130, np.int32), np.full(130, 300, np.int32), 10)
    assert rc == 0 and one.cis.trait_tiles == 3 and one.batch_tiles == 3 and one.n_batches == 1
    assert one.state_bytes == 3 * 5 * 2 * 10 * 64 * 64 * 8
    # AQ_FM_BATCH_TILES is honoured and reported, also beyond the budget; more than the tiles is the tiles
    monkeypatch.setenv("AQ_FM_BATCH_TILES", "1")
    rc, f1 = _plan(hiplib, 100, 300, 130, np.zeros(130, np.int32), np.full(130, 300, np.int32), 10)
    assert rc == 0 and f1.forced == 1 and f1.batch_tiles == 1 and f1.n_batches == 3 and f1.state_bytes == one.state_bytes // 3
    monkeypatch.setenv("AQ_FM_BATCH_TILES", "64")
    rc, f64 = _plan(hiplib, n, p1, q, lo, hi, L)
    assert rc == 0 and f64.forced == 1 and f64.batch_tiles == 64 and f64.n_batches == 2 and f64.state_bytes > f64.state_budget
    monkeypatch.setenv("AQ_FM_BATCH_TILES", "1000")
    assert _plan(hiplib, n, p1, q, lo, hi, L)[1].batch_tiles == tiles
    monkeypatch.setenv("AQ_FM_BATCH_TILES", "0")
    assert _plan(hiplib, n, p1, q, lo, hi, L)[0] == 1 and b"AQ_FM_BATCH_TILES" in hiplib.aq_last_error()
    monkeypatch.delenv("AQ_FM_BATCH_TILES")
    # L = 0 and L = 17 are refused; so is a window outside the matrix; no window at all is no batch
    for bad in (0, 17):
        rc, z = _plan(hiplib, n, p1, q, lo, hi, bad)
        assert rc == 1 and b"L must lie in [1, 16]" in hiplib.aq_last_error() and z.L == 0
    assert _plan(hiplib, n, p1, q, lo, hi + 1, L)[0] == 1
    rc, none = _plan(hiplib, n, p1, q, lo, lo, L)
    assert rc == 0 and none.n_batches == 0 and none.batch_tiles == 0 and none.state_bytes == 0


def test_argument_errors_need_no_gpu(hiplib):
    z = np.zeros(3, dtype=np.int32)
    pm = _lib.AqFinemapParams(10, 100, 1e-3, 0.2, 0.95, 1e-4)
    tail = [None] * 17

    def call(lo, hi, params, cap=0, h=None):
        return hiplib.aq_prep_cis_finemap(h, None if lo is None else _lib.as_ip(lo), None if hi is None else _lib.as_ip(hi), None,
                                          None if params is None else C.byref(params), cap, *tail)
    assert call(None, z, pm) == 1 and b"aq_prep_cis_finemap: NULL s_lo" in hiplib.aq_last_error()
    assert call(z, z, None) == 1 and b"NULL params" in hiplib.aq_last_error()
    for field, bad, word in (("L", 0, b"L must lie"), ("L", 17, b"L must lie"), ("max_iter", 0, b"max_iter"), ("tol", -1.0, b"tol"),
                             ("tol", float("nan"), b"tol"), ("scaled_prior_variance", 0.0, b"scaled_prior_variance"),
                             ("coverage", 1.0, b"coverage"), ("alpha_min", 1.5, b"alpha_min")):
        p2 = _lib.AqFinemapParams(10, 100, 1e-3, 0.2, 0.95, 1e-4)
        setattr(p2, field, bad)
        assert call(z, z, p2) == 1 and word in hiplib.aq_last_error(), field
    assert call(z, z, pm, cap=-1) == 1 and b"cap >= 0" in hiplib.aq_last_error()
    assert call(z, z, pm) == 1 and b"NULL handle" in hiplib.aq_last_error()
    assert hiplib.aq_prep_set_purity(None, None, None, 0, None, None) == 1 and b"aq_prep_set_purity" in hiplib.aq_last_error()
    one = np.zeros(1)
    assert hiplib.aq_prep_cis_finemap_time(None, _lib.as_ip(z), _lib.as_ip(z), 10, 0, *[_lib.as_dp(one)] * 4, None) == 1
    assert hiplib.aq_prep_debug_set_column(None, 0, None) == 1
    # the public entry refuses its arguments before it prepares anything
    X, Y = np.zeros((8, 4)), np.zeros((8, 2))
    kw = dict(trait_chrom=["1", "1"], trait_start=[1, 2], snp_chrom=["1"] * 4, snp_pos=[1, 2, 3, 4])
    for bad in (dict(L=0), dict(L=17), dict(L=2.5), dict(coverage=1.0), dict(coverage=0.0), dict(min_abs_corr=1.5), dict(tol=-1e-3),
                dict(max_iter=0), dict(scaled_prior_variance=0.0), dict(alpha_min=2.0), dict(max_rows=0), dict(window=-1)):
        with pytest.raises(A.AtlasqtlError, match="cis_finemap"):
            A.cis_finemap(Y, X, **kw, **bad)
    with pytest.raises(A.AtlasqtlError, match="snp_chrom and snp_pos"):
        A.cis_finemap(Y, X, ["1", "1"], [1, 2])
    with pytest.raises(A.AtlasqtlError, match="traits="):
        CIS._traits_arg(["nope"], ["a", "b"])
    assert CIS._traits_arg([1, "a"], ["a", "b"]).tolist() == [True, True] and CIS._traits_arg(None, ["a"]) is None
