"""GPU: cis fine-mapping (aq_prep_cis_finemap, aq_prep_set_purity; csrc/aq_finemap_kernels.h) against the long-double
restatement of tests/finemap_util.py run on the handle's own matrices, against itself to the bit (two calls, the batches,
active=, a converged trait), against the plain cis scan, and end to end.

Shapes (n, p, q), those of the conditional scan's tests: (20, 5, 2) and (50, 17, 5) below one tile; (333, 257, 33) odd n,
nothing a multiple of 16; (257, 130, 130) one past 64 both ways, two to three trait tiles; (130, 1000, 20) many work items per
trait tile.  Each with the window patterns `all` and `band` of finemap_util.windows and with L = 1, 3 and 10.  Column
finemap_util.ZERO_COL of every handle is replaced by zeros (aq_prep_debug_set_column: the preparation would remove it)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import finemap_util as FU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = FU.LD
SHAPES = [(20, 5, 2), (50, 17, 5), (333, 257, 33), (257, 130, 130), (130, 1000, 20)]
RUNS = [(s, w, L) for s in SHAPES for w in FU.PATTERNS for L in (1, 3, 10)]
STATE = ("alpha_dense", "mu_dense", "V", "lbf", "sigma2", "elbo", "n_iter", "converged", "n_undef")


def _id(run):
    (n, p, q), pattern, L = run
    return f"{n}x{p}x{q}-{pattern}-L{L}"


def _handle(shape):
    """a fresh handle of the shape's inputs with the zero column planted"""
    from atlasqtl_amd import _lib
    from atlasqtl_amd import prepare as P
    n, p, q = shape
    X, Y = FU.case(n, p, q)
    prep = P.prepare_on_device(Y, X)[0]
    assert prep.p == p
    _lib.check(_lib.lib().aq_prep_debug_set_column(prep.handle, FU.ZERO_COL, _lib.as_dp(np.zeros(n))), "aq_prep_debug_set_column")
    return prep


@functools.lru_cache(maxsize=None)
def _matrices(shape):
    """Once per shape, shared and left unchanged: the handle's own matrices."""
    prep = _handle(shape)
    try:
        Xs, Yc = prep.X_host(), prep.Y.copy()
    finally:
        prep.close()
    assert (Xs[:, FU.ZERO_COL] == 0).all()
    Xs.setflags(write=False)
    Yc.setflags(write=False)
    return Xs, Yc


@functools.lru_cache(maxsize=None)
def _reference(shape, pattern, L):
    """Once per run, shared and left unchanged: the definition in long double and in float64, 8 iterations with the states
    after 1, 2 and 8."""
    Xs, Yc = _matrices(shape)
    lo, hi = FU.windows(pattern, shape[1], shape[2])
    return (FU.reference(Xs, Yc, lo, hi, L, 8, snapshots=(1, 2, 8)),
            FU.reference(Xs, Yc, lo, hi, L, 8, dtype=np.float64, snapshots=(1, 2, 8)))


def fit(shape, pattern, L, prep=None, **kw):
    lo, hi = FU.windows(pattern, shape[1], shape[2])
    own = prep is None
    prep = _handle(shape) if own else prep
    try:
        return prep.cis_finemap(lo, hi, L=L, dense=True, **kw)
    finally:
        if own:
            prep.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b, keys=STATE, traits=slice(None)):
    for key in keys:
        x, y = (np.moveaxis(v[key], 1, 0) if key == "elbo" else v[key] for v in (a, b))
        assert np.array_equal(_bits(x[traits]), _bits(y[traits])), key


@pytest.mark.parametrize("run", RUNS, ids=[_id(r) for r in RUNS])
def test_fixed_iterations_against_long_double(run):
    """tol = 0 and max_iter = 1, 2, 8: dense alpha, mu, V, sigma2, lbf and the ELBO trace against the long-double reference.
    Per trait and quantity the bar is 16 x max(e64, 64 ulp of the quantity's scale): e64 the deviation of the definition run
    in float64 from itself in long double, the scale the largest |reference value| of the trait, at least 1 for alpha and lbf
    (finemap_util.deviation says why).
    The ELBO also within 1e-9 relative, whatever is measured.  Two calls give the same bits."""
    shape, pattern, L = run
    n, p, q = shape
    lo, hi = FU.windows(pattern, p, q)
    ref, r64 = _reference(shape, pattern, L)
    # the reference first: the only decision that separates two evaluations is the null check, and every one that decides
    # anything (V_new > 0; at V_new = 0 the variance is 0 either way) is clear of 0
    assert all(m > 1e-6 for m in ref["margins"]), min(ref["margins"])
    assert ref["n_undef"][0] == 1 and lo[0] <= FU.ZERO_COL < hi[0]
    worst = 0.0
    prep = _handle(shape)
    try:
        for k in (1, 2, 8):
            got = fit(shape, pattern, L, prep, tol=0.0, max_iter=k)
            if k == 8:
                _same_bits(got, fit(shape, pattern, L, prep, tol=0.0, max_iter=k))
            g = dict(alpha=got["alpha_dense"], mu=got["mu_dense"], V=got["V"], sigma2=got["sigma2"], lbf=got["lbf"], elbo=got["elbo"])
            a, b = dict(ref["snaps"][k], elbo=ref["elbo"][:k]), dict(r64["snaps"][k], elbo=r64["elbo"][:k])
            for key in FU.QUANTITIES + ("elbo",):
                err, scale = FU.deviation(g, a, key)
                e64, _ = FU.deviation(b, a, key)
                bar = 16 * np.maximum(e64, 64 * 2.0 ** -52 * scale)
                ratio = float(np.max(err / bar))
                worst = max(worst, ratio)
                print(f"{_id(run)} after {k}: {key}: worst |gpu - reference| {float(err.max()):.2e}, float64's own {float(e64.max()):.2e}, "
                      f"worst error / bar {ratio:.3f}")
                assert (err <= bar).all(), (key, k, ratio)
            el = np.asarray(ref["elbo"][:k], dtype=np.float64)
            has = hi > lo
            assert np.all(np.abs(got["elbo"][:, has] - el[:, has]) <= 1e-9 * np.abs(el[:, has]))
            assert np.isnan(got["elbo"][:, ~has]).all()
            np.testing.assert_array_equal(got["n_iter"], np.where(has, k, 0))
            np.testing.assert_array_equal(got["n_undef"], ref["n_undef"])
            assert not got["converged"].any() and np.isnan(got["sigma2"][~has]).all()
    finally:
        prep.close()
    print(f"{_id(run)}: worst error / bar over all quantities and iterations {worst:.3f}")


BIT_RUNS = [((257, 130, 130), "all", 3, 4), ((333, 257, 33), "band", 10, 2), ((130, 1000, 20), "all", 1, 3)]


def test_the_batches_change_no_bit(tmp_path):
    """AQ_FM_BATCH_TILES = 1 in a child process gives the bits of the single batch of this process."""
    runs = [f"{n},{p},{q},{pattern},{L},{iters}" for (n, p, q), pattern, L, iters in BIT_RUNS]
    out = str(tmp_path / "batch1.npz")
    env = dict(os.environ, AQ_FM_BATCH_TILES="1")
    r = subprocess.run([sys.executable, "-m", "tests.finemap_child", out] + runs, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    child = np.load(out)
    assert "AQ_FM_BATCH_TILES" not in os.environ
    for (shape, pattern, L, iters), run in zip(BIT_RUNS, runs):
        here = fit(shape, pattern, L, tol=0.0, max_iter=iters)
        tiles = here["plan"]["trait_tiles"]
        assert here["plan"]["n_batches"] == 1 and here["plan"]["batch_tiles"] == tiles and here["plan"]["forced"] == 0
        assert int(child[f"batch_tiles_{run}"]) == 1 and int(child[f"n_batches_{run}"]) == tiles
        _same_bits(here, {key: child[f"{key}_{run}"] for key in STATE})
    assert max(fit(s, w, L, tol=0.0, max_iter=1)["plan"]["trait_tiles"] for s, w, L, _ in BIT_RUNS) >= 3


@pytest.mark.parametrize("shape,pattern,L,iters", BIT_RUNS)
def test_active_gives_the_bits_of_the_full_call(shape, pattern, L, iters):
    """active= for a subset: those traits get the bits they have in the full call, nothing is reported for the others."""
    q = shape[2]
    lo, hi = FU.windows(pattern, shape[1], q)
    active = np.zeros(q, dtype=bool)
    active[::3] = True
    active[-1] = True
    prep = _handle(shape)
    try:
        full = prep.cis_finemap(lo, hi, L=L, tol=0.0, max_iter=iters, dense=True, cap=L * shape[1] * q)
        part = prep.cis_finemap(lo, hi, L=L, tol=0.0, max_iter=iters, dense=True, cap=L * shape[1] * q, active=active)
    finally:
        prep.close()
    _same_bits(full, part, traits=active)
    off = ~active
    assert np.isnan(part["sigma2"][off]).all() and np.isnan(part["V"][off]).all() and np.isnan(part["lbf"][off]).all()
    assert np.isnan(part["elbo"][:, off]).all() and (part["n_iter"][off] == 0).all() and (part["n_undef"][off] == 0).all()
    assert (part["alpha_dense"][off] == 0).all() and not np.isin(part["trait"], np.nonzero(off)[0]).any()
    rows = lambda o: {(int(s), int(t), int(l)): (float(a), float(m)) for s, t, l, a, m in zip(o["snp"], o["trait"], o["effect"], o["alpha"], o["mu"])}
    want = {k: v for k, v in rows(full).items() if active[k[1]]}
    assert rows(part) == want and len(want) > 0


CONV_RUNS = [((257, 130, 130), "band", 10), ((130, 1000, 20), "band", 3), ((257, 130, 130), "all", 10)]


@pytest.mark.parametrize("shape,pattern,L", CONV_RUNS)
def test_convergence(shape, pattern, L):
    """The default tol: n_iter is the reference's for every trait whose last two ELBO steps in the reference are clear of tol
    (outside [tol / 2, 2 tol]), at least 3/4 of the traits with a window; traits stop at different iterations; and a trait
    that stopped after k iterations has, to the bit, the state of the run with tol = 0 and max_iter = k: it was not written
    again."""
    tol, max_iter = 1e-3, 100
    n, p, q = shape
    lo, hi = FU.windows(pattern, p, q)
    Xs, Yc = _matrices(shape)
    ref = FU.reference(Xs, Yc, lo, hi, L, max_iter, tol=tol, dtype=np.float64)
    el, ni = ref["elbo"], ref["n_iter"]
    has = hi > lo
    assert ref["converged"][has].all() and ni.max() < max_iter
    clear = np.zeros(q, dtype=bool)
    for t in np.nonzero(has)[0]:
        steps = [el[k, t] - el[k - 1, t] for k in (ni[t] - 2, ni[t] - 1) if k >= 1]
        clear[t] = all(not (tol / 2 <= s <= 2 * tol) for s in steps)
    assert clear.sum() * 4 >= has.sum() * 3, (clear.sum(), has.sum())
    prep = _handle(shape)
    try:
        got = fit(shape, pattern, L, prep, tol=tol, max_iter=max_iter)
        np.testing.assert_array_equal(got["n_iter"][clear], ni[clear])
        assert got["converged"][has].all() and not got["converged"][~has].any()
        stops = np.unique(got["n_iter"][has])
        print(f"{shape} {pattern} L={L}: {clear.sum()} of {has.sum()} traits clear of tol; the traits stop after {stops.tolist()} iterations")
        assert stops.size >= 3
        for k in {int(stops[0]), int(stops[stops.size // 2]), int(stops[-1])}:
            fixed = fit(shape, pattern, L, prep, tol=0.0, max_iter=k)
            at_k = got["n_iter"] == k
            assert at_k.any()
            _same_bits(got, fixed, keys=("alpha_dense", "mu_dense", "V", "lbf"), traits=at_k)
            assert np.array_equal(_bits(got["elbo"][:k, at_k]), _bits(fixed["elbo"][:, at_k])) and np.isnan(got["elbo"][k:, at_k]).all()
    finally:
        prep.close()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pattern", FU.PATTERNS)
def test_one_effect_against_the_cis_scan(shape, pattern):
    """L = 1, one iteration: every trait's top-alpha predictor is the best_snp of the plain cis scan where the reference's is
    clear of the runner-up; n_undef counts the zero column; the trait with an empty window gets nothing."""
    n, p, q = shape
    lo, hi = FU.windows(pattern, p, q)
    ref, _ = _reference(shape, pattern, 1)
    al = np.asarray(ref["snaps"][1]["alpha"][:, 0, :], dtype=np.float64)
    prep = _handle(shape)
    try:
        got = prep.cis_finemap(lo, hi, L=1, tol=0.0, max_iter=1, dense=True, cap=p * q)
        scan = prep.cis(lo, hi, np.full(q, np.inf), 0)
    finally:
        prep.close()
    has = hi > lo
    top = np.argsort(-al, axis=1, kind="stable")
    clear = has & (al[np.arange(q), top[:, 0]] > (1.0 + 1e-6) * al[np.arange(q), top[:, 1]])   # far beyond any rounding
    assert clear.sum() >= max(1, has.sum() // 2)
    np.testing.assert_array_equal(np.argmax(got["alpha_dense"][:, 0, :], axis=1)[clear], top[clear, 0])
    np.testing.assert_array_equal(scan["best_snp"][clear], top[clear, 0])
    assert got["n_undef"][0] == 1 and scan["n_undef"][0] == 1
    np.testing.assert_array_equal(got["n_undef"], [int(lo[t] <= FU.ZERO_COL < hi[t]) for t in range(q)])
    assert (got["alpha_dense"][:, :, FU.ZERO_COL] == 0).all() and (got["mu_dense"][:, :, FU.ZERO_COL] == 0).all()
    for t in np.nonzero(~has)[0]:
        assert got["n_iter"][t] == 0 and np.isnan(got["sigma2"][t]) and not (got["trait"] == t).any()
    if pattern == "band" and q > 4:
        assert not has[4]


@pytest.mark.parametrize("shape,pattern,L", [((50, 17, 5), "band", 3), ((257, 130, 130), "all", 10), ((130, 1000, 20), "band", 3)])
def test_rows_and_cap(shape, pattern, L):
    """The rows are the dense alpha thresholded at thr_t over the effects with V > 0, as sets; cap = 0 only counts; beyond cap
    n_rows is still the full count."""
    from atlasqtl_amd import cis_susie as CIS
    n, p, q = shape
    lo, hi = FU.windows(pattern, p, q)
    cov, amin = 0.9, 1e-3
    kw = dict(L=L, tol=0.0, max_iter=3, coverage=cov, alpha_min=amin)
    prep = _handle(shape)
    try:
        full = prep.cis_finemap(lo, hi, dense=True, cap=L * p * q, **kw)
        count = prep.cis_finemap(lo, hi, cap=0, **kw)
        short = prep.cis_finemap(lo, hi, cap=full["n_rows"] - 1, **kw)
    finally:
        prep.close()
    thr = CIS.row_threshold(amin, cov, (hi - lo) - full["n_undef"])
    A, M = full["alpha_dense"], full["mu_dense"]
    want = {}
    for t in np.nonzero(hi > lo)[0]:
        for l in np.nonzero(full["V"][t] > 0)[0]:
            for s in range(lo[t], hi[t]):
                if s != FU.ZERO_COL and A[t, l, s] >= thr[t]:
                    want[(s, int(t), int(l))] = (A[t, l, s], M[t, l, s])
    rows = lambda o: {(int(s), int(t), int(l)): (float(a), float(m)) for s, t, l, a, m in zip(o["snp"], o["trait"], o["effect"], o["alpha"], o["mu"])}
    assert (full["V"][hi > lo] == 0).any() and (full["V"][hi > lo] > 0).any()
    assert full["n_rows"] == len(want) > 0 and rows(full) == want
    assert (full["mu2"] >= full["mu"] ** 2).all() and np.isfinite(full["mu2"]).all()
    assert count["n_rows"] == full["n_rows"] and count["snp"].size == 0
    assert short["n_rows"] == full["n_rows"] and short["snp"].size == full["n_rows"] - 1
    assert set(rows(short).items()) <= set(want.items()) and len(rows(short)) == full["n_rows"] - 1


def test_purity_against_numpy():
    shape = (257, 130, 130)
    Xs, _ = _matrices(shape)
    rng = np.random.default_rng(5)
    sets = [[7], [4, 5], [5, 6], [FU.ZERO_COL, 9], list(rng.permutation(130)[:100]), list(range(5, 30)), [129]]
    prep = _handle(shape)
    try:
        mn, mean = prep.set_purity(sets)
        again = prep.set_purity(sets)
    finally:
        prep.close()
    assert np.array_equal(_bits(mn), _bits(again[0])) and np.array_equal(_bits(mean), _bits(again[1]))
    for b, s in enumerate(sets):
        if len(s) == 1:
            assert mn[b] == 1.0 and mean[b] == 1.0             # a set of one has purity 1
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            R = np.abs(np.nan_to_num(np.corrcoef(np.asarray(Xs[:, s], dtype=LD).astype(np.float64).T), nan=0.0))
        pairs = R[np.triu_indices(len(s), 1)]
        assert abs(mn[b] - pairs.min()) <= 1e-12 and abs(mean[b] - pairs.mean()) <= 1e-12, b
    assert mn[1] > 0.8 and mn[3] == 0.0                        # the causal variant and its LD neighbour; a constant column counts as 0


def planted(seed=0):
    """n = 300, p = 200 variants 1000 bp apart on one chromosome, q = 6 genes: gene 0 has two causal variants, 60 and 140, each
    with neighbours on both sides in LD r ~ 0.9; gene 1 has no signal; the others one effect each."""
    n, p, q = 300, 200, 6
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    for c in (60, 140):
        for nb in (c - 1, c + 1):
            X[:, nb] = 0.9 * X[:, c] + np.sqrt(1 - 0.81) * X[:, nb]
    Y = rng.standard_normal((n, q))
    Y[:, 0] += 0.8 * X[:, 60] - 0.7 * X[:, 140]
    for t in range(2, q):
        Y[:, t] += 0.6 * X[:, 20 + 30 * t]
    return dict(X=np.asfortranarray(X), Y=np.asfortranarray(Y), snp_chrom=np.array(["1"] * p, dtype=object), snp_pos=1000 * np.arange(p),
                trait_chrom=["1"] * q, trait_start=[100_000, 100_000, 80_000, 110_000, 140_000, 170_000], window=90_000)


def test_end_to_end():
    import atlasqtl_amd as A
    from atlasqtl_amd import _lib
    c = planted()
    kw = {k: c[k] for k in ("snp_chrom", "snp_pos", "trait_chrom", "trait_start", "window")}
    fm = A.cis_finemap(c["Y"], c["X"], **kw, L=5, dense=True)
    cs = fm["cs"]
    mine = cs["trait"] == 0
    sets = {int(l): set(cs["snp"][mine & (cs["cs"] == l)].tolist()) for l in np.unique(cs["cs"][mine])}
    assert fm["n_cs"][0] == 2 and len(sets) == 2                # two credible sets, each with its causal variant
    assert sorted(60 in s for s in sets.values()) == [False, True] and sorted(140 in s for s in sets.values()) == [False, True]
    assert all(s <= {59, 60, 61} or s <= {139, 140, 141} for s in sets.values())
    assert fm["n_cs"][1] == 0 and not (cs["trait"] == 1).any()  # no signal: none
    assert (fm["n_cs"][2:] >= 1).all() and fm["converged"].all() and (cs["purity_min"] >= 0.5).all()
    assert np.allclose(cs["beta"], cs["alpha"] * fm["mu"][cs["trait"], cs["cs"], cs["snp"]]) and (cs["pip"] >= cs["alpha"] - 1e-15).all()
    assert fm["alpha"].shape == (6, 5, 200) and fm["plan"]["L"] == 5 and fm["elbo"].shape[1] == 6
    pip = {(int(s), int(t)): v for s, t, v in zip(fm["pip"]["snp"], fm["pip"]["trait"], fm["pip"]["pip"])}
    assert all(v <= 1.0 + 1e-15 for v in pip.values()) and pip[(60, 0)] > 0.9 and pip[(140, 0)] > 0.9
    # traits=: only those are fitted
    sub = A.cis_finemap(c["Y"], c["X"], **kw, L=5, traits=[0, 3])
    assert sub["n_cs"].tolist() == [2, 0, 0, fm["n_cs"][3], 0, 0] and np.isnan(sub["sigma2"][[1, 2, 4, 5]]).all()
    Y = c["Y"].copy()
    Y[3, 2] = np.nan
    with pytest.raises(_lib.AtlasqtlHipError, match="aq_prep_cis_finemap"):
        A.cis_finemap(Y, c["X"], **kw)
