"""GPU: LD pruning of the prepared matrix (aq_prep_ld_prune / aq_prep_ld_band, csrc/aq_ld_kernels.h) against the long-double
restatement of tests/ld_util.py run on the handle's own unpruned matrix, at shapes chosen for the kernels' edges: n with a
K tail (50, 333), odd n (8-byte loads) and several K chunks; p below one 16-column tile, off a multiple of 16 and of 64;
windows off a multiple of 16 and 64, of one column, and wider than p; groups whose borders are not tile borders."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

from tests import ld_util as LU

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _unpruned(n, p, form="int8"):
    """(G, Y, Xs of an unpruned handle, bool_cst | bool_coll, the long-double Gram matrix of Xs), computed once per shape."""
    from atlasqtl_amd import prepare as P
    G, Y = LU.ld_case(n, p, 3, seed=1000 * n + p, na=0.1)
    prep, cst, coll, _ = P.prepare_on_device(Y, G if form == "int8" else G.astype(np.float64))
    Xs = prep.X_host()
    prep.close()
    for a in (G, Y, Xs):
        a.setflags(write=False)
    return G, Y, Xs, cst | coll, LU.gram_ld(Xs)


def _to_original(rm0, of, r2, first_removed):
    """The restatement's compact results in the numbering of the columns given."""
    orig = np.where(~first_removed)[0]
    rm_full = np.zeros(first_removed.size, dtype=bool)
    of_full = np.full(first_removed.size, -1)
    r2_full = np.full(first_removed.size, np.nan, dtype=LU.LD)
    rm_full[orig[rm0]] = True
    of_full[orig[rm0]] = orig[of[rm0]]
    r2_full[orig[rm0]] = r2[rm0]
    return rm_full, of_full, r2_full


def _check_prune(prep, gram, first_removed, n, r2, window, group=None, pos=None, window_bp=None):
    """ld_removed and ld_of exactly, ld_r2 to (n + 2) 2^-53, given that no eligible r^2 lies within 1e-9 of the threshold."""
    cg = None if group is None else np.asarray(group)[~first_removed]
    cp = None if pos is None else np.asarray(pos)[~first_removed]
    w = min(window, gram.shape[0])
    rm0, of, rr, margin = LU.greedy(LU.band_ld(None, w, gram=gram), r2, w, cg, cp, window_bp)
    print(f"n={n} p1={gram.shape[0]} r2={r2} window={window}: removed {rm0.sum()}, margin {margin:.3e}")
    assert margin > 1e-9
    rm_ref, of_ref, r2_ref = _to_original(rm0, of, rr, first_removed)
    np.testing.assert_array_equal(prep.ld_removed, rm_ref)
    np.testing.assert_array_equal(prep.ld_of, of_ref)
    assert np.array_equal(np.isnan(prep.ld_r2), ~rm_ref)
    err = np.abs(prep.ld_r2[rm_ref].astype(LU.LD) - r2_ref[rm_ref])
    print(f"   max |ld_r2 error| {float(err.max()) if err.size else 0.0:.3e} (bound {(n + 2) * U:.3e})")
    assert (err <= (n + 2) * U).all()
    assert prep.p == gram.shape[0] - rm0.sum() and prep.shape == (n, prep.p)
    return rm_ref


@pytest.mark.parametrize("n,p,window", [(50, 12, 1), (50, 12, 5), (50, 12, 4096), (50, 100, 17), (333, 100, 16), (333, 100, 64),
                                        (333, 257, 100), (333, 257, 4096), (1000, 257, 5), (1000, 257, 17), (1000, 100, 100),
                                        (5000, 100, 64), (5000, 12, 16)])
def test_band_values(n, p, window):
    """Every entry within (n + 2) 2^-53 of the long-double quotient: the worst case of an n-term fp64 dot product in any
    order with sum |x y| <= n - 1, the division and the rounding of the result.  NaN exactly where j - 1 - b < 0."""
    from atlasqtl_amd import prepare as P
    G, Y, Xs, _, gram = _unpruned(n, p)
    prep, _, _, _ = P.prepare_on_device(Y, G)
    try:
        band = prep.ld_band(window)
    finally:
        prep.close()
    p1 = Xs.shape[1]
    assert band.shape == (p1, window)
    wc = min(window, p1)                                        # beyond p1 columns back there is nothing but NaN
    ref = LU.band_ld(None, wc, gram=gram)
    assert np.isnan(band[:, wc:]).all()
    jj, bb = np.meshgrid(np.arange(p1), np.arange(wc), indexing="ij")
    np.testing.assert_array_equal(np.isnan(band[:, :wc]), jj - 1 - bb < 0)
    ok = jj - 1 - bb >= 0
    err = np.abs(band[:, :wc][ok].astype(LU.LD) - ref[ok])
    print(f"n={n} p1={p1} window={window}: max |error| {float(err.max()):.3e} (bound {(n + 2) * U:.3e})")
    assert (err <= (n + 2) * U).all()


@pytest.mark.parametrize("r2", [0.2, 0.5, 0.8])
@pytest.mark.parametrize("n,p,window", [(50, 12, 5), (333, 100, 17), (1000, 257, 100), (333, 257, 4096), (5000, 100, 64), (50, 100, 1)])
def test_pruning_result(n, p, window, r2):
    from atlasqtl_amd import prepare as P
    G, Y, _, first, gram = _unpruned(n, p)
    prep, cst, coll, _ = P.prepare_on_device(Y, G, ld_prune={"r2": r2, "window": window})
    try:
        np.testing.assert_array_equal(cst | coll, first)        # bool_cst, bool_coll are what they were
        rm = _check_prune(prep, gram, first, n, r2, window)
        assert not (rm & first).any() and not rm[0]
    finally:
        prep.close()


@pytest.mark.parametrize("r2", [0.2, 0.5, 0.8])
@pytest.mark.parametrize("n,p,window", [(333, 100, 16), (1000, 257, 64)])
def test_pruning_with_groups_and_window_bp(n, p, window, r2):
    from atlasqtl_amd import prepare as P
    G, Y, _, first, gram = _unpruned(n, p)
    group = LU.three_groups(p)
    pos = 1000 + np.cumsum(np.random.default_rng(p).integers(1, 400, size=p))
    labels = np.array(["chrX", "chr2", "chr10"])[group]          # any labels; their codes need not be ordered
    for kw, ref_kw in (({"groups": labels}, {"group": group}),
                       ({"positions": pos, "window_bp": 600}, {"pos": pos, "window_bp": 600}),
                       ({"groups": labels, "positions": pos, "window_bp": 600}, {"group": group, "pos": pos, "window_bp": 600})):
        prep, _, _, _ = P.prepare_on_device(Y, G, ld_prune={"r2": r2, "window": window, **kw})
        try:
            rm = _check_prune(prep, gram, first, n, r2, window, **ref_kw)
            if "group" in ref_kw:                                # a tag never sits across a border
                assert (group[prep.ld_of[rm]] == group[rm]).all()
        finally:
            prep.close()


def test_chain_on_the_gpu():
    from atlasqtl_amd import prepare as P
    X, R = LU.chain_abc()
    assert R[0, 1] ** 2 > 0.5 + 1e-9 and R[1, 2] ** 2 > 0.5 + 1e-9 and R[0, 2] ** 2 < 0.5 - 1e-9
    prep, _, _, _ = P.prepare_on_device(np.random.default_rng(0).normal(size=(X.shape[0], 2)), X, ld_prune={"r2": 0.5, "window": 2})
    try:
        assert list(prep.ld_removed) == [False, True, False] and list(prep.ld_of) == [-1, 0, -1] and prep.p == 2
    finally:
        prep.close()


@pytest.mark.parametrize("n,p,window", [(333, 100, 17), (1000, 257, 100)])
def test_kept_columns_keep_their_bits(n, p, window):
    from atlasqtl_amd import prepare as P
    G, Y, Xs, first, _ = _unpruned(n, p)
    a, _, _, _ = P.prepare_on_device(Y, G)
    Ya = a.Y.copy()
    a.close()
    prep, _, _, _ = P.prepare_on_device(Y, G, ld_prune={"r2": 0.5, "window": window})
    try:
        kept = ~prep.ld_removed[~first]
        assert 0 < kept.sum() < kept.size
        Xp = prep.X_host()
        assert Xp.shape == (n, kept.sum())
        assert Xp.tobytes() == np.asfortranarray(Xs[:, kept]).tobytes()
        assert prep.Y.tobytes() == Ya.tobytes()
        # and the band of the pruned matrix is the band of those columns
        band = prep.ld_band(3)
        ref = LU.band_ld(Xp, 3)
        ok = ~np.isnan(ref)
        assert (np.abs(band[ok].astype(LU.LD) - ref[ok]) <= (n + 2) * U).all()
    finally:
        prep.close()


def test_every_input_form_gives_the_restatements_set(tmp_path):
    """fp64, int8, PlinkBed (chromosomes from the .bim as default groups) and covariates: each against the restatement run on
    that handle's own unpruned matrix; the three forms of the same genotypes agree with one another."""
    from atlasqtl_amd import PlinkBed
    from atlasqtl_amd import prepare as P
    from tests import bed_util as BU
    from tests.cov_util import covariates
    n, p, window, r2 = 333, 100, 17, 0.5
    G, Y, _, _, _ = _unpruned(n, p)
    BU.write_fileset(tmp_path / "ld", 2 - G.astype(np.int64), pad_rng=np.random.default_rng(3))      # A1 dosage = G
    group = LU.three_groups(p)
    chrom = np.array(["2", "X", "10"])[group]                    # three chromosomes in blocks, in place of bed_util's cycle
    with open(tmp_path / "ld.bim") as f:
        rows = [ln.split() for ln in f]
    with open(tmp_path / "ld.bim", "w") as f:
        f.writelines("\t".join([c] + r[1:]) + "\n" for c, r in zip(chrom, rows))
    bed = PlinkBed(str(tmp_path / "ld"))
    assert bed.chrom == list(chrom)
    sets = []
    for X, kw, grp in ((G.astype(np.float64), {}, None), (G, {}, None), (bed, {"groups": np.zeros(p, dtype=int)}, None),
                       (bed, {}, group), (G, {"groups": chrom}, group)):
        plain, cst, coll, _ = P.prepare_on_device(Y, X)
        gram = LU.gram_ld(plain.X_host())
        plain.close()
        prep, _, _, _ = P.prepare_on_device(Y, X, ld_prune={"r2": r2, "window": window, **kw})
        try:
            sets.append(_check_prune(prep, gram, cst | coll, n, r2, window, group=grp))
        finally:
            prep.close()
    np.testing.assert_array_equal(sets[0], sets[1])
    np.testing.assert_array_equal(sets[0], sets[2])
    np.testing.assert_array_equal(sets[3], sets[4])
    assert sets[0].sum() > sets[3].sum() > 0                      # across a chromosome border nothing is eligible
    Z = covariates(n, 4, np.random.default_rng(8))
    plain, cst, coll, _ = P.prepare_on_device(Y, G, covariates=Z)
    gram = LU.gram_ld(plain.X_host())
    plain.close()
    prep, _, _, _ = P.prepare_on_device(Y, G, covariates=Z, ld_prune={"r2": r2, "window": window})
    try:
        _check_prune(prep, gram, cst | coll, n, r2, window)
        assert prep.n_cov == 4
    finally:
        prep.close()


def test_whole_run_equals_the_run_on_the_kept_columns():
    import atlasqtl_amd as A
    from atlasqtl_amd import prepare as P
    n, p, q = 333, 100, 6
    G, _, _, first, gram = _unpruned(n, p)
    rng = np.random.default_rng(11)
    X = G.astype(np.float64)
    Y = X[:, [20, 60]] @ rng.normal(size=(2, q)) + rng.normal(size=(n, q))
    ld = {"r2": 0.5, "window": 17}
    a = A.atlasqtl(Y, X, p0=(2, 4), ld_prune=ld, user_seed=3, verbose=0)
    rm0, of, _, margin = LU.greedy(LU.band_ld(None, 17, gram=gram), 0.5, 17)
    assert margin > 1e-9
    rm_ref, of_ref, _ = _to_original(rm0, of, np.zeros(rm0.size, dtype=LU.LD), first)
    names = [f"Cov_x_{j + 1}" for j in range(p)]
    assert a.rmvd_ld_x == {names[j]: names[of_ref[j]] for j in np.where(rm_ref)[0]} and len(a.rmvd_ld_x) > 5
    kept = ~(first | rm_ref)
    assert a.names_x == [nm for nm, k in zip(names, kept) if k]
    assert np.array_equal(np.isnan(a.ld_r2_x), ~rm_ref) and (a.ld_r2_x[rm_ref] > 0.5).all()
    b = A.atlasqtl(Y, X[:, kept], p0=(2, 4), user_seed=3, verbose=0)
    assert "rmvd_ld_x" not in b and b.rmvd_coll_x is None and b.rmvd_cst_x is None
    assert a.it == b.it and a.lb_opt == b.lb_opt and a.converged == b.converged
    np.testing.assert_array_equal(a.gam_vb, b.gam_vb)
    np.testing.assert_array_equal(a.beta_vb, b.beta_vb)
    assert a.gam_vb.shape == (kept.sum(), q)
    # summary() and the sparse output on the pruned result
    out = A.summary(a, file=io.StringIO())
    assert out["rs_thres"].size == kept.sum() and [nm for nm, _ in out["top"]] and set(nm for nm, _ in out["top"]) <= set(a.names_x)
    s = A.atlasqtl(Y, X, p0=(2, 4), ld_prune=ld, user_seed=3, verbose=0, sparse_output={"thres": 0.5, "summary": True})
    sel = np.argwhere(a.gam_vb > 0.5)
    assert s.nb_pairwise == len(sel) > 0 and set(zip(s.assoc["snp"], s.assoc["trait"])) == set(map(tuple, sel))
    assert list(s.assoc["snp_name"]) == [a.names_x[j] for j in s.assoc["snp"]] and s.rmvd_ld_x == a.rmvd_ld_x
    assert A.summary(s, file=io.StringIO())["nb_pairwise"] == out["nb_pairwise"]
    # a list_hyper of the original p is accepted and serves the kept predictors: the run on the kept columns is the same
    hyper = dict(eta=1.0, kappa=1.0, n0=-2.0, nu=0.01, rho=1.0, t02=0.1)
    c = A.atlasqtl(Y, X, p0=(2, 4), list_hyper=A.set_hyper(q, p, **hyper), ld_prune=ld, user_seed=3, verbose=0, maxit=40)
    d = A.atlasqtl(Y, X[:, kept], p0=(2, 4), list_hyper=A.set_hyper(q, int(kept.sum()), **hyper), user_seed=3, verbose=0, maxit=40)
    assert c.gam_vb.shape == (kept.sum(), q) and c.rmvd_ld_x == a.rmvd_ld_x and c.it == d.it
    np.testing.assert_array_equal(c.gam_vb, d.gam_vb)
    with pytest.raises(A.AtlasqtlError, match=r"dimensions \(p\)"):
        A.atlasqtl(Y, X, p0=(2, 4), list_hyper=A.set_hyper(q, int(kept.sum()), **hyper), ld_prune=ld, user_seed=3, verbose=0)


def test_second_prune_is_refused():
    from atlasqtl_amd import _lib
    from atlasqtl_amd import prepare as P
    G, Y, _, _, _ = _unpruned(50, 12)
    L = _lib.lib()
    prep, _, _, _ = P.prepare_on_device(Y, G)
    try:
        assert L.aq_prep_ld_info(prep.handle, None, None, None, None) == 1            # not pruned yet
        assert "has not run" in L.aq_last_error().decode()
        ld = _lib.AqPrepLd()
        ld.window, ld.r2, ld.group, ld.pos, ld.window_bp = 5, 0.5, None, None, 0
        assert L.aq_prep_ld_prune(prep.handle, C.byref(ld)) == 0
        pk = C.c_int32(-1)
        assert L.aq_prep_ld_info(prep.handle, C.byref(pk), None, None, None) == 0
        before = pk.value
        assert L.aq_prep_ld_prune(prep.handle, C.byref(ld)) == 1
        assert "pruned already" in L.aq_last_error().decode()
        assert L.aq_prep_ld_info(prep.handle, C.byref(pk), None, None, None) == 0 and pk.value == before
    finally:
        prep.close()
