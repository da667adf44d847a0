"""GPU: the genetic relationship matrix of a prepared handle (aq_prep_grm, csrc/aq_grm_kernels.h) and the genotype PCs built
on it, against the long-double restatement of tests/grm_util.py run on the handle's own matrix, at shapes chosen for the
kernels' edges: n below one tile (20, 50), off a multiple of 16 (50, 130, 333), odd (257, 333: 8-byte loads), over several
tiles of 128 with a last tile of one sample (257) and of 64 (130); p below one MFMA step (3), off a multiple of 4 and of the
16-predictor chunk (257), and over many chunks (1000, 5000).  Every shape runs with one workgroup per tile and with the
predictors split over 2 and 5 (AQ_GRM_SPLITS), which at small p leaves splits with no predictor at all."""
import functools

import numpy as np
import pytest

from tests import grm_util as GU

pytestmark = pytest.mark.gpu

SHAPES = [(20, 3), (50, 12), (50, 100), (333, 257), (130, 1000), (1000, 257), (257, 5000)]
Y0 = functools.lru_cache(maxsize=None)(lambda n: np.zeros((n, 1), order="F"))


@functools.lru_cache(maxsize=None)
def _case(n, p, form="int8"):
    """(X as given, Xs of its handle, the long-double GRM of Xs, the matrix of elementwise bounds), once per shape."""
    from atlasqtl_amd import prepare as P
    G = GU.pop_case(n, p, 1000 * n + p)
    X = G if form == "int8" else G.astype(np.float64)
    prep = P.prepare_on_device(Y0(n), X)[0]
    Xs = prep.X_host()
    prep.close()
    K, B = GU.grm_ld(Xs), GU.grm_bound(Xs)
    for a in (X, Xs, K, B):
        a.setflags(write=False)
    return X, Xs, K, B


def _seq_sum(v):
    return float(np.cumsum(np.asarray(v, dtype=np.float64))[-1])     # cumsum adds in index order, one rounding per entry


def _trace_slack(n, diag_bounds):
    """What |trace K - (n - 1)| may be: the diagonal entries' own bounds; the columns' sums of squares, n - 1 to within
    2 (n + 2) 2^-53 relative (an n-term sum, a square root and a division behind every entry, squared); and the n - 1
    additions of the trace itself."""
    return float(diag_bounds) + 2 * (n + 2) * GU.U * (n - 1) + (n - 1) * GU.U * (n - 1)


def _check_grm(prep, K_ref, B, label):
    """The elementwise bound and the four properties on an open handle; returns K."""
    n = prep.n
    K, tr = prep.grm(return_trace=True)
    K2, tr2 = prep.grm(return_trace=True)
    assert K.shape == (n, n) and K.flags.f_contiguous
    assert np.isfinite(K).all() and (B > 0).all()
    err = np.abs(K.astype(GU.LD) - K_ref)
    ratio = float(np.max(err / B))
    rows = np.abs(K.astype(GU.LD).sum(axis=1))
    row_ratio = float(np.max(rows / B.sum(axis=1)))
    print(f"{label}: p1={prep.p} worst |error| / bound {ratio:.3f}, worst |row sum| / bound {row_ratio:.3f}")
    assert (err <= B).all()
    np.testing.assert_array_equal(K, K.T)                       # exactly symmetric
    assert K.tobytes() == K2.tobytes() and tr == tr2            # two calls, the same bits
    assert tr == _seq_sum(np.diag(K))                           # the diagonal as returned, added in index order
    assert (rows <= B.sum(axis=1)).all()                        # K 1 = 0: every column of Xs is centred
    return K


@pytest.mark.parametrize("splits", [None, 2, 5])
@pytest.mark.parametrize("n,p", SHAPES)
def test_grm_of_int8_dosages(n, p, splits, monkeypatch):
    """Every entry within (p1 + 2) 2^-53 (sum_j |Xs[a, j] Xs[b, j]|) / p1 of the long-double value: the worst case of a
    p1-term fp64 dot product in any order, plus the division and the final rounding, so it holds for any tiling and any S."""
    from atlasqtl_amd import prepare as P
    G, Xs, K_ref, B = _case(n, p)
    if splits is None:
        monkeypatch.delenv("AQ_GRM_SPLITS", raising=False)
    else:
        monkeypatch.setenv("AQ_GRM_SPLITS", str(splits))
    prep = P.prepare_on_device(Y0(n), G)[0]
    try:
        assert prep.p == Xs.shape[1]
        _check_grm(prep, K_ref, B, f"n={n} p={p} S={splits or 'plan'}")
    finally:
        prep.close()


@pytest.mark.parametrize("splits", [None, 2, 5])
@pytest.mark.parametrize("n,p", [(50, 100), (333, 257)])
def test_grm_of_float64_input(n, p, splits, monkeypatch):
    import atlasqtl_amd as A
    from atlasqtl_amd import prepare as P
    X, Xs, K_ref, B = _case(n, p, "float64")
    if splits is None:
        monkeypatch.delenv("AQ_GRM_SPLITS", raising=False)
    else:
        monkeypatch.setenv("AQ_GRM_SPLITS", str(splits))
    prep = P.prepare_on_device(Y0(n), X)[0]
    try:
        K = _check_grm(prep, K_ref, B, f"float64 n={n} p={p} S={splits or 'plan'}")
    finally:
        prep.close()
    np.testing.assert_array_equal(A.genotype_grm(X), K)          # the public function is this path


def test_forced_splits_out_of_range_are_refused(monkeypatch):
    from atlasqtl_amd import _lib
    from atlasqtl_amd import prepare as P
    G, _, _, _ = _case(50, 12)
    prep = P.prepare_on_device(Y0(50), G)[0]
    try:
        for bad in ("0", "65", "-3"):
            monkeypatch.setenv("AQ_GRM_SPLITS", bad)
            with pytest.raises(_lib.AtlasqtlHipError, match="aq_prep_grm: AQ_GRM_SPLITS"):
                prep.grm()
    finally:
        prep.close()


@pytest.mark.parametrize("n,p", [(333, 257), (130, 1000)])
def test_other_handle_states(n, p):
    """With covariates and after ld_prune, K is that of the handle's current matrix, under the same bound."""
    import atlasqtl_amd as A
    from atlasqtl_amd import prepare as P
    from tests.cov_util import covariates
    G, Xs0, _, _ = _case(n, p)
    Z = covariates(n, 4, np.random.default_rng(n + p))
    ld = {"r2": 0.1, "window": 50}                               # removes 16 of 257 and 151 of 1000 columns of the plain matrix
    for kw in ({"covariates": Z}, {"ld_prune": ld}, {"covariates": Z, "ld_prune": ld}):
        prep = P.prepare_on_device(Y0(n), G, **kw)[0]
        try:
            Xs = prep.X_host()
            if "ld_prune" in kw:
                assert 1 < prep.p < Xs0.shape[1]                 # something was pruned
            if "covariates" in kw:
                assert prep.n_cov == 4 and not np.array_equal(Xs[:, 0], Xs0[:, 0])
            K = _check_grm(prep, GU.grm_ld(Xs), GU.grm_bound(Xs), f"n={n} p={p} {sorted(kw)}")
        finally:
            prep.close()
        np.testing.assert_array_equal(A.genotype_grm(G, **kw), K)


def test_limit_on_a_handle():
    """n = 10 241 is AQ_ERR_UNSUPPORTED and names the entry.  n = 10 240, the plan's largest grid (3240 tiles) and the largest
    offsets into K, is served: two predictors keep it to the copy of K, checked on rows at the tile borders."""
    from atlasqtl_amd import _lib
    from atlasqtl_amd import prepare as P
    for n in (10241, 10240):
        G = np.zeros((n, 2), dtype=np.int8)
        G[::2, 0] = 1
        G[::3, 1] = 2
        prep = P.prepare_on_device(Y0(n), G)[0]
        try:
            if n > 10240:
                with pytest.raises(_lib.AtlasqtlHipError, match=r"\[3\] aq_prep_grm: n = 10241 exceeds 10240"):
                    prep.grm()
                continue
            K, tr = prep.grm(return_trace=True)
            Xs = prep.X_host()
        finally:
            prep.close()
        rows = np.array([0, 1, 127, 128, 5000, 10111, 10112, 10239])
        Xl = Xs.astype(GU.LD)
        ref = (Xl[rows] @ Xl.T) / GU.LD(2)
        bound = GU.LD(4 * GU.U) * (np.abs(Xl[rows]) @ np.abs(Xl.T)) / GU.LD(2)
        assert (np.abs(K[rows].astype(GU.LD) - ref) <= bound).all()
        np.testing.assert_array_equal(K[rows], K[:, rows].T)
        d = np.diag(K)
        assert tr == float(np.cumsum(d)[-1])                     # cumsum adds in index order
        assert abs(tr - (n - 1)) <= _trace_slack(n, GU.LD(4 * GU.U) * (Xl * Xl).sum() / GU.LD(2))


@pytest.mark.parametrize("n,p", [s for s in SHAPES if s[0] >= 50])
def test_genotype_pcs(n, p):
    """Davis-Kahan with the GRM's error plus LAPACK's backward error as the perturbation: after sign alignment
    ||v - v_ref||_2 <= (||B||_F + n 2^-52 lambda_1) / gap_i, gap_i the distance of the reference's lambda_i to its nearest other
    eigenvalue; the eigenvalues within ||B||_F + n 2^-52 lambda_1.  Condition: gap_i >= 0.1 lambda_1 for both PCs (on pop_case
    with these seeds it is 0.12 ... 0.45, and the right-hand side is then <= 2e-11)."""
    import atlasqtl_amd as A
    G, Xs, K_ref, B = _case(n, p)
    lam_ref, V_ref, gap, lam1 = GU.top_eig(K_ref, 2)
    print(f"n={n} p={p}: gap / lambda_1 = {gap / lam1}")
    assert (gap >= 0.1 * lam1).all()
    out = A.genotype_pcs(G, 2)
    pert = float(np.sqrt((B.astype(np.float64) ** 2).sum())) + n * 2.0 ** -52 * lam1
    V = out["pcs"]
    assert V.shape == (n, 2) and out["eigenvalues"].shape == (2,) and out["p_used"] == Xs.shape[1]
    np.testing.assert_array_equal(V, GU.pc_sign(V))              # the sign rule
    np.testing.assert_allclose(np.linalg.norm(V, axis=0), 1.0, rtol=1e-14)
    assert np.abs(V.sum(axis=0)).max() <= 1e-9                   # orthogonal to the intercept
    for i in range(2):
        v = V[:, i] if V[:, i] @ V_ref[:, i] >= 0 else -V[:, i]
        dist = float(np.linalg.norm(v - V_ref[:, i]))
        print(f"   PC{i + 1}: ||v - v_ref|| = {dist:.3e} (bound {pert / gap[i]:.3e}), |lambda - ref| = "
              f"{abs(out['eigenvalues'][i] - lam_ref[i]):.3e} (bound {pert:.3e})")
        assert pert / gap[i] <= 2e-11
        assert dist <= pert / gap[i]
        assert abs(out["eigenvalues"][i] - lam_ref[i]) <= pert
    assert out["eigenvalues"][0] > out["eigenvalues"][1] > 0
    # var_explained is eigenvalue / trace K, the trace being the diagonal of the GRM added in index order
    K = A.genotype_grm(G)
    tr = _seq_sum(np.diag(K))
    np.testing.assert_array_equal(out["var_explained"], out["eigenvalues"] / tr)
    assert abs(tr - (n - 1)) <= _trace_slack(n, np.trace(B))
    again = A.genotype_pcs(G, 2)
    assert all(np.array_equal(out[k], again[k]) for k in ("pcs", "eigenvalues", "var_explained"))


# ---- end to end ----
@functools.lru_cache(maxsize=None)
def _e2e():
    n, p, q, d = 130, 300, 6, 3
    from tests.cov_util import covariates
    G = GU.pop_case(n, p, 1000 * n + p)
    rng = np.random.default_rng(17)
    Z = covariates(n, d, rng)
    Y = G[:, [20, 150]].astype(np.float64) @ rng.normal(size=(2, q)) + Z @ rng.normal(size=(d, q)) * 0.1 + rng.normal(size=(n, q))
    Y[rng.random((n, q)) < 0.1] = np.nan
    return G, Y, Z


def _same_fit(a, b):
    np.testing.assert_array_equal(a.gam_vb, b.gam_vb)
    np.testing.assert_array_equal(a.beta_vb, b.beta_vb)
    assert a.it == b.it and a.lb_opt == b.lb_opt and a.names_x == b.names_x


def test_atlasqtl_with_genotype_pcs_is_the_run_with_them_as_covariates(tmp_path):
    """The same code path on the same bits: atlasqtl(genotype_pcs=2) against the PCs of genotype_pcs() appended by hand, for
    int8 dosages and through a PlinkBed."""
    import atlasqtl_amd as A
    from tests import bed_util as BU
    G, Y, Z = _e2e()
    n, d = Z.shape
    BU.write_fileset(tmp_path / "pcs", 2 - G.astype(np.int64), pad_rng=np.random.default_rng(3))      # A1 dosage = G
    kw = dict(p0=(2, 4), user_seed=3, verbose=0, maxit=60)
    for X in (G, A.PlinkBed(str(tmp_path / "pcs"))):
        pcs = A.genotype_pcs(X, 2)
        assert pcs["pcs"].shape == (n, 2)
        a = A.atlasqtl(Y, X, covariates=Z, genotype_pcs=2, **kw)
        b = A.atlasqtl(Y, X, covariates=np.hstack([Z, pcs["pcs"]]), **kw)
        _same_fit(a, b)
        assert a.n_covariates == d + 2 and b.n_covariates == d + 2
        np.testing.assert_array_equal(a.genotype_pcs, pcs["pcs"])
        np.testing.assert_array_equal(a.pc_eigenvalues, pcs["eigenvalues"])
        np.testing.assert_array_equal(a.pc_var_explained, pcs["var_explained"])
        assert "genotype_pcs" not in b and "pc_eigenvalues" not in b
        # the PCs matter: without them the fit is another one
        c = A.atlasqtl(Y, X, covariates=Z, **kw)
        assert c.n_covariates == d and not np.array_equal(a.gam_vb, c.gam_vb)
    # without user covariates the PCs are the covariates
    pcs = A.genotype_pcs(G, 2)
    a = A.atlasqtl(Y, G, genotype_pcs={"k": 2}, **kw)
    b = A.atlasqtl(Y, G, covariates=pcs["pcs"], **kw)
    _same_fit(a, b)
    assert a.n_covariates == 2


def test_inner_ld_prune_thins_only_the_matrix_of_the_pcs():
    import atlasqtl_amd as A
    G, Y, Z = _e2e()
    d = Z.shape[1]
    kw = dict(p0=(2, 4), user_seed=3, verbose=0, maxit=60)
    plain = A.genotype_pcs(G, 2)
    # r2 = 0.5 removes none of these unlinked variants (their largest r^2 is 0.23); r2 = 0.1 removes 51 of the 300
    for ld in ({"r2": 0.5, "window": 50}, {"r2": 0.1, "window": 50}):
        pcs = A.genotype_pcs(G, 2, ld_prune=ld)
        if ld["r2"] < 0.5:
            assert pcs["p_used"] < plain["p_used"] and not np.array_equal(pcs["pcs"], plain["pcs"])
        a = A.atlasqtl(Y, G, covariates=Z, genotype_pcs={"k": 2, "ld_prune": ld}, **kw)
        b = A.atlasqtl(Y, G, covariates=np.hstack([Z, pcs["pcs"]]), **kw)
        _same_fit(a, b)
        np.testing.assert_array_equal(a.genotype_pcs, pcs["pcs"])
        assert a.n_covariates == d + 2
        # the fit's own predictor set is unpruned: nothing was removed for LD, every non-redundant predictor is there
        assert "rmvd_ld_x" not in a and len(a.names_x) == plain["p_used"] == a.gam_vb.shape[0]
    ld = {"r2": 0.1, "window": 50}
    # and the outer ld_prune= still governs the fit alone
    c = A.atlasqtl(Y, G, covariates=Z, genotype_pcs=2, ld_prune=ld, **kw)
    np.testing.assert_array_equal(c.genotype_pcs, plain["pcs"])
    assert c.rmvd_ld_x and len(c.names_x) < plain["p_used"]
