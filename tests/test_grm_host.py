"""Host: the genetic relationship matrix and the genotype PCs (aq_prep_grm, genotype_pcs(), atlasqtl(genotype_pcs=)) as far
as they need no device -- the launch plan of aq_grm_plan_query, the argument errors of aq_prep_grm, every host check of the
genotype_pcs option, the sign rule, and the restatement of tests/grm_util.py on a case worked out by hand."""
import ctypes as C

import numpy as np
import pytest

from atlasqtl_amd import _lib
from tests import grm_util as GU

GB = 1 << 30


def _plan(hiplib, n, p1, ncu=256, free=200 * GB):
    pl = _lib.AqGrmPlan()
    rc = hiplib.aq_grm_plan_query(n, p1, ncu, free, C.byref(pl))
    return rc, pl


def _tile_rc(t):
    """t = ti (ti + 1) / 2 + tj, ti >= tj: the numbering include/atlasqtl_hip.h gives."""
    ti = 0
    while (ti + 1) * (ti + 2) // 2 <= t:
        ti += 1
    return ti, t - ti * (ti + 1) // 2


SHAPES = [(2, 1), (20, 3), (50, 12), (64, 100), (65, 100), (130, 1000), (256, 5000), (257, 5000), (333, 257), (1000, 257),
          (1000, 50000), (4999, 20000), (10240, 20000), (10240, 1)]


@pytest.mark.parametrize("n,p1", SHAPES)
@pytest.mark.parametrize("ncu", [1, 64, 256, 304])
def test_plan_covers_one_triangle_exactly_once(hiplib, n, p1, ncu):
    rc, pl = _plan(hiplib, n, p1, ncu)
    assert rc == 0, hiplib.aq_last_error()
    T, nt = pl.tile, pl.tiles_per_edge
    assert T in (64, 128) and nt == -(-n // T) and pl.n_tiles == nt * (nt + 1) // 2
    # the grid is n_tiles x splits workgroups; workgroup (t, s) owns tile _tile_rc(t) and the chunks of split s
    tiles = [_tile_rc(t) for t in range(pl.n_tiles)]
    assert len(set(tiles)) == pl.n_tiles and all(0 <= tj <= ti < nt for ti, tj in tiles)
    assert set(tiles) == {(i, j) for i in range(nt) for j in range(i + 1)}
    # every sample pair lies in a tile of the triangle or in the mirror of one
    assert (nt - 1) * T < n <= nt * T
    # the splits cover every predictor exactly once
    chunks = -(-p1 // pl.chunk)
    assert pl.splits >= 1 and pl.chunks_per_split == -(-chunks // pl.splits)
    assert pl.splits * pl.chunks_per_split * pl.chunk >= p1
    # S = 1 when the tiles alone give two workgroups per CU; otherwise no more workgroups than that needs
    if pl.n_tiles >= 2 * ncu:
        assert pl.splits == 1
    else:
        assert (pl.splits - 1) * pl.n_tiles < 2 * ncu
    assert pl.scratch_bytes == pl.splits * pl.n_tiles * T * T * 8 and pl.k_bytes == n * n * 8
    # the same inputs, the same answer
    rc2, pl2 = _plan(hiplib, n, p1, ncu)
    assert rc2 == 0 and bytes(pl) == bytes(pl2)


def test_plan_fills_the_device_at_the_bench_shape(hiplib):
    rc, pl = _plan(hiplib, 1000, 50000, 256)
    assert rc == 0 and pl.tile == 128 and pl.n_tiles == 36 and pl.splits == 15      # ceil(512 / 36)
    rc, pl = _plan(hiplib, 10240, 20000, 256)
    assert rc == 0 and pl.tile == 128 and pl.n_tiles == 3240 and pl.splits == 1
    rc, pl = _plan(hiplib, 1000, 257, 256)                                          # 17 chunks: no split below 8 chunks
    assert rc == 0 and pl.splits == 2
    rc, pl = _plan(hiplib, 1000, 100, 256)
    assert rc == 0 and pl.splits == 1


@pytest.mark.parametrize("n,p1", [(1000, 50000), (333, 5000), (10240, 20000), (130, 100000)])
def test_plan_scratch_stays_within_the_free_memory(hiplib, n, p1):
    rc, full = _plan(hiplib, n, p1)
    assert rc == 0
    one_split = full.scratch_bytes // full.splits
    for free in (full.k_bytes + full.scratch_bytes, full.k_bytes + max(full.scratch_bytes - 1, one_split), full.k_bytes + one_split + 5,
                 full.k_bytes + one_split):
        rc, pl = _plan(hiplib, n, p1, free=free)
        assert rc == 0 and pl.splits >= 1 and pl.scratch_bytes <= free and pl.k_bytes + pl.scratch_bytes <= free
    rc, pl = _plan(hiplib, n, p1, free=full.k_bytes + full.scratch_bytes)
    assert pl.splits == full.splits
    rc, pl = _plan(hiplib, n, p1, free=full.k_bytes + one_split)
    assert pl.splits == 1
    rc, _ = _plan(hiplib, n, p1, free=full.k_bytes + one_split - 1)                  # not even one split fits
    assert rc == 2 and "aq_grm_plan_query" in hiplib.aq_last_error().decode() and "free" in hiplib.aq_last_error().decode()
    rc, _ = _plan(hiplib, n, p1, free=0)
    assert rc == 2


def test_plan_argument_errors(hiplib):
    assert hiplib.aq_grm_plan_query(100, 10, 256, GB, None) == 1
    assert "aq_grm_plan_query" in hiplib.aq_last_error().decode() and "NULL" in hiplib.aq_last_error().decode()
    for n, p1, ncu, free in ((1, 10, 256, GB), (100, 0, 256, GB), (100, 10, 0, GB), (100, 10, 256, -1)):
        rc, _ = _plan(hiplib, n, p1, ncu, free)
        assert rc == 1 and "aq_grm_plan_query" in hiplib.aq_last_error().decode()


def test_argument_errors_of_aq_prep_grm_come_before_the_device(hiplib):
    """AQ_ERR_ARG (1) for a NULL handle or output, naming aq_prep_grm.  AQ_ERR_UNSUPPORTED (3) for n > 10240: a handle exists
    only where a device does, so without one the limit is reached through the plan, which names its own entry; aq_prep_grm
    runs the same check of n (aq_grm_check_n) before its first device call, and tests/test_gpu_grm.py meets it on a handle."""
    K = np.zeros(4)
    assert hiplib.aq_prep_grm(None, _lib.as_dp(K), None) == 1
    msg = hiplib.aq_last_error().decode()
    assert "aq_prep_grm" in msg and "NULL handle" in msg
    assert hiplib.aq_prep_grm(None, None, None) == 1
    assert "aq_prep_grm" in hiplib.aq_last_error().decode()
    ms = C.c_double(0.0)
    assert hiplib.aq_prep_grm_time(None, 1, C.byref(ms), None) == 1
    assert "aq_prep_grm_time" in hiplib.aq_last_error().decode()
    for n in (10241, 20480):
        rc, _ = _plan(hiplib, n, 100)
        msg = hiplib.aq_last_error().decode()
        assert rc == 3 and msg.startswith("aq_grm_plan_query: n = ") and str(n) in msg and "10240" in msg
    assert _plan(hiplib, 10240, 100)[0] == 0


def test_plan_struct_and_binding_agree():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "atlasqtl_hip.h")).read()
    body = re.search(r"typedef struct aq_grm_plan \{(.*?)\} aq_grm_plan;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    fields = [(d.split()[1], ctype[d.split()[0]]) for d in body.split(";") if d.strip()]
    assert fields == list(_lib.AqGrmPlan._fields_)


# ---- the genotype_pcs option ----
def test_option_forms():
    from atlasqtl_amd.prepare import genotype_pcs_options
    assert genotype_pcs_options(3, 100) == {"k": 3, "ld_prune": None}
    assert genotype_pcs_options(np.int64(10), 100, d=4) == {"k": 10, "ld_prune": None}
    assert genotype_pcs_options({"k": 2}, 100) == {"k": 2, "ld_prune": None}
    o = genotype_pcs_options({"k": 2, "ld_prune": {"r2": 0.5, "window": 50}}, 100)
    assert o == {"k": 2, "ld_prune": {"r2": 0.5, "window": 50}}
    assert genotype_pcs_options(96, 5000)["k"] == 96 and genotype_pcs_options(90, 5000, d=6)["k"] == 90
    assert genotype_pcs_options(18, 20)["k"] == 18 and genotype_pcs_options(1, 3)["k"] == 1
    assert genotype_pcs_options(1, 10240)["k"] == 1


@pytest.mark.parametrize("bad,n,d,match", [
    (0, 100, 0, r"k must lie in \[1, 96\]"), (-1, 100, 0, "k must lie"), (97, 5000, 0, r"k must lie in \[1, 96\]"),
    (91, 5000, 6, r"k must lie in \[1, 90\]"), (19, 20, 0, r"k must lie in \[1, 18\]"), (1, 2, 0, "k must lie"),
    (1, 5000, 96, "k must lie"), (2.0, 100, 0, "genotype_pcs must be"), (2.5, 100, 0, "genotype_pcs must be"),
    (True, 100, 0, "genotype_pcs must be"), ("2", 100, 0, "genotype_pcs must be"), ([2], 100, 0, "genotype_pcs must be"),
    ({"k": 2.0}, 100, 0, "k must be a whole number"), ({"k": None}, 100, 0, "k must be a whole number"),
    ({"k": True}, 100, 0, "k must be a whole number"), ({}, 100, 0, "genotype_pcs must be"),
    ({"ld_prune": {}}, 100, 0, "genotype_pcs must be"), ({"k": 2, "r2": 0.5}, 100, 0, "genotype_pcs must be"),
    ({"k": 2, "ld": None}, 100, 0, "genotype_pcs must be"), ({"k": 2, "ld_prune": {"r2": 2}}, 100, 0, "ld_prune: r2 must be"),
    ({"k": 2, "ld_prune": {"windows": 5}}, 100, 0, "ld_prune must be"), ({"k": 2, "ld_prune": 0.5}, 100, 0, "ld_prune must be"),
    (2, 10241, 0, "at most 10240"), ({"k": 2}, 20000, 0, "at most 10240"),
])
def test_every_rejection_of_the_option(bad, n, d, match):
    from atlasqtl_amd.prepare import AtlasqtlError, genotype_pcs_options
    with pytest.raises(AtlasqtlError, match=match) as e:
        genotype_pcs_options(bad, n, d)
    assert "genotype_pcs" in str(e.value)


def test_python_validates_before_the_device():
    """Everything that can be known on the host is refused there: no device is visible when the non-GPU tests run, so an
    AtlasqtlHipError ("no HIP device") would show a check that came too late."""
    import atlasqtl_amd as A
    from atlasqtl_amd.prepare import AtlasqtlError
    rng = np.random.default_rng(0)
    Y, X, Z = rng.normal(size=(40, 2)), rng.normal(size=(40, 9)), rng.normal(size=(40, 3))
    kw = dict(p0=(2, 4), verbose=0)
    with pytest.raises(AtlasqtlError, match=r"k must lie in \[1, 38\]"):
        A.atlasqtl(Y, X, genotype_pcs=39, **kw)
    with pytest.raises(AtlasqtlError, match=r"k must lie in \[1, 38\]"):
        A.atlasqtl(Y, X.astype(np.int8), genotype_pcs={"k": 0}, covariates=Z, **kw)
    with pytest.raises(AtlasqtlError, match="genotype_pcs must be"):
        A.atlasqtl(Y, X, genotype_pcs={"k": 2, "window": 5}, **kw)
    with pytest.raises(AtlasqtlError, match="window must be"):
        A.atlasqtl(Y, X, genotype_pcs={"k": 2, "ld_prune": {"window": 5000}}, **kw)
    with pytest.raises(AtlasqtlError, match=r"groups must hold one entry per predictor given \(9\)"):
        A.atlasqtl(Y, X, genotype_pcs={"k": 2, "ld_prune": {"groups": np.zeros(8, dtype=int)}}, **kw)
    with pytest.raises(AtlasqtlError, match="window_bp needs positions"):
        A.atlasqtl(Y, X, genotype_pcs={"k": 2, "ld_prune": {"window_bp": 100}}, **kw)
    with pytest.raises(AtlasqtlError, match="same number of samples"):
        A.atlasqtl(Y[:30], X, genotype_pcs=2, **kw)
    with pytest.raises(AtlasqtlError, match="covariates and Y must have the same number of samples"):
        A.atlasqtl(Y, X, genotype_pcs=2, covariates=Z[:30], **kw)
    with pytest.raises(AtlasqtlError, match="covariates must be"):
        A.atlasqtl(Y, X, genotype_pcs=2, covariates=np.full((40, 2), np.nan), **kw)
    with pytest.raises(AtlasqtlError, match=r"k must lie in \[1, 1\]"):               # 96 - 95 covariates leave room for one
        A.atlasqtl(rng.normal(size=(200, 2)), rng.normal(size=(200, 9)), genotype_pcs=2, covariates=rng.normal(size=(200, 95)), **kw)
    big = np.zeros((10241, 1), dtype=np.int8)
    with pytest.raises(AtlasqtlError, match="at most 10240"):
        A.atlasqtl(np.zeros((10241, 1)), big, genotype_pcs=1, **kw)
    with pytest.raises(AtlasqtlError, match="at most 10240"):
        A.genotype_pcs(big, 1)
    with pytest.raises(AtlasqtlError, match="at most 10240"):
        A.genotype_grm(big)
    with pytest.raises(AtlasqtlError, match=r"k must lie in \[1, 38\]"):
        A.genotype_pcs(X, 39)
    with pytest.raises(AtlasqtlError, match="k must be a whole number"):
        A.genotype_pcs(X, 2.0)
    with pytest.raises(AtlasqtlError, match=r"k must lie in \[1, 35\] = \[1, n - 2 - d\]"):       # the residuals on 3 covariates
        A.genotype_pcs(X, 36, covariates=Z)
    with pytest.raises(AtlasqtlError, match="covariates and Y must have the same number of samples"):
        A.genotype_pcs(X, 2, covariates=Z[:30])
    with pytest.raises(AtlasqtlError, match="r2 must be"):
        A.genotype_pcs(X, 2, ld_prune={"r2": 0})
    with pytest.raises(AtlasqtlError, match="X must be"):
        A.genotype_grm(np.zeros(5))


def test_without_the_option_nothing_is_asked_of_it():
    """genotype_pcs=None: the call reaches the device path as before (and, with no device here, fails there loudly)."""
    import atlasqtl_amd as A
    if _lib.lib().aq_device_count() > 0:
        pytest.skip("a HIP device is visible here")
    rng = np.random.default_rng(1)
    with pytest.raises(_lib.AtlasqtlHipError, match="no HIP device"):
        A.atlasqtl(rng.normal(size=(30, 2)), rng.normal(size=(30, 5)), p0=(2, 4), verbose=0, genotype_pcs=None)
    with pytest.raises(_lib.AtlasqtlHipError, match="no HIP device"):
        A.atlasqtl(rng.normal(size=(30, 2)), rng.normal(size=(30, 5)), p0=(2, 4), verbose=0, genotype_pcs=2)


# ---- the sign rule and the eigenpairs ----
def test_sign_rule():
    from atlasqtl_amd.prepare import pc_sign_
    V = np.array([[0.1, -0.5, 0.5, -0.0],
                  [-0.9, 0.5, -0.5, -1.0],
                  [0.3, -0.5, 0.5, 0.0],
                  [0.9, 0.5, -0.5, 1.0]])
    got = pc_sign_(V)
    # column 0: |-0.9| = |0.9|, the first decides: flipped.  1: all equal, the first (-0.5) decides: flipped.  2: kept.
    # 3: -1.0 comes before 1.0: flipped
    want = np.stack([-V[:, 0], -V[:, 1], V[:, 2], -V[:, 3]], axis=1)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, GU.pc_sign(V))
    assert got[1, 0] == 0.9 and got[0, 1] == 0.5 and got[1, 3] == 1.0
    np.testing.assert_array_equal(pc_sign_(got), got)             # idempotent
    np.testing.assert_array_equal(pc_sign_(-got), got)            # either sign of an eigenvector gives the same bits
    assert V[1, 0] == -0.9                                        # the argument is not changed
    rng = np.random.default_rng(5)
    W = rng.normal(size=(37, 6))
    np.testing.assert_array_equal(pc_sign_(W), GU.pc_sign(W))
    assert (np.max(pc_sign_(W), axis=0) == np.max(np.abs(W), axis=0)).all()


def test_pcs_of_a_matrix_with_known_eigenpairs():
    """K = 5 u u' + 2 v v' + 0.5 w w' with orthonormal u, v, w: the PCs are u and v, signed by the rule, in that order."""
    from atlasqtl_amd.prepare import pcs_from_grm_
    Q = np.linalg.qr(np.random.default_rng(4).normal(size=(6, 6)))[0]
    u, v, w = Q[:, 0], Q[:, 1], Q[:, 2]
    K = 5 * np.outer(u, u) + 2 * np.outer(v, v) + 0.5 * np.outer(w, w)
    out = pcs_from_grm_(K, 2)
    np.testing.assert_allclose(out["eigenvalues"], [5.0, 2.0], rtol=1e-14)
    np.testing.assert_allclose(out["var_explained"], np.array([5.0, 2.0]) / np.trace(K), rtol=1e-14)
    want = GU.pc_sign(np.stack([u, v], axis=1))
    assert (want[np.argmax(np.abs(want), axis=0), [0, 1]] > 0).all()
    np.testing.assert_allclose(out["pcs"], want, atol=1e-14)
    np.testing.assert_allclose(np.linalg.norm(out["pcs"], axis=0), 1.0, rtol=1e-14)
    assert pcs_from_grm_(K, 2, trace=15.0)["var_explained"][0] == pytest.approx(1 / 3)
    lam, vec, gap, lam1 = GU.top_eig(K.astype(GU.LD), 2)
    np.testing.assert_allclose(lam, [5.0, 2.0], rtol=1e-14)
    np.testing.assert_allclose(gap, [3.0, 1.5], rtol=1e-13)
    assert lam1 == pytest.approx(5.0) and np.allclose(vec, out["pcs"], atol=1e-14)


def test_restatement_on_a_hand_made_case():
    Xs = np.array([[1.0, -2.0, 0.5], [-1.0, 0.0, 0.5], [0.0, 2.0, -1.0]])
    K = GU.grm_ld(Xs)
    assert K.dtype == GU.LD and float(K[0, 0]) == pytest.approx(5.25 / 3) and float(K[0, 2]) == pytest.approx(-4.5 / 3)
    assert float(K[1, 2]) == pytest.approx(-0.5 / 3) and (K == K.T).all()
    B = GU.grm_bound(Xs)
    assert float(B[0, 2]) == pytest.approx(5 * 2.0 ** -53 * 4.5 / 3) and float(B[1, 1]) == pytest.approx(5 * 2.0 ** -53 * 1.25 / 3)
    # numpy's own fp64 product stays within the bound (far within: 0.27 of it at worst on the shapes of tests/test_gpu_grm.py)
    G = GU.pop_case(130, 300, 7).astype(np.float64)
    G = G[:, G.std(axis=0) > 0]
    Xs = (G - G.mean(axis=0)) / G.std(axis=0, ddof=1)
    err = np.abs((Xs @ Xs.T / Xs.shape[1]).astype(GU.LD) - GU.grm_ld(Xs))
    assert (err <= GU.grm_bound(Xs)).all()


def test_pop_case_has_three_populations_and_a_spectral_gap():
    G = GU.pop_case(120, 400, 3)
    assert G.dtype == np.int8 and G.shape == (120, 400) and set(np.unique(G)) == {0, 1, 2}
    np.testing.assert_array_equal(GU.pop_case(120, 400, 3), G)
    X = G.astype(np.float64)
    X = X[:, X.std(axis=0) > 0]
    Xs = (X - X.mean(axis=0)) / X.std(axis=0, ddof=1)
    lam, vec, gap, lam1 = GU.top_eig(GU.grm_ld(Xs), 2)
    assert (gap >= 0.1 * lam1).all()
    # the two PCs separate the three populations: within a population the scores agree far better than between them
    m = np.arange(120) % 6
    pop = np.where(m < 3, 0, np.where(m < 5, 1, 2))
    centres = np.stack([vec[pop == g].mean(axis=0) for g in range(3)])
    within = max(np.abs(vec[pop == g] - centres[g]).max() for g in range(3))
    between = min(np.linalg.norm(centres[a] - centres[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    assert between > 2 * within
