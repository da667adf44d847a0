"""GPU: the relationship operator applied to a block of vectors (aq_prep_grm_apply, csrc/aq_pcs_kernels.h) against the
long-double restatement of tests/pcs_util.py run on the handle's own matrix, and the genotype PCs that subspace iteration
takes with it (genotype_pcs(solver="subspace"), atlasqtl(genotype_pcs={"solver": "subspace"})) against solver="eigh" on the
same device, at shapes chosen for the kernels' edges: the smallest shape there is; odd n (8-byte loads), p1 below one chunk
and one panel, L below one tile; exact tile sizes; one past the tile edges in n and in L; the widest block; and n past the
10 240 of the n x n route, odd and even."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests import grm_util as GU
from tests import pcs_util as PU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = os.path.join(ROOT, "tests", "golden", "plink_toy")
APPLY_CASES = [(2, 1, 1), (63, 17, 5), (64, 16, 16), (257, 1000, 17), (131, 700, 128), (10241, 96, 8), (20000, 64, 4)]
SPLIT_CASES = APPLY_CASES[1:4]
Y0 = functools.lru_cache(maxsize=None)(lambda n: np.zeros((n, 1), order="F"))
EIG_RTOL = 1.65e-14           # the bar of tests/test_pcs_host.py: ten times what the iteration measured against eigh there


@functools.lru_cache(maxsize=None)
def _apply_case(n, p, L):
    """(X, Q, Xs of the handle, the long-double Z, the matrix of elementwise bounds, the long-double trace), once per shape."""
    from atlasqtl_amd import prepare as P
    X, Q = PU.apply_case(n, p, L)
    prep = P.prepare_on_device(Y0(n), X)[0]
    Xs = prep.X_host()
    prep.close()
    assert Xs.shape == (n, p)
    Z, B, tr = PU.apply_ld(Xs, Q), PU.apply_bound(Xs, Q), PU.trace_ld(Xs)
    for a in (Xs, Z, B):
        a.setflags(write=False)
    return X, Q, Xs, Z, B, tr


def _check_apply(Zg, trg, n, p, L, label):
    X, Q, Xs, Z, B, tr = _apply_case(n, p, L)
    assert Zg.shape == (n, L) and np.isfinite(Zg).all()
    err = np.abs(Zg.astype(GU.LD) - Z)
    print(f"{label}: worst |error| / bound {float(np.max(err / B)):.3f}, trace rel. error "
          f"{float(abs(GU.LD(trg) - tr) / tr):.3e} (bound {(n + p) * GU.U:.3e})")
    assert (B > 0).all() and (err <= B).all()
    assert abs(GU.LD(trg) - tr) <= GU.LD((n + p) * GU.U) * tr


@pytest.mark.parametrize("n,p,L", APPLY_CASES)
def test_apply_against_the_long_double_restatement(n, p, L, monkeypatch):
    """Every entry within (n + p1 + 4) 2^-53 |Xs| (|Xs'| |Q|) / p1 of the long-double value; the trace within (n + p1) 2^-53
    relative of the long-double sum of squares / p1; two calls, the same bits; Q = 0 gives Z = 0 exactly, in a block next to a
    random one too."""
    from atlasqtl_amd import prepare as P
    monkeypatch.delenv("AQ_PCS_SPLITS", raising=False)
    X, Q, Xs, Z, B, tr = _apply_case(n, p, L)
    prep = P.prepare_on_device(Y0(n), X)[0]
    try:
        Zg, trg = prep.grm_apply(Q, return_trace=True)
        Zg2, trg2 = prep.grm_apply(Q, return_trace=True)
        Z0 = prep.grm_apply(np.zeros((n, L)))
        Qh = np.array(Q, order="F")
        Qh[:, L // 2:] = 0.0
        Zh = prep.grm_apply(Qh)
        Zp = prep.grm_apply(Q)                                    # without the trace: the same Z
    finally:
        prep.close()
    assert Zg.flags.f_contiguous and Zg.tobytes() == Zg2.tobytes() == Zp.tobytes() and trg == trg2
    _check_apply(Zg, trg, n, p, L, f"n={n} p1={p} L={L}")
    assert not Z0.any() and not np.signbit(Z0).any()
    assert not Zh[:, L // 2:].any()
    # an entry of the product depends on its own column of Q alone, whatever stands next to it
    np.testing.assert_array_equal(Zh[:, :L // 2], Zg[:, :L // 2])


@pytest.mark.parametrize("splits", [1, 3, 64])
def test_forced_splits_in_a_fresh_process(splits, tmp_path):
    """AQ_PCS_SPLITS = 1, 3 and 64 (at p1 = 16 and 17 that leaves all but one or two splits without a predictor) in a child
    process of its own: the plan has that many splits and the result stays within the same bound."""
    out = str(tmp_path / "z.npz")
    shapes = [f"{n},{p},{L}" for n, p, L in SPLIT_CASES]
    env = dict(os.environ, AQ_PCS_SPLITS=str(splits))
    r = subprocess.run([sys.executable, "-m", "tests.pcs_apply_child", out] + shapes, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    for (n, p, L), shape in zip(SPLIT_CASES, shapes):
        assert int(got[f"splits_{shape}"]) == splits and int(got[f"p1_{shape}"]) == p
        _check_apply(got[f"Z_{shape}"], float(got[f"tr_{shape}"]), n, p, L, f"S={splits} n={n} p1={p} L={L}")


def test_arguments_refused_on_a_handle(monkeypatch):
    """L outside [1, 128] is AQ_ERR_ARG and names the entry; so are forced splits outside [1, 64]."""
    import ctypes as C
    from atlasqtl_amd import _lib
    from atlasqtl_amd import prepare as P
    monkeypatch.delenv("AQ_PCS_SPLITS", raising=False)
    X, Q, *_ = _apply_case(63, 17, 5)
    prep = P.prepare_on_device(Y0(63), X)[0]
    try:
        L = _lib.lib()
        buf = np.zeros((63, 129), order="F")
        for bad in (0, 129, -1):
            assert L.aq_prep_grm_apply(prep.handle, _lib.as_dp(buf), bad, _lib.as_dp(buf), None) == 1
            msg = L.aq_last_error().decode()
            assert msg.startswith("aq_prep_grm_apply: L must lie in [1, 128]")
            ms = C.c_double(0.0)
            assert L.aq_prep_grm_apply_time(prep.handle, bad, 1, C.byref(ms), None) == 1
            assert L.aq_last_error().decode().startswith("aq_prep_grm_apply_time: L must lie in [1, 128]")
        assert L.aq_prep_grm_apply(prep.handle, None, 5, _lib.as_dp(buf), None) == 1
        assert "aq_prep_grm_apply" in L.aq_last_error().decode()
        with pytest.raises(P.AtlasqtlError, match="grm_apply: Q must be n x L"):
            prep.grm_apply(np.zeros((62, 5)))
        for bad in ("0", "65", "-3"):
            monkeypatch.setenv("AQ_PCS_SPLITS", bad)
            with pytest.raises(_lib.AtlasqtlHipError, match="aq_prep_grm_apply: AQ_PCS_SPLITS"):
                prep.grm_apply(Q)
    finally:
        prep.close()


# ---- genotype_pcs(solver="subspace") against solver="eigh" on the same device ----
def _check_against_eigh(X, k, label, **kw):
    """The criteria of tests/test_pcs_host.py with solver="eigh" as the truth, its gaps taken from the GRM it decomposes."""
    import atlasqtl_amd as A
    ref = A.genotype_pcs(X, k, **kw)
    lam_all, V_all, gap, lam1 = GU.top_eig(A.genotype_grm(X, **kw), k)
    np.testing.assert_allclose(lam_all, ref["eigenvalues"], rtol=1e-13)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = A.genotype_pcs(X, k, solver="subspace", **kw)
    assert out["solver"] == "subspace" and out["converged"] is True and 1 <= out["iterations"] <= 300
    assert ref["solver"] == "eigh" and ref["converged"] is True and ref["iterations"] == 0 and ref["residuals"] is None
    assert out["p_used"] == ref["p_used"]
    assert (out["residuals"] <= 1e-8).all()
    PU.check_pcs(out, ref["eigenvalues"], ref["pcs"], gap, lam1, k, EIG_RTOL, label)
    rel = np.abs(out["var_explained"] - ref["var_explained"]) / ref["var_explained"]
    print(f"{label}: var_explained rel. difference {rel}")
    assert (rel <= 1e-12).all()
    again = A.genotype_pcs(X, k, solver="subspace", **kw)
    assert all(np.array_equal(out[key], again[key]) for key in ("pcs", "eigenvalues", "var_explained", "residuals"))
    assert again["iterations"] == out["iterations"]
    return out, ref


def test_subspace_pcs_of_float64_input():
    _check_against_eigh(GU.pop_case(131, 700, 131700).astype(np.float64), 2, "float64 (131, 700)")


def test_subspace_pcs_of_int8_dosages():
    _check_against_eigh(GU.pop_case(257, 1000, 258000), 2, "int8 (257, 1000)")


def test_subspace_pcs_of_a_plink_bed():
    """6 samples, 3 variants with missing genotypes: the block is clipped to n - 1 = 5 vectors, more than K has rank."""
    import atlasqtl_amd as A
    out, ref = _check_against_eigh(A.PlinkBed(TOY, missing="mean"), 1, "plink_toy")
    assert out["pcs"].shape == (6, 1)


def test_subspace_pcs_with_covariates_and_with_ld_prune():
    from tests.cov_util import covariates
    G = GU.pop_case(131, 700, 131700)
    Z = covariates(131, 4, np.random.default_rng(831))
    _check_against_eigh(G, 2, "covariates", covariates=Z)
    out, ref = _check_against_eigh(G, 2, "ld_prune", ld_prune={"r2": 0.1, "window": 50})
    assert 1 < out["p_used"] < 700


def test_past_the_limit_of_the_n_by_n_route():
    """n = 10 241, p = 96, k = 2, oversample 6: accepted and converged where solver="eigh" is still refused, and checked
    against the p1 x p1 route (eigh of Xs' Xs / p1, mapped back by Xs and normalised)."""
    import atlasqtl_amd as A
    from atlasqtl_amd import prepare as P
    n, p = 10241, 96
    G = GU.pop_case(n, p, 10241096)
    with pytest.raises(P.AtlasqtlError, match="at most 10240"):
        A.genotype_pcs(G, 2)
    with pytest.raises(P.AtlasqtlError, match="at most 10240"):
        A.genotype_pcs(G, 2, solver="eigh")
    prep = P.prepare_on_device(Y0(n), G)[0]
    Xs = prep.X_host()
    prep.close()
    lam, V, gap, lam1 = PU.pcs_by_columns(Xs, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = A.genotype_pcs(G, 2, solver="subspace", oversample=6)
    assert out["converged"] is True and out["p_used"] == Xs.shape[1] and out["pcs"].shape == (n, 2)
    PU.check_pcs(out, lam, V, gap, lam1, 2, EIG_RTOL, "n=10241 p=96")
    tr = float(PU.trace_ld(Xs))
    assert np.abs(out["var_explained"] - lam / tr).max() <= 1e-12 * (lam / tr).max()


def test_atlasqtl_with_subspace_pcs():
    """atlasqtl(genotype_pcs={"k": 2, "solver": "subspace"}) at (131, 700, q = 4).
    Against the same PCs appended by hand it is the same code path on the same bits, the tolerance tests/test_gpu_grm.py uses
    for the eigh path against its own reference: none.  Against genotype_pcs=2 (eigh) on the same input the two runs are fed
    PCs that differ by at most the Davis-Kahan bound delta, stop after the same number of iterations, and gam_vb agrees to
    first order in delta: a log-odds behind an entry of gam_vb is an n-term sum of terms of order one, each moved by a relative
    delta when the covariates move by delta, the logistic function has slope <= 1/4, and the `it` sweeps add their shifts at
    most linearly: |gam_vb - gam_vb'| <= n it delta / 4."""
    import atlasqtl_amd as A
    n, p, q = 131, 700, 4
    G = GU.pop_case(n, p, 131700)
    rng = np.random.default_rng(23)
    Y = G[:, [20, 350]].astype(np.float64) @ rng.normal(size=(2, q)) + rng.normal(size=(n, q))
    kw = dict(p0=(2, 4), user_seed=3, verbose=0, maxit=60)
    a = A.atlasqtl(Y, G, genotype_pcs={"k": 2, "solver": "subspace"}, **kw)
    e = A.atlasqtl(Y, G, genotype_pcs=2, **kw)
    pcs = A.genotype_pcs(G, 2, solver="subspace")
    b = A.atlasqtl(Y, G, covariates=pcs["pcs"], **kw)
    np.testing.assert_array_equal(a.genotype_pcs, pcs["pcs"])
    np.testing.assert_array_equal(a.gam_vb, b.gam_vb)
    np.testing.assert_array_equal(a.beta_vb, b.beta_vb)
    assert a.it == b.it and a.lb_opt == b.lb_opt
    assert a.pc_solver == "subspace" and a.pc_converged is True and a.pc_iterations == pcs["iterations"] >= 1
    assert e.pc_solver == "eigh" and e.pc_converged is True and e.pc_iterations == 0
    assert a.n_covariates == e.n_covariates == 2 and "pc_solver" not in b
    np.testing.assert_array_equal(a.pc_eigenvalues, pcs["eigenvalues"])
    np.testing.assert_array_equal(a.pc_var_explained, pcs["var_explained"])
    # the PCs of the two paths
    lam, V, gap, lam1 = GU.top_eig(A.genotype_grm(G), 2)
    bound = 2 * pcs["residuals"] * lam1 / gap
    dist = np.array([np.linalg.norm(a.genotype_pcs[:, i] - e.genotype_pcs[:, i] * (e.genotype_pcs[:, i] @ a.genotype_pcs[:, i]))
                     for i in range(2)])
    delta = float(bound.max())
    diff = float(np.max(np.abs(a.gam_vb - e.gam_vb)))
    print(f"it {a.it} / {e.it}; PCs differ by {dist} (bound {bound}); max |gam_vb difference| {diff:.3e} "
          f"(bound {n * a.it * delta / 4:.3e})")
    assert (dist <= bound).all()
    assert a.it == e.it
    assert diff <= n * a.it * delta / 4
