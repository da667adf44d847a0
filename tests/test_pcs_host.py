"""Host: genotype PCs by subspace iteration (aq_prep_grm_apply, subspace_pcs_, genotype_pcs(solver="subspace")) as far as
they need no device -- the launch plan of aq_pcs_plan_query, the argument errors of the entries, the iteration itself on a
NumPy operator against eigh of K, and every host check of the solver options."""
import ctypes as C
import functools
import os
import re
import warnings

import numpy as np
import pytest

from atlasqtl_amd import _lib
from tests import grm_util as GU
from tests import pcs_util as PU

GB = 1 << 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(hiplib, n, p1, L, ncu=256, free=200 * GB):
    pl = _lib.AqPcsPlan()
    rc = hiplib.aq_pcs_plan_query(n, p1, L, ncu, free, C.byref(pl))
    return rc, pl


# ---- the plan ----
@pytest.mark.parametrize("n,p1,L", [(2, 1, 1), (131, 700, 10), (10240, 20000, 112), (82944, 50000, 128), (63, 17, 5),
                                    (257, 1000, 17), (10241, 96, 8), (20000, 64, 4)])
@pytest.mark.parametrize("ncu", [1, 64, 256, 304])
def test_plan_fields(hiplib, n, p1, L, ncu):
    rc, pl = _plan(hiplib, n, p1, L, ncu)
    assert rc == 0, hiplib.aq_last_error()
    # the block padded to the MFMA tile
    assert pl.lp % 16 == 0 and L <= pl.lp < L + 16 and pl.lp <= 128
    # the first product: the panels cover every predictor, the chunks every sample
    assert pl.panel == 64 and pl.n_panels == -(-p1 // 64)
    assert pl.sample_chunk == 32 and pl.n_pad % 32 == 0 and n <= pl.n_pad < n + 32
    # the second product: the tiles cover every sample, the splits every predictor exactly once
    assert pl.tile == 64 and pl.n_tiles == -(-n // 64)
    chunks = -(-p1 // pl.chunk)
    assert pl.chunk == 16 and 1 <= pl.splits <= 64 and pl.chunks_per_split == -(-chunks // pl.splits)
    assert pl.splits * pl.chunks_per_split * pl.chunk >= p1
    # one split when the tiles alone give two workgroups per CU; otherwise no more workgroups than that needs, and no
    # split the plan chose itself is shorter than 8 chunks
    if pl.n_tiles >= 2 * ncu:
        assert pl.splits == 1
    else:
        assert (pl.splits - 1) * pl.n_tiles < 2 * ncu
    assert pl.splits == 1 or pl.splits <= chunks // 8
    # the memory
    assert pl.t_bytes == pl.n_panels * 64 * pl.lp * 8
    assert pl.scratch_bytes == pl.splits * pl.n_tiles * 64 * pl.lp * 8
    assert pl.io_bytes == (2 * n * L + pl.n_pad * pl.lp) * 8
    assert pl.scratch_bytes + pl.t_bytes <= 200 * GB and pl.scratch_bytes + pl.t_bytes + pl.io_bytes <= 200 * GB
    # none of it grows as n^2
    assert pl.scratch_bytes + pl.t_bytes + pl.io_bytes < n * n * 8 or n < 4096
    rc2, pl2 = _plan(hiplib, n, p1, L, ncu)
    assert rc2 == 0 and bytes(pl) == bytes(pl2)


def test_plan_at_the_shapes_it_is_for(hiplib):
    rc, pl = _plan(hiplib, 10240, 20000, 26)
    assert rc == 0 and pl.lp == 32 and pl.n_panels == 313 and pl.n_tiles == 160 and pl.splits == 4      # ceil(512 / 160)
    rc, pl = _plan(hiplib, 82944, 50000, 128)
    assert rc == 0 and pl.lp == 128 and pl.n_tiles == 1296 and pl.splits == 1
    rc, pl = _plan(hiplib, 131, 700, 10)                                # 44 chunks: no split below 8 chunks
    assert rc == 0 and pl.n_tiles == 3 and pl.splits == 5


@pytest.mark.parametrize("n,p1,L", [(131, 700, 10), (10240, 20000, 112), (82944, 50000, 128)])
def test_plan_stays_within_the_free_memory(hiplib, n, p1, L):
    rc, full = _plan(hiplib, n, p1, L, ncu=2048)
    assert rc == 0
    fixed, one = full.t_bytes + full.io_bytes, full.scratch_bytes // full.splits
    for free in (fixed + full.scratch_bytes, fixed + max(full.scratch_bytes - 1, one), fixed + one + 5, fixed + one):
        rc, pl = _plan(hiplib, n, p1, L, ncu=2048, free=free)
        assert rc == 0 and pl.splits >= 1 and pl.t_bytes + pl.io_bytes + pl.scratch_bytes <= free
    assert _plan(hiplib, n, p1, L, ncu=2048, free=fixed + one)[1].splits == 1
    rc, _ = _plan(hiplib, n, p1, L, ncu=2048, free=fixed + one - 1)
    msg = hiplib.aq_last_error().decode()
    assert rc == 2 and "aq_pcs_plan_query" in msg and "free" in msg
    assert _plan(hiplib, n, p1, L, free=0)[0] == 2


def test_plan_argument_errors(hiplib):
    assert hiplib.aq_pcs_plan_query(100, 10, 4, 256, GB, None) == 1
    assert "aq_pcs_plan_query" in hiplib.aq_last_error().decode() and "NULL" in hiplib.aq_last_error().decode()
    for n, p1, L, ncu, free in ((100, 10, 0, 256, GB), (100, 10, 129, 256, GB), (100, 10, -1, 256, GB), (1, 10, 4, 256, GB),
                                (0, 10, 4, 256, GB), (100, 0, 4, 256, GB), (100, 10, 4, 0, GB), (100, 10, 4, 256, -1)):
        rc, _ = _plan(hiplib, n, p1, L, ncu, free)
        msg = hiplib.aq_last_error().decode()
        assert rc == 1 and "aq_pcs_plan_query" in msg
        if not 1 <= L <= 128:
            assert "L must lie in [1, 128]" in msg
    assert _plan(hiplib, 100, 10, 128)[0] == 0 and _plan(hiplib, 82944, 10, 1)[0] == 0 and _plan(hiplib, 20480, 100, 26)[0] == 0


def test_plan_struct_and_binding_agree():
    txt = open(os.path.join(ROOT, "include", "atlasqtl_hip.h")).read()
    body = re.search(r"typedef struct aq_pcs_plan \{(.*?)\} aq_pcs_plan;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    fields = [(d.split()[1], ctype[d.split()[0]]) for d in body.split(";") if d.strip()]
    assert fields == list(_lib.AqPcsPlan._fields_)
    assert C.sizeof(_lib.AqPcsPlan) == 10 * 4 + 3 * 8


def test_argument_errors_of_the_entries_come_before_the_device(hiplib):
    """AQ_ERR_ARG (1), naming the entry: a NULL handle or operand, and -- on a handle, which exists only where a device does --
    L outside [1, 128], which tests/test_gpu_pcs_subspace.py meets."""
    Q = np.zeros(4)
    assert hiplib.aq_prep_grm_apply(None, _lib.as_dp(Q), 1, _lib.as_dp(Q), None) == 1
    msg = hiplib.aq_last_error().decode()
    assert "aq_prep_grm_apply" in msg and "NULL handle" in msg
    ms = C.c_double(0.0)
    assert hiplib.aq_prep_grm_apply_time(None, 4, 1, C.byref(ms), None) == 1
    assert "aq_prep_grm_apply_time" in hiplib.aq_last_error().decode()


# ---- the iteration on a NumPy operator ----
CASES = [(131, 700, 5, 2, 8), (64, 300, 2, 2, 4), (300, 50, 1, 2, 8), (1000, 3000, 7, 2, 14)]


@functools.lru_cache(maxsize=None)
def _case(n, p, seed, k):
    """(Xs, trace K, eigenvalues, eigenvectors, gaps, lambda_1 of eigh of K), once per case."""
    Xs = PU.standardise(GU.pop_case(n, p, seed))
    K = GU.grm_ld(Xs)
    lam, V, gap, lam1 = GU.top_eig(K, k)
    for a in (Xs, lam, V, gap):
        a.setflags(write=False)
    return Xs, float(np.trace(K)), lam, V, gap, lam1


# The largest relative eigenvalue error measured on the four cases at both tolerances, against numpy.linalg.eigh of K, was
# 1.65e-15 (n = 300, p = 50, tol = 1e-11; printed when this file runs with -s); the bar is ten times that.
EIG_RTOL = 1.65e-14


@pytest.mark.parametrize("tol", [1e-8, 1e-11])
@pytest.mark.parametrize("n,p,seed,k,oversample", CASES)
def test_subspace_iteration_against_eigh_of_k(n, p, seed, k, oversample, tol):
    """Measured: the eigenvalues agree with eigh of K to <= 1.65e-15 relative on these cases (a Ritz value is second order
    in the vector's error), and every case converges in 8 ... 30 iterations."""
    from atlasqtl_amd.prepare import subspace_pcs_
    Xs, tr, lam, V, gap, lam1 = _case(n, p, seed, k)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = subspace_pcs_(PU.operator(Xs), n, k, oversample, tol, 100, 0, trace=tr)
    assert out["converged"] is True and 1 <= out["iterations"] <= 30
    assert (out["residuals"] <= tol).all() and (out["residuals"] >= 0).all()
    PU.check_pcs(out, lam, V, gap, lam1, k, EIG_RTOL, f"n={n} p={p} tol={tol}")
    np.testing.assert_array_equal(out["var_explained"], out["eigenvalues"] / tr)
    assert out["eigenvalues"][0] > out["eigenvalues"][1] > 0
    assert np.abs(out["pcs"].sum(axis=0)).max() <= 1e-9           # orthogonal to the intercept, as every column of Xs is


def test_non_convergence_warns_and_returns_an_orthonormal_basis():
    from atlasqtl_amd.prepare import subspace_pcs_
    Xs, tr, lam, V, gap, lam1 = _case(131, 700, 5, 2)
    with pytest.warns(UserWarning, match="has not converged after 2 iterations"):
        out = subspace_pcs_(PU.operator(Xs), 131, 2, 8, 1e-14, 2, 0, trace=tr)
    assert out["converged"] is False and out["iterations"] == 2 and (out["residuals"] > 1e-14).any()
    assert np.max(np.abs(out["pcs"].T @ out["pcs"] - np.eye(2))) <= 64 * GU.U * 2
    np.testing.assert_array_equal(out["pcs"], GU.pc_sign(out["pcs"]))
    assert np.isfinite(out["eigenvalues"]).all() and np.isfinite(out["var_explained"]).all()


def test_equal_inputs_give_equal_bits():
    from atlasqtl_amd.prepare import subspace_pcs_
    Xs, tr, *_ = _case(64, 300, 2, 2)
    a = subspace_pcs_(PU.operator(Xs), 64, 2, 4, 1e-8, 100, 3, trace=tr)
    b = subspace_pcs_(PU.operator(Xs), 64, 2, 4, 1e-8, 100, 3, trace=tr)
    for key in ("pcs", "eigenvalues", "var_explained", "residuals"):
        assert a[key].tobytes() == b[key].tobytes()
    assert a["iterations"] == b["iterations"] and a["converged"] and b["converged"]
    c = subspace_pcs_(PU.operator(Xs), 64, 2, 4, 1e-8, 100, 4, trace=tr)      # another seed: another start, the same answer
    assert c["pcs"].tobytes() != a["pcs"].tobytes()
    np.testing.assert_allclose(c["pcs"], a["pcs"], atol=1e-6)
    assert np.isnan(subspace_pcs_(PU.operator(Xs), 64, 2, 4, 1e-8, 100, 3)["var_explained"]).all()


def test_restatement_on_a_hand_made_case():
    Xs = np.array([[1.0, -2.0], [-1.0, 0.0], [0.0, 2.0]])
    Q = np.array([[1.0, 0.0], [2.0, 0.0], [-1.0, 0.0]])
    Z = PU.apply_ld(Xs, Q)
    # Xs' q = (-1, -4); Xs (Xs' q) = (7, 1, -8); / 2
    np.testing.assert_allclose(Z[:, 0].astype(float), [3.5, 0.5, -4.0], rtol=1e-15)
    assert (Z[:, 1] == 0).all() and Z.dtype == GU.LD
    B = PU.apply_bound(Xs, Q)
    # |Xs'| |q| = (3, 4); |Xs| that = (11, 3, 8); (3 + 2 + 4) 2^-53 / 2
    np.testing.assert_allclose(B[:, 0].astype(float), np.array([11.0, 3.0, 8.0]) * 9 * GU.U / 2, rtol=1e-15)
    assert (B[:, 1] == 0).all()
    assert float(PU.trace_ld(Xs)) == 5.0
    np.testing.assert_allclose(PU.operator(Xs)(Q), Z.astype(float), rtol=1e-15)
    # the p1 x p1 route gives the eigenpairs of K
    Xs = PU.standardise(GU.pop_case(300, 50, 1))
    lam, V, gap, lam1 = PU.pcs_by_columns(Xs, 2)
    lam_k, V_k, gap_k, lam1_k = GU.top_eig(GU.grm_ld(Xs), 2)
    np.testing.assert_allclose(lam, lam_k, rtol=1e-13)
    np.testing.assert_allclose(V, V_k, atol=1e-12)
    np.testing.assert_allclose(gap, gap_k, rtol=1e-10)


# ---- the option ----
def test_option_forms():
    from atlasqtl_amd.prepare import genotype_pcs_options
    assert genotype_pcs_options(3, 100) == {"k": 3, "ld_prune": None}
    assert genotype_pcs_options({"k": 3}, 100) == {"k": 3, "ld_prune": None}
    assert genotype_pcs_options({"k": 2, "solver": "subspace"}, 100) == {"k": 2, "ld_prune": None, "solver": "subspace"}
    o = genotype_pcs_options({"k": 2, "solver": "subspace", "oversample": 6, "tol": 1e-10, "max_iter": 50, "seed": 4}, 20000, d=3)
    assert o == {"k": 2, "ld_prune": None, "solver": "subspace", "oversample": 6, "tol": 1e-10, "max_iter": 50, "seed": 4}
    assert genotype_pcs_options({"k": 2, "solver": "eigh"}, 10240) == {"k": 2, "ld_prune": None, "solver": "eigh"}
    assert genotype_pcs_options({"k": 96, "solver": "subspace", "oversample": 32}, 82944)["k"] == 96
    assert genotype_pcs_options({"k": 2, "tol": 1}, 100)["tol"] == 1


def test_oversample_default_and_clip():
    from atlasqtl_amd.prepare import pc_solver_options
    assert pc_solver_options(2, 1000, "genotype_pcs") == dict(solver="eigh", oversample=16, tol=1e-8, max_iter=300, seed=0)
    assert pc_solver_options(2, 1000, "genotype_pcs", "subspace", 6)["oversample"] == 6
    assert pc_solver_options(96, 1000, "genotype_pcs", "subspace")["oversample"] == 16
    assert pc_solver_options(96, 1000, "genotype_pcs", "subspace", 32)["oversample"] == 32          # L = 128
    assert pc_solver_options(5, 12, "genotype_pcs", "subspace")["oversample"] == 6                  # L <= n - 1 = 11
    assert pc_solver_options(5, 12, "genotype_pcs", "subspace", 20)["oversample"] == 6
    assert pc_solver_options(2, 3, "genotype_pcs", "subspace")["oversample"] == 0


@pytest.mark.parametrize("bad,n,d,match", [
    ({"k": 2, "solver": "lanczos"}, 100, 0, "solver must be 'eigh' or 'subspace'"),
    ({"k": 2, "solver": None}, 100, 0, "solver must be"), ({"k": 2, "solver": 1}, 100, 0, "solver must be"),
    ({"k": 2, "solver": "subspace", "oversample": 2.0}, 100, 0, "oversample must be None or a whole number"),
    ({"k": 2, "solver": "subspace", "oversample": -1}, 100, 0, "oversample must be"),
    ({"k": 2, "solver": "subspace", "oversample": True}, 100, 0, "oversample must be"),
    ({"k": 2, "solver": "subspace", "max_iter": 0}, 100, 0, "max_iter must be a whole number >= 1"),
    ({"k": 2, "solver": "subspace", "max_iter": 10.0}, 100, 0, "max_iter must be"),
    ({"k": 2, "solver": "subspace", "seed": -1}, 100, 0, "seed must be a whole number >= 0"),
    ({"k": 2, "solver": "subspace", "seed": 0.5}, 100, 0, "seed must be"),
    ({"k": 2, "solver": "subspace", "tol": 0}, 100, 0, "tol must be a number > 0"),
    ({"k": 2, "solver": "subspace", "tol": -1e-8}, 100, 0, "tol must be"),
    ({"k": 2, "solver": "subspace", "tol": "1e-8"}, 100, 0, "tol must be"),
    ({"k": 2, "solver": "subspace", "tol": float("nan")}, 100, 0, "tol must be"),
    ({"k": 2, "solver": "subspace", "tol": True}, 100, 0, "tol must be"),
    ({"k": 96, "solver": "subspace", "oversample": 33}, 5000, 0, "k \\+ oversample must be at most 128"),
    ({"k": 2, "solver": "subspace", "oversample": 127}, 5000, 0, "k \\+ oversample must be at most 128"),
    ({"k": 2, "solver": "subspace"}, 82945, 0, "at most 82944"),
    ({"k": 2, "solver": "eigh"}, 10241, 0, "at most 10240"),
    ({"k": 97, "solver": "subspace"}, 20000, 0, r"k must lie in \[1, 96\]"),
    ({"k": 2.0, "solver": "subspace"}, 20000, 0, "k must be a whole number"),
    ({"k": 2, "solver": "subspace", "window": 5}, 100, 0, "genotype_pcs must be"),
    ({"solver": "subspace"}, 100, 0, "genotype_pcs must be"),
    # unchanged
    (2, 10241, 0, "at most 10240"), ({"k": 2}, 20000, 0, "at most 10240"), ({"k": 2, "window": 5}, 100, 0, "genotype_pcs must be"),
    ({"k": 2, "r2": 0.5}, 100, 0, "genotype_pcs must be"), ({"k": 2, "ld": None}, 100, 0, "genotype_pcs must be"),
    (0, 100, 0, r"k must lie in \[1, 96\]"), ({"k": 2, "ld_prune": {"r2": 2}}, 100, 0, "ld_prune: r2 must be"),
])
def test_every_rejection_of_the_option(bad, n, d, match):
    from atlasqtl_amd.prepare import AtlasqtlError, genotype_pcs_options
    with pytest.raises(AtlasqtlError, match=match) as e:
        genotype_pcs_options(bad, n, d)
    assert "genotype_pcs" in str(e.value)


def test_the_refusal_above_10240_names_the_other_solver():
    from atlasqtl_amd.prepare import AtlasqtlError, genotype_pcs_options
    with pytest.raises(AtlasqtlError, match='at most 10240 .* solver="subspace"'):
        genotype_pcs_options(2, 10241)


def test_python_validates_before_the_device():
    """Every check of the solver arguments runs on the host: no device is visible when the non-GPU tests run, so an
    AtlasqtlHipError ("no HIP device") would show a check that came too late -- and is the only thing left to fail for
    solver="subspace" at n = 10 241."""
    import atlasqtl_amd as A
    from atlasqtl_amd.prepare import AtlasqtlError
    rng = np.random.default_rng(0)
    Y, X = rng.normal(size=(40, 2)), rng.normal(size=(40, 9))
    kw = dict(p0=(2, 4), verbose=0)
    for bad, match in (({"solver": "qr"}, "solver must be"), ({"oversample": 1.5}, "oversample must be"), ({"tol": 0.0}, "tol must be"),
                       ({"max_iter": 0}, "max_iter must be"), ({"seed": -2}, "seed must be"),
                       ({"oversample": 127}, "k \\+ oversample must be at most 128")):
        with pytest.raises(AtlasqtlError, match=match):
            A.genotype_pcs(X, 2, **{"solver": "subspace", **bad})
        with pytest.raises(AtlasqtlError, match=match):
            A.atlasqtl(Y, X, genotype_pcs={"k": 2, "solver": "subspace", **bad}, **kw)
    with pytest.raises(AtlasqtlError, match=r"k must lie in \[1, 38\]"):
        A.genotype_pcs(X, 39, solver="subspace")
    with pytest.raises(AtlasqtlError, match="k must be a whole number"):
        A.genotype_pcs(X, 2.0, solver="subspace")
    with pytest.raises(AtlasqtlError, match="r2 must be"):
        A.genotype_pcs(X, 2, solver="subspace", ld_prune={"r2": 0})
    big = np.zeros((10241, 1), dtype=np.int8)
    with pytest.raises(AtlasqtlError, match="at most 10240"):
        A.genotype_pcs(big, 1)
    with pytest.raises(AtlasqtlError, match="at most 10240"):
        A.genotype_pcs(big, 1, solver="eigh")
    with pytest.raises(AtlasqtlError, match="at most 10240"):
        A.atlasqtl(np.zeros((10241, 1)), big, genotype_pcs={"k": 1, "solver": "eigh"}, **kw)
    if _lib.lib().aq_device_count() == 0:
        with pytest.raises(_lib.AtlasqtlHipError, match="no HIP device"):
            A.genotype_pcs(big, 1, solver="subspace")
        with pytest.raises(_lib.AtlasqtlHipError, match="no HIP device"):
            A.atlasqtl(np.zeros((10241, 1)), big, genotype_pcs={"k": 1, "solver": "subspace"}, **kw)
