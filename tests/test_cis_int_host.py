"""The host side of the interaction cis scan, without a GPU: the ABI entries and the mirrored plan struct; the planner through
aq_cisint_plan_query against aq_cis_plan_query on the same windows, and the LDS formula; the refusals of interaction_basis and
of cis_screen(interaction=) that come before the first device call; the long-double reference of tests/cisint_util.py against
an ordinary least-squares fit of y ~ 1 + Z + e + g + g o e, and what cisint_util.case plants."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from atlasqtl_amd import _lib
from atlasqtl_amd import cis as CIS
from atlasqtl_amd import cis_interaction as INT
from atlasqtl_amd.prepare import AtlasqtlError
from tests import cisint_util as CI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aq_cisint_plan_query", "aq_prep_cis_int", "aq_prep_cis_int_time")
SMALL = [(20, 5, 2), (50, 17, 5)]
CONFIGS = [(s, d, k) for s in SMALL for d in (0, 3) for k in CI.E_KINDS]


def _id(cfg):
    (n, p, q), d, kind = cfg
    return f"{n}x{p}x{q}-d{d}-{kind}"


def test_header_binding_and_library_agree(hiplib):
    txt = open(os.path.join(ROOT, "include", "atlasqtl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "aq_prep_handle": C.c_void_p, "const int32_t *": _lib.ip, "int32_t *": _lib.ip,
             "const double *": _lib.dp, "double *": _lib.dp, "int64_t *": C.POINTER(C.c_int64),
             "aq_cisint_plan *": C.POINTER(_lib.AqCisintPlan)}
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and hasattr(hiplib, name), name
        args = re.search(r"\bint " + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        types = [re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip() for a in args.split(",")]
        assert [ctype[t] for t in types] == list(_lib.SYMBOLS[name][1]), name
        assert _lib.SYMBOLS[name][0] is C.c_int
    body = re.search(r"typedef struct aq_cisint_plan \{(.*?)\} aq_cisint_plan;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            typ, names = decl.split(None, 1)
            fields += [(nm.strip(), {"int32_t": C.c_int32, "int64_t": C.c_int64, "aq_cis_plan": _lib.AqCisPlan}[typ])
                       for nm in names.split(",")]
    assert fields == list(_lib.AqCisintPlan._fields_)
    assert C.sizeof(_lib.AqCisintPlan) == C.sizeof(_lib.AqCisPlan) + 4 * 4 + 3 * 8


# ---- the planner ----
def _query(hiplib, n, p1, q, lo, hi, nb, ncu=256):
    lo32, hi32 = np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)
    pl = _lib.AqCisintPlan()
    rc = hiplib.aq_cisint_plan_query(n, p1, q, ncu, _lib.as_ip(lo32), _lib.as_ip(hi32), nb, C.byref(pl))
    return rc, pl


def test_plan_against_the_cis_plan_and_the_lds_formula(hiplib):
    n, p1, q = 1001, 5000, 130
    lo = np.arange(q) * 30
    hi = lo + 100
    hi[7] = lo[7]                                              # one trait without a window
    rc, pl = _query(hiplib, n, p1, q, lo, hi, 12)
    assert rc == 0
    cp = _lib.AqCisPlan()
    assert hiplib.aq_cis_plan_query(n, p1, q, 0, 256, _lib.as_ip(lo.astype(np.int32)), _lib.as_ip(hi.astype(np.int32)), 0, C.byref(cp)) == 0
    assert bytes(pl.cis) == bytes(cp) and cp.q_active == q - 1 and cp.masked == 0 and cp.pb == 0
    # two panels of 64 rows of 18 doubles; two columns of (double, int) candidates; per trait three doubles and four ints
    lds = 2 * 64 * 18 * 8 + 2 * 64 * 12 + 64 * (3 * 8 + 4 * 4)
    assert pl.lds_bytes == lds == 22528 and pl.lds_bytes == cp.lds_bytes + 64 * 8 and pl.lds_bytes <= 65536
    assert (pl.streams, pl.n_basis, pl.mult_pad) == (2, 12, 1008)
    assert pl.yo_bytes == 8 * (q - 1) * n and pl.pred_bytes == 36 * p1 and pl.basis_bytes == 8 * (12 * n + 1008)
    rc, pl = _query(hiplib, 16, p1, q, lo, lo, 1)              # no window at all; n a whole chunk
    assert rc == 0 and (pl.cis.n_items, pl.yo_bytes, pl.mult_pad) == (0, 8 * 16, 16)


def test_plan_refusals(hiplib):
    n, p1, q = 100, 500, 4
    lo, hi = np.zeros(q), np.full(q, 500)
    rc, pl = _query(hiplib, n, p1, q, lo, hi, 0)
    assert rc == 1 and b"aq_cisint_plan_query: n_basis >= 1 required" in hiplib.aq_last_error() and pl.streams == 0 and pl.cis.tile == 0
    assert _query(hiplib, n, p1, q, lo, hi, 256)[0] == 0
    rc, pl = _query(hiplib, n, p1, q, lo, hi, 257)
    assert rc == 3 and b"at most 256" in hiplib.aq_last_error() and pl.streams == 0
    rc, _ = _query(hiplib, n, p1, q, lo, np.full(q, 501), 2)
    assert rc == 1 and b"outside [0, 500]" in hiplib.aq_last_error()
    assert _query(hiplib, 80000, 10, 7000, np.zeros(7000), np.full(7000, 10), 2)[0] == 3 and b"exceed 4 GiB" in hiplib.aq_last_error()
    lo32 = np.zeros(q, dtype=np.int32)
    assert hiplib.aq_cisint_plan_query(n, p1, q, 256, _lib.as_ip(lo32), _lib.as_ip(lo32), 2, None) == 1
    assert hiplib.aq_cisint_plan_query(n, p1, q, 256, None, _lib.as_ip(lo32), 2, C.byref(_lib.AqCisintPlan())) == 1
    # the entries refuse NULL arguments, the handle among them, before anything else
    d = C.c_double(0.0)
    v = np.zeros(4)
    assert hiplib.aq_prep_cis_int(None, _lib.as_ip(lo32), _lib.as_ip(lo32), _lib.as_dp(v), 1, _lib.as_dp(v), _lib.as_dp(v), -1,
                                  *([None] * 9)) == 1
    assert b"aq_prep_cis_int: NULL handle" in hiplib.aq_last_error()
    assert hiplib.aq_prep_cis_int(None, _lib.as_ip(lo32), _lib.as_ip(lo32), None, 1, _lib.as_dp(v), _lib.as_dp(v), 0, *([None] * 9)) == 1
    assert b"NULL s_lo, s_hi, basis, mult or r2_cut" in hiplib.aq_last_error()
    assert hiplib.aq_prep_cis_int_time(None, _lib.as_ip(lo32), _lib.as_ip(lo32), _lib.as_dp(v), 1, _lib.as_dp(v), 0, C.byref(d), C.byref(d),
                                       None) == 1
    assert b"aq_prep_cis_int_time: NULL handle" in hiplib.aq_last_error()
    assert hiplib.aq_prep_cis_int_time(None, _lib.as_ip(lo32), _lib.as_ip(lo32), _lib.as_dp(v), 1, _lib.as_dp(v), 1, None, C.byref(d),
                                       None) == 1
    assert b"aq_prep_cis_int_time: NULL argument" in hiplib.aq_last_error()


# ---- interaction_basis and the refusals of cis_screen ----
def test_interaction_basis_spans_one_covariates_and_e():
    rng = np.random.default_rng(3)
    n = 40
    Z, e = rng.standard_normal((n, 3)), rng.standard_normal(n) + 2.0
    for cov, d in ((None, 0), (Z, 3)):
        B, m = INT.interaction_basis(e, cov, n, d)
        Q, m2 = CI.basis(e, cov)
        assert B.shape == (d + 2, n) and B.flags["C_CONTIGUOUS"] and B.dtype == np.float64
        np.testing.assert_allclose(m, e - e.mean(), rtol=0, atol=1e-15)
        np.testing.assert_array_equal(m, m2)
        assert np.max(np.abs(B @ B.T - np.eye(d + 2))) < 1e-14
        assert np.max(np.abs(B.T @ B - Q.T @ Q)) < 1e-13          # the same span as the QR basis
        np.testing.assert_allclose(B[0], 1.0 / np.sqrt(n))
        assert np.linalg.norm(m - B.T @ (B @ m)) <= 1e-14 * np.linalg.norm(m)


def test_interaction_basis_refusals():
    rng = np.random.default_rng(4)
    n = 30
    Z, e = rng.standard_normal((n, 2)), rng.standard_normal(n)
    with pytest.raises(AtlasqtlError, match=r"one value per sample \(30\)"):
        INT.interaction_basis(e[:-1], None, n, 0)
    with pytest.raises(AtlasqtlError, match="one value per sample"):
        INT.interaction_basis(np.stack([e, e], axis=1), None, n, 0)
    bad = e.copy()
    bad[3] = np.nan
    with pytest.raises(AtlasqtlError, match="finite without missing value"):
        INT.interaction_basis(bad, None, n, 0)
    bad[3] = np.inf
    with pytest.raises(AtlasqtlError, match="finite without missing value"):
        INT.interaction_basis(bad, None, n, 0)
    with pytest.raises(AtlasqtlError, match="interaction is constant"):
        INT.interaction_basis(np.full(n, 2.5), None, n, 0)
    with pytest.raises(AtlasqtlError, match="span of the intercept and the covariates"):
        INT.interaction_basis(3.0 + 2.0 * Z[:, 0] - Z[:, 1], Z, n, 2)
    with pytest.raises(AtlasqtlError, match="have rank 0, but the data were prepared with 2"):
        INT.interaction_basis(e, None, n, 2)
    with pytest.raises(AtlasqtlError, match="have rank 2, but the data were prepared with 0"):
        INT.interaction_basis(e, Z, n, 0)
    dup = np.column_stack([Z, Z[:, 0] + Z[:, 1]])              # a collinear column is dropped: rank 2, not 3
    with pytest.raises(AtlasqtlError, match="have rank 2, but the data were prepared with 3"):
        INT.interaction_basis(e, dup, n, 3)
    assert INT.interaction_basis(e, dup, n, 2)[0].shape == (4, n)
    with pytest.raises(AtlasqtlError, match="one row per sample"):
        INT.interaction_basis(e, Z[:-1], n, 2)


def test_cis_screen_refuses_before_any_device_call(monkeypatch):
    """Every refusal comes from the host: the preparation, the first thing that touches a device, is never reached."""
    import atlasqtl_amd as A

    def no_device(*a, **k):
        raise AssertionError("the preparation was reached")
    monkeypatch.setattr(CIS, "prepare_data_", no_device)
    n, p, q = 20, 5, 2
    X, Y, Z, e = CI.case(n, p, q, 3, "continuous")
    kw = dict(trait_chrom=["1"] * q, trait_start=np.full(q, 2), window=10, snp_chrom=["1"] * p, snp_pos=np.arange(p))
    with pytest.raises(AtlasqtlError, match="interaction= together with permutations="):
        A.cis_screen(Y, X, interaction=e, permutations=10, **kw)
    with pytest.raises(AtlasqtlError, match="interaction= together with condition_on="):
        A.cis_screen(Y, X, interaction=e, condition_on=[[0], []], **kw)
    Yn = np.array(Y)
    Yn[3, 1] = np.nan
    with pytest.raises(AtlasqtlError, match="interaction= needs complete Y"):
        A.cis_screen(Yn, X, interaction=e, **kw)
    with pytest.raises(AtlasqtlError, match="interaction is constant"):
        A.cis_screen(Y, X, interaction=np.ones(n), **kw)
    with pytest.raises(AtlasqtlError, match=r"one value per sample \(20\)"):
        A.cis_screen(Y, X, interaction=e[:-1], **kw)
    with pytest.raises(AtlasqtlError, match="span of the intercept and the covariates"):
        A.cis_screen(Y, X, interaction=Z[:, 1] + 1.0, covariates=Z, **kw)
    with pytest.raises(AssertionError, match="the preparation was reached"):     # a good call gets as far as the preparation
        A.cis_screen(Y, X, interaction=e, covariates=Z, **kw)


# ---- the reference ----
@pytest.mark.parametrize("cfg", CONFIGS, ids=[_id(c) for c in CONFIGS])
def test_reference_is_the_ols_t_of_the_interaction_coefficient(cfg):
    (n, p, q), d, kind = cfg
    X, Y, Z, e = CI.case(n, p, q, d, kind)
    Xs, Yc = CI.prepared(X, Y, Z)
    B, m = CI.basis(e, Z)
    lo, hi = CI.windows("all", p, q)
    ref = CI.reference(Xs, Yc, lo, hi, B, m)
    assert ref["df"] == n - 4 - d and ref["defined"].sum() >= (p - 2) * q
    r = np.asarray(ref["r"], dtype=np.float64)
    base = [np.ones(n)] + ([Z[:, l] for l in range(d)] if d else []) + [e]
    worst = 0.0
    for s, t in zip(*np.nonzero(ref["defined"])):
        g = Xs[:, s]
        D = np.column_stack(base + [g, g * e])                 # e itself, not centred: g is in the model
        beta, _, rank, _ = np.linalg.lstsq(D, Yc[:, t], rcond=None)
        assert rank == d + 4
        res = Yc[:, t] - D @ beta
        cov = (res @ res) / (n - d - 4) * np.linalg.inv(D.T @ D)
        t_ols = beta[-1] / np.sqrt(cov[-1, -1])
        t_ref = CI.t_of(r[s, t], ref["df"])
        worst = max(worst, abs(t_ref - t_ols) / abs(t_ols))
        assert abs(t_ref - t_ols) <= 1e-8 * abs(t_ols), (s, t, t_ref, t_ols)
    print(f"{_id(cfg)}: worst |t_ref - t_ols| / |t_ols| {worst:.2e} over {int(ref['defined'].sum())} pairs")
    # a constant added to e, or e rescaled, leaves r within the bounds
    for e2 in (e + 7.25, -3.0 * e):
        B2, m2 = CI.basis(e2, Z)
        ref2 = CI.reference(Xs, Yc, lo, hi, B2, m2)
        np.testing.assert_array_equal(ref2["defined"], ref["defined"])
        sign = np.sign((e2 - e2.mean()) @ (e - e.mean()))       # -3 e turns the sign of g o e, and of r
        ok = ref["defined"]
        assert (np.abs(sign * ref2["r"][ok] - ref["r"][ok]) <= ref["bound"][ok] + ref2["bound"][ok]).all()


@pytest.mark.parametrize("cfg", CONFIGS, ids=[_id(c) for c in CONFIGS])
def test_case_inputs_hold_their_plants(cfg):
    (n, p, q), d, kind = cfg
    X, Y, Z, e = CI.case(n, p, q, d, kind)
    Xs, Yc = CI.prepared(X, Y, Z)
    B, m = CI.basis(e, Z)
    if kind == "binary":
        assert set(np.unique(e)) == {0.0, 1.0} and (X[e == 0, CI.ZERO] == 0).all() and (X[e == 1, CI.ZERO] != 0).all()
    np.testing.assert_array_equal(X[:, CI.EQ], e)
    for pattern in CI.PATTERNS:
        lo, hi = CI.windows(pattern, p, q)
        ref = CI.reference(Xs, Yc, lo, hi, B, m)
        assert CI.thresholds_are_clear(ref) and CI.plants_hold(ref, kind, d, lo, hi)
        assert np.isnan(ref["int_tol"][CI.EQ]) and (np.asarray(ref["int_tol"][3:], dtype=np.float64) > 1e-6).all()
