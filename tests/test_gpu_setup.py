"""GPU: what aq_vb_create builds once per handle -- the MFMA operand layouts XA / XU, the row panels XR, the Gram blocks G / Gx, the
per-trait Gram blocks GK, the index lists midx / mcnt4 / mobs and the trait-tiled mis, R, gam, mu -- read back through
aq_vb_debug_get_setup and held entry by entry to the restatement of tests/setup_util.py: the layouts bit for bit against the index
maps, every Gram entry against its long-double value under the bound derived there (whose FACTOR and constants come from the
derivations, not from these runs).  tests/test_setup_host.py shows on the CPU that the bounds hold for a correct implementation,
fail for a plain running sum and for a cancelling diagonal that is not redone, and that the inputs reach every edge the cases name.

Every case creates a handle, asserts from aq_vb_get_status and the geometry record that the planner gave it the kernel family it is
written for, reads the buffers and destroys the handle; no sweep runs.  The problems come from setup_util.make_setup_problem
(genotypes of tests.util's regime generator, explicit hyper-parameters): tests.util.make_problem cannot build p = 1 (its automatic
hyper-parameters have no solution there) and make_regime_problem refuses p <= 80.

Worst error / bound per case and buffer on an MI355X (-s prints them; DESIGN.md section 3 records them): G at most 0.35, Gx 0.43,
GK 0.42 (G - correction), 0.28 (direct sums) and 0.19 (redone diagonals) of their bars."""
import ctypes as C

import numpy as np
import pytest

from tests import setup_util as S

pytestmark = pytest.mark.gpu

MASK, WIDE = 1, 2                # aq_vb_status.instance_flags


def _read(run, name):
    """One buffer of the handle (None when the handle does not hold it)."""
    from atlasqtl_amd._lib import lib
    L = lib()
    nbytes = int(L.aq_vb_debug_get_setup(run.h, S.WHICH[name], None, 0))
    assert nbytes >= 0, L.aq_last_error()
    if nbytes == 0:
        return None
    dtype = np.int32 if name == "geometry" else S.DTYPES.get(name, np.float64)
    out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
    assert int(L.aq_vb_debug_get_setup(run.h, S.WHICH[name], out.ctypes.data_as(C.c_void_p), nbytes)) == nbytes, L.aq_last_error()
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _open(name, monkeypatch):
    """(problem, handle, status, geometry) of a case, the planner's family asserted."""
    from atlasqtl_amd.core import VbRun
    family, n, p, q, regime, pattern, env = S.CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)           # read by aq_vb_create
    prob = S.case_problem(name)
    run = VbRun(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], None, 0.1, 10, True, True)
    try:
        st = run.status()
        geo = dict(zip(S.GEOMETRY_FIELDS, (int(v) for v in _read(run, "geometry"))))
        assert len(geo) == len(S.GEOMETRY_FIELDS)
        want = {"complete": dict(use_la=1, la_mask=0, la_wide=0, use_mis=0, use_tw=0), "short": dict(use_la=1, la_mask=1, la_wide=0, use_mis=0, use_tw=0),
                "wide": dict(use_la=1, la_mask=1, la_wide=1, use_mis=0, use_tw=0), "fallback": dict(use_la=0, la_mask=0, la_wide=0, use_mis=1, use_tw=0)}[family]
        assert {k: geo[k] for k in want} == want, (geo, st)
        assert st["core_kernel"] == (3 if family == "fallback" else 0)
        assert st["instance_flags"] & 3 == {"complete": 0, "short": MASK, "wide": MASK | WIDE, "fallback": 0}[family]
        if family in ("short", "wide"):
            assert st["split_parts"] == (9 if family == "wide" else 1)
        assert st["it"] == 0 and st["tiles_per_group"] == 1
        assert geo["dmode"] == 0 and geo["nb"] == -(-p // 16) and geo["p_pad"] == 16 * geo["nb"]
        assert geo["ntile"] == -(-q // 16) and geo["q_pad"] == 16 * geo["ntile"]
        assert geo["n_pad"] == st["n_pad"] >= n and geo["n_pad"] % 16 == 0
        if family == "wide":
            assert geo["n_pad"] == 864
        if family != "complete":
            assert geo["Mmax"] == S.expected_mmax(prob["miss"], family == "wide") and geo["NR"] == geo["n_pad"] + 8
    except BaseException:
        run.close()
        raise
    return prob, run, st, geo


def _check_x_layouts(prob, run, geo):
    n, p = prob["X"].shape
    for name, idx in (("XA", S.map_xa(geo["nb"], geo["n_pad"], n, p, geo["dmode"])), ("XU", S.map_xu(geo["nb"], geo["n_pad"], n, p))):
        got = _read(run, name)
        assert got is not None and got.size == idx.size
        assert np.array_equal(_bits(got), _bits(S.gather(idx, prob["X"])).reshape(-1)), name


def _check_tiled(prob, run, geo, names):
    n, p, q = prob["n"], prob["p"], prob["q"]
    src = {"R": (np.nan_to_num(prob["Y"], nan=0.0), n, geo["n_pad"]), "mis": ((~prob["miss"]).astype(np.float64), n, geo["n_pad"]),
           "gam": (prob["list_init"]["gam_vb"], p, geo["p_pad"]), "mu": (prob["list_init"]["mu_beta_vb"], p, geo["p_pad"])}
    for name in names:
        mat, rows, rows_pad = src[name]
        idx = S.map_tiled(geo["ntile"], rows_pad, rows, q)
        got = _read(run, name)
        assert got is not None and got.size == idx.size, name
        assert np.array_equal(_bits(got), _bits(S.gather(idx, mat)).reshape(-1)), name      # padding zero, NaN -> 0 in R


def _check_gram(name, prob, run, geo):
    G, Gx = (_read(run, w).reshape(geo["nb"], 16, 16) for w in ("G", "Gx"))
    gram = S.gram_reference(prob["X"])
    ratios = S.check_gram(prob["X"], G, Gx, gram)
    print(f"\nSETUP {name} n_pad={geo['n_pad']} G={ratios['G']:.3f} Gx={ratios['Gx']:.3f}")
    assert ratios["G"] <= 1.0 and ratios["Gx"] <= 1.0, ratios
    return G, Gx, gram


def _check_lists(prob, run, geo, wide):
    midx, mcnt4, mobs = S.index_lists(prob["miss"], geo["n_pad"], geo["Mmax"], geo["q_pad"], wide)
    assert np.array_equal(_read(run, "midx").reshape(geo["q_pad"], geo["Mmax"]), midx)
    assert np.array_equal(_read(run, "mcnt4"), mcnt4)
    if wide:
        assert np.array_equal(_read(run, "mobs"), mobs)
    else:
        assert _read(run, "mobs") is None
    return mcnt4, mobs


@pytest.mark.parametrize("name", [n_ for n_, c in S.CASES.items() if c[0] == "complete"])
def test_complete_y_layouts_and_gram_blocks(name, monkeypatch):
    """Complete Y, look-ahead kernel: XA, XU, R, gam, mu bit for bit (padding zero), G bitwise symmetric with zero rows and columns
    beyond p, Gx block 0 zero, every entry of G and Gx inside the compensated sum's bound.  n = 4000 is where a plain running sum
    is two orders outside it."""
    prob, run, st, geo = _open(name, monkeypatch)
    try:
        for w in ("XR", "GK", "midx", "mcnt4", "mobs", "mis"):
            assert _read(run, w) is None, w
        _check_x_layouts(prob, run, geo)
        _check_tiled(prob, run, geo, ("R", "gam", "mu"))
        _check_gram(name, prob, run, geo)
    finally:
        run.close()


@pytest.mark.parametrize("name", [n_ for n_, c in S.CASES.items() if c[0] in ("short", "wide")])
def test_masked_lists_and_per_trait_gram_blocks(name, monkeypatch):
    """Y with missing values in the look-ahead kernel's MASK instances.  short-*: aq_k_gk_blocks + aq_k_gk_diag_exact, lists of
    0, 1, 15, 16, 17, 5 % and Mmax samples, rare variants whose carriers are all missing, LD pairs across the block borders.
    wide-*: aq_k_gk_blocks_g, traits on both sides of and at 2 m = n, listed by their missing or by their observed samples.
    Exact: midx / mcnt4 / mobs, mis and R, complete traits and padded slots = G / Gx, cross block 0 = 0.  Bounded: everything else."""
    family = S.CASES[name][0]
    prob, run, st, geo = _open(name, monkeypatch)
    try:
        assert _read(run, "XR") is None                      # released once the GK blocks were built
        _check_x_layouts(prob, run, geo)
        _check_tiled(prob, run, geo, ("R", "mis", "gam", "mu"))
        mcnt4, mobs = _check_lists(prob, run, geo, family == "wide")
        G, Gx, gram = _check_gram(name, prob, run, geo)
        GK = _read(run, "GK")
        assert GK.size == geo["ntile"] * geo["nb"] * S.GK_STRIDE
        ratios, counts = S.check_gk(prob["X"], prob["miss"], mcnt4, mobs, geo["q_pad"], G, Gx, GK, gram)
        print(f"SETUP {name} GK " + " ".join(f"{row}={ratios[row]:.3f}/{counts[row]}" for row in S.GK_ROWS if row in ratios))
        assert counts["redone"] > 0 and (counts["direct"] > 0) == (family == "wide")
        assert all(v <= 1.0 for v in ratios.values()), ratios
    finally:
        run.close()


def test_fallback_masked_kernel_row_panels_and_lists(monkeypatch):
    """AQ_KERNEL = 3, the only family whose XR outlives aq_vb_create: XR, midx / mcnt4, mis (and XA, XU, R, gam, mu) bit for bit."""
    name = "fallback-n50"
    prob, run, st, geo = _open(name, monkeypatch)
    try:
        assert _read(run, "GK") is None
        n, p = prob["X"].shape
        idx = S.map_xr(geo["nb"], geo["NR"], n, p)
        assert np.array_equal(_bits(_read(run, "XR")), _bits(S.gather(idx, prob["X"])).reshape(-1))
        _check_lists(prob, run, geo, False)
        _check_x_layouts(prob, run, geo)
        _check_tiled(prob, run, geo, ("R", "mis", "gam", "mu"))
        _check_gram(name, prob, run, geo)
    finally:
        run.close()


def test_hook_arguments_lengths_and_lifetime(monkeypatch):
    """The hook itself: bad arguments are errors with a message, a capacity that does not suffice copies nothing, a buffer the
    handle does not hold has length 0 (the generic kernel keeps no operand panels and no Gram blocks), and reading changes
    nothing the handle owns."""
    from atlasqtl_amd._lib import lib
    from atlasqtl_amd.core import VbRun
    L = lib()
    assert L.aq_vb_debug_get_setup(None, 0, None, 0) == -1 and b"NULL handle" in L.aq_last_error()
    prob = S.case_problem("fallback-n50")
    monkeypatch.setenv("AQ_KERNEL", "2")
    run = VbRun(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], None, 0.1, 10, True, True)
    try:
        live = int(L.aq_debug_live_device_bytes())
        for which in (-1, len(S.WHICH)):
            assert L.aq_vb_debug_get_setup(run.h, which, None, 0) == -1 and b"which" in L.aq_last_error()
        assert L.aq_vb_debug_get_setup(run.h, 0, None, -1) == -1
        assert L.aq_vb_debug_get_setup(run.h, 0, None, 8) == -1 and b"NULL buffer" in L.aq_last_error()
        geo = dict(zip(S.GEOMETRY_FIELDS, (int(v) for v in _read(run, "geometry"))))
        assert geo["use_tw"] == 1 and geo["use_la"] == 0 and run.status()["core_kernel"] == 2
        for w in ("XA", "XU", "XR", "G", "Gx", "GK", "midx", "mcnt4", "mobs"):
            assert _read(run, w) is None, w
        buf = np.full(4, -7.0)
        nbytes = L.aq_vb_debug_get_setup(run.h, S.WHICH["R"], buf.ctypes.data_as(C.c_void_p), buf.nbytes)
        assert nbytes == geo["ntile"] * geo["n_pad"] * 16 * 8 > buf.nbytes and np.all(buf == -7.0)
        _check_tiled(prob, run, geo, ("R", "mis", "gam", "mu"))
        assert int(L.aq_debug_live_device_bytes()) == live
    finally:
        run.close()
