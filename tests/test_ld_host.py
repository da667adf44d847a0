"""Host: LD pruning (aq_prep_ld_prune, prepare_on_device(ld_prune=), atlasqtl(ld_prune=)) as far as it needs no device -- the
restatement of tests/ld_util.py on cases worked out by hand, every rejection of ld_prune_options, the refusal of
add_collinear_back, and the argument errors of the three C entries, which come before any device call."""
import ctypes as C

import numpy as np
import pytest

from atlasqtl_amd import _lib
from tests import ld_util as LU


def _band_from_corr(R, window):
    return LU.band_ld(None, window, gram=np.asarray(R, dtype=LU.LD))


def _corr6():
    """Six columns, correlations written by hand (symmetric, unit diagonal; only r^2 matters to the rule).
         0-1 0.95   0-2 0.10   1-2 0.95   2-3 0.60   3-4 0.92   2-4 0.91   4-5 0.99   3-5 0.20   0-5 0.99"""
    R = np.eye(6)
    for (i, j), v in {(0, 1): 0.95, (0, 2): 0.10, (1, 2): -0.95, (2, 3): 0.60, (3, 4): 0.92, (2, 4): 0.91, (4, 5): 0.99,
                      (3, 5): 0.20, (0, 5): 0.99}.items():
        R[i, j] = R[j, i] = v
    return R


def test_oracle_on_a_hand_written_six_column_case():
    R = _corr6()
    band = _band_from_corr(R, 5)
    assert np.isnan(band[0]).all() and band[1, 0] == LU.LD(0.95) and np.isnan(band[1, 1:]).all()
    assert band[5, 4] == LU.LD(0.99) and band[2, 0] == LU.LD(-0.95)        # (0, 5) at b = 4; the sign is kept
    # r2 = 0.8, window 5: 1 goes (tag 0); 2 stays (its partner 1 is gone, 0-2 is weak); 3 stays (0.36); 4 goes, tag 2 (the
    # smallest of 2 and 3); 5 goes: 4 is gone, but 0 is kept and 0.99^2 > 0.8
    rm, of, r2, margin = LU.greedy(band, 0.8, 5)
    assert list(rm) == [False, True, False, False, True, True]
    assert list(of) == [-1, 0, -1, -1, 2, 0]
    assert float(r2[1]) == pytest.approx(0.9025) and float(r2[4]) == pytest.approx(0.8281) and np.isnan(r2[[0, 2, 3]].astype(float)).all()
    assert margin == pytest.approx(0.8 - 0.36, abs=1e-12) or margin < 0.8 - 0.36
    # window 4: the pair (0, 5) is out of reach and 4 is gone, so 5 stays
    rm, of, _, _ = LU.greedy(_band_from_corr(R, 4), 0.8, 4)
    assert list(rm) == [False, True, False, False, True, False] and of[5] == -1
    # window 1: neighbours only; 2 stays because 1 is gone, 4 goes with tag 3, 5 stays
    rm, of, _, _ = LU.greedy(_band_from_corr(R, 1), 0.8, 1)
    assert list(rm) == [False, True, False, False, True, False] and list(of) == [-1, 0, -1, -1, 3, -1]
    # strictly greater: a threshold equal to an r^2 keeps the column
    rm, _, _, _ = LU.greedy(band, float(LU.LD(0.95) ** 2), 5)
    assert not rm[1] and rm[5]
    # r2 = 1 removes nothing
    assert not LU.greedy(band, 1.0, 5)[0].any()


def test_chain_keeps_the_first_and_the_third():
    _, R = LU.chain_abc()
    assert R[0, 1] ** 2 > 0.5 and R[1, 2] ** 2 > 0.5 and R[0, 2] ** 2 < 0.5
    rm, of, _, _ = LU.greedy(LU.band_ld(None, 2, gram=R), 0.5, 2)
    assert list(rm) == [False, True, False] and list(of) == [-1, 0, -1]


def test_groups_and_window_bp_decide_eligibility():
    R = _corr6()
    band = _band_from_corr(R, 5)
    # 0 | 1 2 3 | 4 5: the pairs 0-1 and 0-5 cross a border; 4-5 do not
    rm, of, _, _ = LU.greedy(band, 0.8, 5, group=np.array([0, 1, 1, 1, 2, 2]))
    assert list(rm) == [False, False, True, False, False, True] and list(of) == [-1, -1, 1, -1, -1, 4]
    # positions: 0-1 are 500 apart (out at 100 bp), 1-2 10 apart, 2-4 and 3-4 within 100, 4-5 and 0-5 far
    pos = np.array([0, 500, 510, 560, 600, 5000])
    rm, of, _, _ = LU.greedy(band, 0.8, 5, pos=pos, window_bp=100)
    assert list(rm) == [False, False, True, False, True, False] and list(of) == [-1, -1, 1, -1, 3, -1]
    assert LU.eligible(1, 3, 2) and not LU.eligible(1, 4, 2) and not LU.eligible(3, 3, 2)
    assert LU.eligible(0, 1, 1, pos=pos, window_bp=500) and not LU.eligible(0, 1, 1, pos=pos, window_bp=499)


def test_haplotype_copies_spread_r2():
    G, _ = LU.ld_case(333, 100, 2, seed=1)
    Xs, keep = LU.standardise(G)
    assert Xs.shape[1] <= 95 and not set(keep) & {3, 7, 11, 98, 99}     # a SNP nobody flipped is one more duplicate
    r2 = np.asarray(LU.band_ld(Xs, 1)[1:, 0], dtype=float) ** 2
    assert (r2 > 0.8).sum() >= 5 and (r2 < 0.2).sum() >= 5 and ((r2 > 0.2) & (r2 < 0.8)).sum() >= 5


def test_default_options():
    from atlasqtl_amd.prepare import ld_prune_options
    assert ld_prune_options({}) == {"r2": 0.8, "window": 500, "window_bp": None, "groups": None, "positions": None}
    o = ld_prune_options({"r2": 1, "window": np.int64(4096), "window_bp": 250000})
    assert o["r2"] == 1.0 and o["window"] == 4096 and o["window_bp"] == 250000


@pytest.mark.parametrize("bad", [
    "r2=0.5", ["r2"], {"r_2": 0.5}, {"r2": 0.0}, {"r2": -0.1}, {"r2": 1.0000001}, {"r2": float("nan")}, {"r2": "0.5"}, {"r2": None},
    {"r2": True}, {"window": 0}, {"window": 4097}, {"window": 2.5}, {"window": 10.0}, {"window": None}, {"window": True},
    {"window_bp": 0}, {"window_bp": -5}, {"window_bp": 1.5}, {"groups": 3}, {"groups": np.zeros((2, 2))}, {"groups": []},
    {"positions": [1.5, 2.0]}, {"positions": [1.0, float("nan")]}, {"positions": ["a", "b"]}, {"positions": np.zeros((2, 2), dtype=int)},
    {"positions": []},
])
def test_every_rejection_of_the_options(bad):
    from atlasqtl_amd.prepare import AtlasqtlError, ld_prune_options
    with pytest.raises(AtlasqtlError, match="ld_prune"):
        ld_prune_options(bad)


def test_python_validates_before_the_device():
    """Wrong lengths and window_bp without positions are found with the data in hand, still before the first device call."""
    from atlasqtl_amd.prepare import AtlasqtlError, prepare_on_device
    rng = np.random.default_rng(0)
    Y, X = rng.normal(size=(40, 2)), rng.normal(size=(40, 9))
    with pytest.raises(AtlasqtlError, match="window_bp needs positions"):
        prepare_on_device(Y, X, ld_prune={"window_bp": 1000})
    with pytest.raises(AtlasqtlError, match=r"groups must hold one entry per predictor given \(9\)"):
        prepare_on_device(Y, X, ld_prune={"groups": np.zeros(8, dtype=int)})
    with pytest.raises(AtlasqtlError, match=r"positions must hold one entry per predictor given \(9\)"):
        prepare_on_device(Y, X.astype(np.int8), ld_prune={"positions": np.arange(10), "window_bp": 5})
    with pytest.raises(AtlasqtlError, match="r2 must be"):
        prepare_on_device(Y, X, ld_prune={"r2": 2})
    import atlasqtl_amd as A
    with pytest.raises(AtlasqtlError, match="window must be"):
        A.atlasqtl(Y, X, p0=(2, 4), verbose=0, ld_prune={"window": 5000})


def test_add_collinear_back_is_refused_with_ld_prune():
    import atlasqtl_amd as A
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError, match="not a copy") as e:
        A.atlasqtl(rng.normal(size=(30, 2)), rng.normal(size=(30, 5)), p0=(2, 4), verbose=0, add_collinear_back=True, ld_prune={})
    assert "add_collinear_back" in str(e.value) and "ld_prune" in str(e.value)
    assert not isinstance(e.value, _lib.AtlasqtlHipError)


def _ld(window=10, r2=0.8, window_bp=0, pos=None):
    ld = _lib.AqPrepLd()
    ld.window, ld.r2, ld.group, ld.pos, ld.window_bp = window, r2, None, pos, window_bp
    return ld


def test_argument_errors_of_the_c_entries_come_before_the_device(hiplib):
    """AQ_ERR_ARG (1) and the entry's name: the struct is checked first, then the handle, and nothing touches a device."""
    def prune(h, ld):
        rc = hiplib.aq_prep_ld_prune(h, None if ld is None else C.byref(ld))
        return rc, hiplib.aq_last_error().decode()

    rc, msg = prune(None, None)
    assert rc == 1 and "aq_prep_ld_prune" in msg and "NULL" in msg
    rc, msg = prune(None, _ld())
    assert rc == 1 and "aq_prep_ld_prune" in msg and "NULL handle" in msg
    for w in (0, -3, 4097):
        rc, msg = prune(None, _ld(window=w))
        assert rc == 1 and "window must lie in [1, 4096]" in msg and str(w) in msg
    for r in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        rc, msg = prune(None, _ld(r2=r))
        assert rc == 1 and "r2 must lie in (0, 1]" in msg
    rc, msg = prune(None, _ld(window_bp=1000))
    assert rc == 1 and "window_bp" in msg and "pos" in msg
    pos = np.arange(4, dtype=np.int64)
    rc, msg = prune(None, _ld(window_bp=1000, pos=pos.ctypes.data_as(C.POINTER(C.c_int64))))
    assert rc == 1 and "NULL handle" in msg                              # the struct is fine now
    assert hiplib.aq_prep_ld_info(None, None, None, None, None) == 1
    assert "aq_prep_ld_info" in hiplib.aq_last_error().decode()
    out = np.zeros(4)
    assert hiplib.aq_prep_ld_band(None, 2, _lib.as_dp(out)) == 1
    assert "aq_prep_ld_band" in hiplib.aq_last_error().decode() and "NULL" in hiplib.aq_last_error().decode()
    for w in (0, 4097):
        assert hiplib.aq_prep_ld_band(None, w, _lib.as_dp(out)) == 1
        assert "window must lie in [1, 4096]" in hiplib.aq_last_error().decode()


def test_struct_and_binding_agree():
    """aq_prep_ld of the header against its ctypes mirror: names, order and C types."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "atlasqtl_hip.h")).read()
    body = re.search(r"typedef struct aq_prep_ld \{(.*?)\} aq_prep_ld;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": C.c_int32, "double": C.c_double, "const int32_t *": C.POINTER(C.c_int32), "int64_t": C.c_int64,
             "const int64_t *": C.POINTER(C.c_int64)}
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            m = re.match(r"\s*(.*?[\s\*])(\w+)\s*$", decl)
            fields.append((m.group(2), ctype[m.group(1).strip()]))
    assert fields == list(_lib.AqPrepLd._fields_)
