"""CPU: the restatement of aq_vb_create's set-up (tests/setup_util.py) checked against itself, before tests/test_gpu_setup.py
holds a handle's buffers to it: the index maps address every source entry exactly once; fp64 restatements of the device
algorithms -- the compensated dot product, G minus an in-order correction, the direct sum, the double-double redo -- stay inside
the derived bounds at every case of the GPU file; a plain running sum and an un-redone cancelling diagonal do not (so the bounds
would notice either defect coming back); and the inputs hold what the cases claim.  Run with -s for the ratios."""
import numpy as np
import pytest

from tests import setup_util as S

MASKED = [name for name, c in S.CASES.items() if c[0] in ("short", "wide")]
SHORT = [name for name, c in S.CASES.items() if c[0] == "short"]
WIDE = [name for name, c in S.CASES.items() if c[0] == "wide"]


def _lists(name, n_pad=None):
    """The index lists of a masked case as aq_vb_create would lay them out (n_pad only names the padding row)."""
    family, n, p, q, regime, pattern, env = S.CASES[name]
    prob = S.case_problem(name)
    wide = family == "wide"
    n_pad = n_pad or -(-n // 16) * 16
    q_pad = -(-q // 16) * 16
    Mmax = S.expected_mmax(prob["miss"], wide)
    return (n_pad, q_pad, Mmax) + S.index_lists(prob["miss"], n_pad, Mmax, q_pad, wide)


_restated = {}


def _restated_case(name):
    """(gram reference, G, Gx by the compensated sum; for a masked case also the lists and the restated GK), once per case."""
    if name not in _restated:
        prob = S.case_problem(name)
        gram = S.gram_reference(prob["X"])
        G, Gx = S.kahan_gram_f64(prob["X"])
        out = dict(gram=gram, G=G, Gx=Gx)
        if name in MASKED:
            n_pad, q_pad, Mmax, midx, mcnt4, mobs = _lists(name)
            out.update(n_pad=n_pad, q_pad=q_pad, midx=midx, mcnt4=mcnt4, mobs=mobs,
                       ref=S.gk_reference(prob["X"], prob["miss"], mcnt4, mobs, gram),
                       GK=S.gk_restated_f64(prob["X"], midx, mcnt4, mobs, n_pad, G, Gx))
        _restated[name] = out
    return _restated[name]


# ------------------------------------------------------------------------------------------------------------------------------
# the maps

@pytest.mark.parametrize("n,p,n_pad", [(17, 1, 32), (50, 17, 64), (333, 48, 336), (300, 40, 336), (857, 40, 864)])
def test_x_maps_address_every_entry_once(n, p, n_pad):
    nb = -(-p // 16)
    for idx in (S.map_xa(nb, n_pad, n, p), S.map_xa(nb, n_pad, n, p, dmode=1), S.map_xu(nb, n_pad, n, p), S.map_xr(nb, n_pad + 8, n, p)):
        assert np.array_equal(np.sort(idx[idx >= 0]), np.arange(n * p))
        assert idx.min() >= -1
    assert S.map_xa(nb, n_pad, n, p).shape == (nb, n_pad // 16, 2, 64, 2) and S.map_xr(nb, n_pad + 8, n, p).size == nb * (n_pad + 8) * 16
    X = np.arange(1.0, n * p + 1).reshape(n, p, order="F")
    xr = S.gather(S.map_xr(nb, n_pad + 8, n, p), X)
    assert not xr[:, n:].any() and np.array_equal(xr[0, :n, :min(p, 16)], X[:, :16])       # row n_pad of every panel is zero


@pytest.mark.parametrize("rows,q,rows_pad", [(17, 1, 32), (50, 17, 64), (40, 20, 48), (300, 20, 336)])
def test_tiled_map_addresses_every_entry_once(rows, q, rows_pad):
    ntile = -(-q // 16)
    idx = S.map_tiled(ntile, rows_pad, rows, q)
    assert idx.shape == (ntile, rows_pad, 16)
    assert np.array_equal(np.sort(idx[idx >= 0]), np.arange(rows * q))
    M = np.arange(1.0, rows * q + 1).reshape(rows, q, order="F")
    t = S.gather(idx, M)
    assert t[(q - 1) // 16, 3, (q - 1) % 16] == M[3, q - 1] and not t[:, rows:].any() and not t[-1, :, (q - 1) % 16 + 1:].any()


def test_gk_offsets_fill_the_stride_exactly_once():
    diag, cross = S.gk_offsets()
    i, j, k = np.indices((16, 16, 16))
    assert np.all((diag >= 0) == (i >= j))
    every = np.concatenate([diag[diag >= 0], cross.reshape(-1)])
    assert np.array_equal(np.sort(every), np.arange(S.GK_STRIDE))
    assert diag[diag >= 0].max() == S.GK_DIAG - 1 and cross.min() == S.GK_DIAG
    d = np.arange(16.0 ** 3).reshape(1, 16, 16, 16)
    packed = S.pack_gk(d, -d)
    assert packed.shape == (1, S.GK_STRIDE)
    assert packed[0, (5 * 6 // 2 + 2) * 16 + 7] == d[0, 5, 2, 7] and packed[0, S.GK_DIAG + (16 * 2 + 5) * 16 + 7] == -d[0, 2, 5, 7]


@pytest.mark.parametrize("name", MASKED)
def test_index_lists_hold_every_listed_sample_once(name):
    family, n, p, q = S.CASES[name][:4]
    n_pad, q_pad, Mmax, midx, mcnt4, mobs = _lists(name)
    miss = S.case_problem(name)["miss"]
    assert Mmax % 16 == 0 and midx.shape == (q_pad, Mmax)
    for k in range(q_pad):
        row = midx[k]
        real = row[row != n_pad]
        want = np.zeros(n, dtype=bool) if k >= q else (~miss[:, k] if mobs[k] else miss[:, k])
        assert np.array_equal(real, np.nonzero(want)[0]) and np.all(row[real.size:] == n_pad)
        assert 4 * mcnt4[k] == -(-real.size // 16) * 16 <= Mmax
        assert real.size <= n - real.size or family != "wide"          # the wide split lists the shorter side
        if k < q and family == "wide":
            assert mobs[k] == (2 * int(miss[:, k].sum()) > n)
    assert not mobs[q:].any() and (family == "wide" or not mobs.any())


# ------------------------------------------------------------------------------------------------------------------------------
# the inputs hold what the cases claim

def test_case_table_holds_the_shapes():
    complete = {(c[1], c[2], c[3]) for c in S.CASES.values() if c[0] == "complete"}
    assert complete == {(n, p, q) for n in S.COMPLETE_N for p in S.COMPLETE_P for q in S.COMPLETE_Q} | {(4000, 48, 17)}
    assert S.COMPLETE_P == (1, 15, 16, 17, 33, 48) and S.COMPLETE_N == (17, 50, 333) and S.COMPLETE_Q == (1, 17)
    assert {(c[1], c[2], c[3]) for n_, c in S.CASES.items() if n_ in SHORT} == {(300, 40, 20), (1000, 40, 20), (1040, 40, 20)}
    assert {S.CASES[n_][4] for n_ in SHORT if S.CASES[n_][1] == 300} == {("rare",), ("ld",), ("ld", "rare")}
    assert ("rare",) == S.CASES["short-rare-n1000"][4]
    assert {(c[1], c[2], c[3]) for n_, c in S.CASES.items() if n_ in WIDE} == {(857, 40, 20), (856, 40, 20)}
    assert all(S.CASES[n_][6] == {"AQ_LA_C": "9"} for n_ in WIDE)
    assert S.CASES["fallback-n50"][1:4] == (50, 17, 5) and S.CASES["fallback-n50"][6] == {"AQ_KERNEL": "3"}


@pytest.mark.parametrize("name", list(S.CASES))
def test_problem_has_the_shape_it_names(name):
    family, n, p, q, regime = S.CASES[name][:5]
    prob = S.case_problem(name)
    assert prob["X"].shape == (n, p) and prob["Y"].shape == (n, q) and np.all(np.isfinite(prob["X"]))
    assert np.array_equal(np.isnan(prob["Y"]), prob["miss"]) and prob["miss"].any() == (family != "complete")
    assert np.allclose(np.sum(prob["X"] ** 2, axis=0), n - 1)
    for key in ("gam_vb", "mu_beta_vb"):
        assert np.unique(prob["list_init"][key]).size == p * q           # a misplaced entry of gam / mu cannot go unseen
    assert bool(prob["carriers"]) == ("rare" in regime)


@pytest.mark.parametrize("name", SHORT)
def test_short_cases_hold_every_list_length(name):
    n = S.CASES[name][1]
    prob = S.case_problem(name)
    m = prob["miss"].sum(axis=0)
    Mmax = S.expected_mmax(prob["miss"], False)
    assert Mmax == S.short_longest(n) <= S.MIS_MMAX and (n != 1040 or Mmax == S.MIS_MMAX)
    assert {0, 1, 15, 16, 17, Mmax} <= set(int(v) for v in m)
    assert any(0.03 * n < v < 0.08 * n for v in m)                          # about 5 %
    assert m[16:].min() == 0 and m[16:].max() > 0 and m[:16].min() == 0     # both tiles hold complete and incomplete traits
    if prob["carriers"]:
        dropped = [(j, k) for j, rows in prob["carriers"].items() for k in range(20) if prob["miss"][rows, k].all() and m[k] < 0.5 * n]
        assert {k for j, k in dropped} >= {7, 8, 9, 16}
        assert 39 in {j for j, k in dropped} and {j // 16 for j, k in dropped} == {0, 1, 2}      # every SNP block, and the last column


@pytest.mark.parametrize("name", SHORT)
def test_ld_cases_hold_a_pair_across_each_border(name):
    if "ld" not in S.CASES[name][4]:
        return
    from tests.util import block_borders, r2_pair
    X = S.case_problem(name)["X"]
    gram = _restated_case(name)["gram"]
    for c in block_borders(X.shape[1]):
        assert r2_pair(X, c - 1, c) > 0.9
        assert abs(float(gram["Gx"][c // 16, 0, 15])) > 0.9 * (X.shape[0] - 1)      # Gx is not small


def test_wide_cases_hold_both_sides_of_the_list_switch():
    seen = set()
    for name in WIDE:
        n = S.CASES[name][1]
        prob = S.case_problem(name)
        m = prob["miss"].sum(axis=0)
        seen |= {"2m=n" for v in m if 2 * v == n} | {"2m=n+1" for v in m if 2 * v == n + 1} | {"2m>n" for v in m if 2 * v > n + 1}
        seen |= {"2m<n" for v in m if 0 < 2 * v < n}
        n_pad, q_pad, Mmax, midx, mcnt4, mobs = _lists(name)
        lengths = {int((midx[k] != n_pad).sum()) for k in range(20)}
        assert {0, 1, 15, 16, 17} <= lengths and max(lengths) == n // 2 and Mmax == -(-(n // 2) // 16) * 16
        assert {int(mobs[k]) for k in range(20) if int((midx[k] != n_pad).sum()) in (1, 15, 16, 17)} == {0, 1}
        # all carriers of a rare variant missing: in an indirect trait and in a direct one, in both trait tiles
        gone = {(k, int(mobs[k])) for j, rows in prob["carriers"].items() for k in range(20) if prob["miss"][rows, k].all() and m[k] < n - 20}
        assert {(7, 1), (8, 0), (16, 1), (18, 0)} <= gone
    assert seen == {"2m=n", "2m=n+1", "2m>n", "2m<n"}


@pytest.mark.parametrize("name", MASKED)
def test_redo_threshold_is_clear_and_reached(name):
    """At least one diagonal entry lies below G_jj / 8, none within 1 % of it (the reference cannot know which side the device
    took), and every redone entry is far from the size at which the bound's second-order terms would count."""
    r = _restated_case(name)
    ref, n = r["ref"], S.CASES[name][1]
    assert ref["redone"].any()
    assert ref["margin"].min() > S.REDO_CLEAR, ref["margin"].min()
    for k, b, j in zip(*np.nonzero(ref["redone"])):
        assert ref["D"][k][b, j, j] / r["gram"]["G"][b, j, j] > 100 * (n * n + 2 * n) * S.U
    if S.CASES[name][0] == "short" and "rare" in S.CASES[name][4]:       # the rare variants are among them, not only the long list
        assert {7, 8, 9, 16} <= {int(k) for k in np.nonzero(ref["redone"])[0]}
    if S.CASES[name][0] == "wide":
        assert {8, 18} <= {int(k) for k in np.nonzero(ref["redone"])[0]}
        assert not ref["redone"][r["mobs"][:20] == 1].any()


# ------------------------------------------------------------------------------------------------------------------------------
# the restated algorithms stay inside the bounds, two subtly wrong ones do not

@pytest.mark.parametrize("name", list(S.CASES))
def test_compensated_gram_stays_inside_its_bound(name):
    r = _restated_case(name)
    ratios = S.check_gram(S.case_problem(name)["X"], r["G"], r["Gx"], r["gram"])
    print(f"\nSETUP-HOST {name} G={ratios['G']:.3f} Gx={ratios['Gx']:.3f}")
    assert ratios["G"] <= 1.0 and ratios["Gx"] <= 1.0
    pad = np.arange(16 * r["G"].shape[0]).reshape(-1, 16) >= S.CASES[name][2]
    assert not r["gram"]["bG"][pad].any() and not r["gram"]["bG"].transpose(0, 2, 1)[pad].any()      # SNP >= p: the bound is zero, the entry exact


@pytest.mark.parametrize("name", MASKED)
def test_restated_gk_stays_inside_its_bounds(name):
    r = _restated_case(name)
    prob = S.case_problem(name)
    ratios, counts = S.check_gk(prob["X"], prob["miss"], r["mcnt4"], r["mobs"], r["q_pad"], r["G"], r["Gx"], r["GK"], r["gram"], r["ref"])
    print(f"\nSETUP-HOST {name} " + " ".join(f"{row}={ratios[row]:.3f}/{counts[row]}" for row in S.GK_ROWS if row in ratios))
    assert counts["copy"] > 0 and counts["indirect"] > 0 and counts["redone"] > 0
    assert (counts["direct"] > 0) == (S.CASES[name][0] == "wide")
    assert all(v <= 1.0 for v in ratios.values()), ratios


def test_plain_running_sum_exceeds_the_gram_bound():
    name = "complete-n4000-p48-q17"
    X = S.case_problem(name)["X"]
    G, Gx = S.plain_gram_f64(X)
    gram = _restated_case(name)["gram"]
    rg, rx = S.worst_ratio(G, gram["G"], gram["bG"]), S.worst_ratio(Gx, gram["Gx"], gram["bGx"])
    print(f"\nSETUP-HOST teeth: plain running sum at n = 4000: G={rg:.1f} Gx={rx:.1f} times the bound")
    assert rg > 1.0 and rx > 1.0


@pytest.mark.parametrize("name", SHORT)
def test_unredone_diagonal_exceeds_the_redone_bound(name):
    r = _restated_case(name)
    prob = S.case_problem(name)
    GK = S.gk_restated_f64(prob["X"], r["midx"], r["mcnt4"], r["mobs"], r["n_pad"], r["G"], r["Gx"], redo=False)
    ratios, counts = S.check_gk(prob["X"], prob["miss"], r["mcnt4"], r["mobs"], r["q_pad"], r["G"], r["Gx"], GK, r["gram"], r["ref"])
    print(f"\nSETUP-HOST teeth: {name} without the redo: redone={ratios['redone']:.1f} times the bound ({counts['redone']} entries)")
    assert ratios["redone"] > 1.0 and ratios["indirect"] <= 1.0
