"""GPU: every instance of the two fallback sweep kernels against the CPU oracle (which works in Gram space, so its cost does
not grow with n).

  * the generic wave-per-trait kernel (aq_trait_wave.h, core_kernel == 2): what a handle gets by default when a trait of Y
    misses more than AQ_MIS_MMAX samples at n <= 10 240.  aq_launch_tw compiles it once per (NE, WPT) -- NE samples per lane,
    WPT waves per trait, n_pad = 64 NE WPT -- and stages the SNP columns ns = 4, 2 or 1 at a time;
  * the masked two-barrier MFMA kernel (aq_core_sweep_mis.h, core_kernel == 3): the default when the per-trait Gram blocks of
    the look-ahead MASK instances do not fit.  NT in {1, 2, 4, 8, 16} residual tiles per wave, C = 1 ... 8 sample parts with a
    flag-based exchange, chained SNP segments at C = 1, LDS index lists of up to AQ_MIS_MMAX samples.

Both redo by other means the update of src/coreLoop.cpp:91-138; a wrong lane mapping, a staging loop wrong for one ns, a
part's partial S added twice would show only in the numbers.  The families:
  G1  every compiled generic instance, forced with AQ_KERNEL = 2 (and AQ_TW_WPT), complete Y and 8 % NA, and the ends of the
      natural n ranges;
  G2  the generic kernel as planned, no hook set: a trait with AQ_MIS_MMAX + 1 missing samples, and 40 % NA; and the other
      side of that border, where the look-ahead MASK instances serve;
  G3  two runs of (40, 4) are bit-identical;
  M1  every (NT, C) of the masked kernel, 5 % NA and a single NaN;
  M2  whole runs at the corners of that grid;
  M3  chained segments at every NT;
  M4  a full index list (AQ_MIS_MMAX), an empty one and a list of one in the same trait tile;
  M5  the masked kernel as planned when the Gram blocks do not fit;
  M6  two runs of (8, 8) are bit-identical.
Every case first asserts from aq_vb_get_status that the handle launches the instance the case was written for -- a plan that
lands elsewhere fails -- and then holds the run to the parity bars of tests/test_gpu_split_instances.py::_check.

aq_vb_status reports only n_pad for the generic kernel, and three instances share n_pad = 1024:
tests/test_fallback_coverage_host.py proves (NE, WPT, ns) of every G row from the planner itself, checks every row against
aq_plan_query, and holds the tables to the instances the library compiles (aq_instance_query)."""
import functools

import numpy as np
import pytest

from tests import test_gpu_split_instances as T

pytestmark = pytest.mark.gpu

MASK = T.MASK
SHORT, WHOLE = T.SHORT, T.WHOLE
MIS_MMAX = T.MIS_MMAX            # AQ_MIS_MMAX
N_FALLBACK = 10240               # AQ_KERNEL >= 2 is refused beyond it: only the look-ahead kernel serves a larger n
P, Q = 70, 33                    # five SNP blocks, the last of six SNPs; three trait tiles, one live trait in the last

# --- G1. every compiled generic instance at n = 64 NE WPT - 7 (the last 64-sample slice ragged), complete Y and 8 % NA, SHORT:
#         (NE, WPT, n, AQ_TW_WPT or None, n_pad, ns)
TW_NA = 0.08
TW_FORCED = [
    (4, 1, 249, None, 256, 4), (8, 1, 505, None, 512, 4), (16, 1, 1017, None, 1024, 4), (32, 1, 2041, None, 2048, 4),
    (4, 2, 505, 2, 512, 4), (8, 2, 1017, 2, 1024, 4), (16, 2, 2041, 2, 2048, 4),
    (32, 2, 4089, None, 4096, 4), (40, 2, 5113, None, 5120, 2),
    (4, 4, 1017, 4, 1024, 4), (8, 4, 2041, 4, 2048, 4), (16, 4, 4089, 4, 4096, 4),
    (32, 4, 8185, None, 8192, 2), (40, 4, 10233, None, 10240, 1),
]
# ... and the ends of the natural ranges, complete Y, SHORT: the first n of an instance (the most padding: whole lanes and
# waves hold none of the samples) and n without any padding
TW_ENDS = [
    (32, 2, 2049, None, 4096, 4), (40, 2, 4097, None, 5120, 2), (32, 4, 5121, None, 8192, 2), (40, 4, 8193, None, 10240, 1),
    (32, 1, 2048, None, 2048, 4), (40, 2, 5120, None, 5120, 2), (40, 4, 10240, None, 10240, 1),
]

# --- G2. the generic kernel as planned, no hook: 5 % NA and one trait with AQ_MIS_MMAX + 1 missing samples, WHOLE:
#         n -> (NE, WPT, n_pad, ns)
TW_NATURAL_NA = 0.05
TW_NATURAL_TRAIT = 5
TW_NATURAL = {1500: (32, 1, 2048, 4), 3000: (32, 2, 4096, 4), 5000: (40, 2, 5120, 2), 5121: (32, 4, 8192, 2), 10240: (40, 4, 10240, 1)}
TW_BORDER_N = 3000               # ... the same problem with AQ_MIS_MMAX missing: the look-ahead MASK instances
TW_DENSE = (10240, 40, 17, 0.40, (40, 4, 10240, 1))     # 40 % NA everywhere: (n, p, q, na, instance)

# --- G3. determinism
TW_TWICE = (40, 4, 10233, None, 10240, 1)

# --- M1. every (NT, C) of the masked kernel, AQ_KERNEL = 3 and AQ_MIS_C = C at n = 128 NT C - 5, SHORT, for 5 % NA and for a
#         single NaN (Y[3, 1]; every index list but one is empty).  All 40 pairs can be planned: AQ_MIS_C takes the smallest NT
#         with 128 NT C >= n.  For (16, 6 ... 8) n = 128 NT C - 5 is beyond the kernel's n, so they run at the largest ragged
#         n, 10 235 (mis_n): n_pad = 12 288, 14 336 and 16 384, the last sample parts -- three of the eight at C = 8 --
#         hold nothing but padding.  No hook-free plan picks them: (16, 5) always fits and is found first.
MIS_NT = (1, 2, 4, 8, 16)
MIS_NA = 0.05
MIS_GRID = [(nt, c) for nt in MIS_NT for c in range(1, 9)]
MIS_ONE_NAN = (3, 1)

# --- M2. whole runs at the corners; (16, 5) is the largest pair in which every part holds samples
MIS_WHOLE = [(1, 1), (16, 1), (1, 8), (8, 8), (16, 5), (16, 8)]

# --- M3. chained segments, C = 1, p = 100 (seven SNP blocks): uneven segments, and one block per segment
CHAIN_P = 100
CHAIN_S = (2, 3, 7)

# --- M4. the index lists at their limits: (n, C, NT); in the first trait tile trait 2 misses AQ_MIS_MMAX samples (the LDS
#         list is full), trait 7 none, trait 11 exactly one; the rest 5 %.  WHOLE
LISTS = [(2043, 1, 16), (1500, 3, 4)]
LIST_FULL, LIST_EMPTY, LIST_ONE = 2, 7, 11

# --- M5. the masked kernel as planned on 256 CUs when the Gram blocks do not fit (AQ_GK_MAX_GB), 5 % NA, WHOLE: n -> (C, NT)
MIS_NATURAL = {1100: (5, 2), 2500: (5, 4), 5200: (6, 8), 10240: (5, 16)}
GK_MAX_GB = "0.000001"

# --- M6. determinism
MIS_TWICE = (8, 8)


def tw_ns(n_pad):
    """SNP columns staged at a time (aq_plan_tw): ns n_pad doubles next to 8 x 256 + 32 of block scalars within 150 KB."""
    ns = 4
    while ns > 1 and (ns * n_pad + 8 * 256 + 32) * 8 > 150 * 1024:
        ns //= 2
    return ns


def ledger():
    """What the tables above claim to reach: (generic instances as (NE, WPT, na > 0), the ns values, the masked (NT, C), the
    chained (NT, segments))."""
    generic, ns, masked, chained = set(), set(), set(), set()
    for ne, wpt, n, hook, n_pad, s in TW_FORCED:
        generic |= {(ne, wpt, False), (ne, wpt, True)}
        ns.add(s)
    for ne, wpt, n, hook, n_pad, s in TW_ENDS:
        generic.add((ne, wpt, False))
        ns.add(s)
    for n, (ne, wpt, n_pad, s) in TW_NATURAL.items():
        generic.add((ne, wpt, True))
        ns.add(s)
    ne, wpt, n_pad, s = TW_DENSE[4]
    generic.add((ne, wpt, True))
    ns.add(s)
    generic.add(TW_TWICE[:2] + (True,))
    masked |= set(MIS_GRID) | set(MIS_WHOLE) | {MIS_TWICE}
    masked |= {(nt, c) for n, c, nt in LISTS} | {(nt, c) for c, nt in MIS_NATURAL.values()}
    for nt in MIS_NT:
        masked.add((nt, 1))
        chained |= {(nt, s) for s in CHAIN_S}
    return generic, ns, masked, chained


# ------------------------------------------------------------------------------------------------------------------------------
# the problems (plain NumPy: tests/test_fallback_coverage_host.py builds the same ones for their missingness counts)

def _recentre(Y, k):
    Y[:, k] -= np.nanmean(Y[:, k])


def _set_missing(Y, k, m, rng):
    """Exactly m missing samples in trait k: NaNs are added to, or filled in from N(0, 1) at, rows drawn by rng; re-centred
    over the observed rows."""
    nan = np.isnan(Y[:, k])
    have = int(nan.sum())
    if have < m:
        Y[rng.choice(np.flatnonzero(~nan), size=m - have, replace=False), k] = np.nan
    elif have > m:
        rows = rng.choice(np.flatnonzero(nan), size=have - m, replace=False)
        Y[rows, k] = rng.normal(size=rows.size)
    _recentre(Y, k)
    assert int(np.isnan(Y[:, k]).sum()) == m


@functools.lru_cache(maxsize=4)
def problem(kind, n, p=P, q=Q, na=0.0, arg=0):
    """kind "plain": make_problem with a fraction na of NA; "one_nan": complete Y with the single NaN MIS_ONE_NAN; "trait":
    NA as given and trait TW_NATURAL_TRAIT with exactly arg missing samples; "lists": the three traits of family M4."""
    prob = T._problem(n, p, q, na)
    if kind == "plain":
        return prob
    Y = prob["Y"].copy()
    rng = np.random.default_rng(7)
    if kind == "one_nan":
        assert not np.isnan(Y).any()
        Y[MIS_ONE_NAN] = np.nan
        _recentre(Y, MIS_ONE_NAN[1])
    elif kind == "trait":
        _set_missing(Y, TW_NATURAL_TRAIT, arg, rng)
    elif kind == "lists":
        _set_missing(Y, LIST_FULL, MIS_MMAX, rng)
        _set_missing(Y, LIST_EMPTY, 0, rng)
        _set_missing(Y, LIST_ONE, 1, rng)
    else:
        raise ValueError(kind)
    prob = dict(prob)
    prob["Y"] = Y
    return prob


def missing_of(prob):
    """(max_missing, max_short_list) as aq_vb_create counts them."""
    m = np.isnan(prob["Y"]).sum(axis=0)
    return int(m.max()), int(np.minimum(m, prob["Y"].shape[0] - m).max())


def mis_n(nt, c):
    """n of a masked case: the last sample tile ragged (11 of 16), and within the n the kernel serves."""
    return min(128 * nt * c, N_FALLBACK) - 5


def tw_hooks(hook):
    return {"AQ_KERNEL": 2, **({"AQ_TW_WPT": hook} if hook else {})}


def mis_hooks(c, chain=None):
    return {"AQ_KERNEL": 3, "AQ_MIS_C": c, **({"AQ_CHAIN": chain} if chain else {})}


def _setenv(monkeypatch, hooks):
    for k, v in hooks.items():
        monkeypatch.setenv(k, str(v))


@functools.lru_cache(maxsize=4)
def _reference(key, maxit):
    """The oracle's run of problem(*key), shared by the cases that run the same problem on different instances."""
    return T._reference(problem(*key), maxit)


def _assert_generic(run, ne, wpt, natural=False):
    st = run.status()
    assert st["core_kernel"] == 2, st
    assert st["n_pad"] == 64 * ne * wpt, f"planned n_pad = {st['n_pad']}, the case is written for (NE, WPT) = {(ne, wpt)}"
    assert (st["tiles_matrix"], st["tiles_matrix2"], st["tiles_recurrence"], st["instance_flags"]) == (0, 0, 0, 0), st
    assert (st["split_parts"], st["tiles_per_group"], st["chain_segments"]) == (1, 1, 0), st
    if natural:
        assert st["overrides"] == "", st["overrides"]
    return st


def _assert_masked(run, nt, c, chain=0):
    st = run.status()
    assert st["core_kernel"] == 3, st
    got = (st["tiles_matrix"], st["split_parts"], st["chain_segments"])
    assert got == (nt, c, chain), f"planned (NT, C, segments) = {got}, the case is written for {(nt, c, chain)}"
    assert (st["tiles_matrix2"], st["tiles_recurrence"], st["instance_flags"], st["tiles_per_group"]) == (0, 0, 0, 1), st
    assert st["n_pad"] == 128 * nt * c
    return st


def _check_generic(family, key, ne, wpt, maxit=SHORT, natural=False):
    return T._check(family, problem(*key), (ne, wpt, natural), maxit=maxit, assert_instance=_assert_generic,
                    reference=_reference(key, maxit))


def _check_masked(family, key, nt, c, chain=0, maxit=SHORT):
    return T._check(family, problem(*key), (nt, c, chain), maxit=maxit, assert_instance=_assert_masked,
                    reference=_reference(key, maxit))


# ------------------------------------------------------------------------------------------------------------------------------
# G1. every compiled generic instance

def _tw_id(row):
    return f"NE{row[0]}-WPT{row[1]}-n{row[2]}"


# (sorted by n: the instances that share a problem -- three at n_pad = 1024 -- share its oracle run)
@pytest.mark.parametrize("na", [0.0, TW_NA])
@pytest.mark.parametrize("row", sorted(TW_FORCED, key=lambda r: r[2]), ids=_tw_id)
def test_generic_every_instance_matches_oracle(row, na, monkeypatch):
    """The 14 instances of aq_launch_tw, each with a ragged last slice, complete Y and 8 % NA: the ladder and two ELBO
    evaluations."""
    ne, wpt, n, hook, n_pad, ns = row
    assert n == 64 * ne * wpt - 7 and n_pad == 64 * ne * wpt and ns == tw_ns(n_pad)
    _setenv(monkeypatch, tw_hooks(hook))
    _check_generic("G1", ("plain", n, P, Q, na), ne, wpt)


@pytest.mark.parametrize("row", TW_ENDS, ids=_tw_id)
def test_generic_range_ends_match_oracle(row, monkeypatch):
    """The first n of (32, 2), (40, 2), (32, 4), (40, 4) -- up to half the lanes hold nothing but padding -- and n = 2048, 5120,
    10 240 with no padding at all; complete Y."""
    ne, wpt, n, hook, n_pad, ns = row
    assert n_pad == 64 * ne * wpt and ns == tw_ns(n_pad)
    _setenv(monkeypatch, tw_hooks(hook))
    _check_generic("G1", ("plain", n, P, Q, 0.0), ne, wpt)


# ------------------------------------------------------------------------------------------------------------------------------
# G2. the generic kernel as planned

@pytest.mark.parametrize("n", sorted(TW_NATURAL))
def test_generic_as_planned_for_one_badly_measured_trait_matches_oracle(n):
    """What a user gets by default when one trait misses AQ_MIS_MMAX + 1 samples (5 % NA elsewhere): whole runs, no hook."""
    ne, wpt, n_pad, ns = TW_NATURAL[n]
    key = ("trait", n, P, Q, TW_NATURAL_NA, MIS_MMAX + 1)
    assert missing_of(problem(*key))[0] == MIS_MMAX + 1
    _check_generic("G2", key, ne, wpt, maxit=WHOLE, natural=True)


def test_look_ahead_mask_serves_the_other_side_of_the_list_border():
    """The same problem with AQ_MIS_MMAX missing samples in that trait: the planner stays with the look-ahead kernel's MASK
    instances, and the run matches the oracle as well."""
    key = ("trait", TW_BORDER_N, P, Q, TW_NATURAL_NA, MIS_MMAX)
    assert missing_of(problem(*key))[0] == MIS_MMAX

    def assert_mask(run):
        st = run.status()
        assert st["overrides"] == "", st["overrides"]
        assert st["core_kernel"] == 0 and st["instance_flags"] & MASK and not st["instance_flags"] & T.WIDE, st

    T._check("G2", problem(*key), (), maxit=WHOLE, assert_instance=assert_mask, reference=_reference(key, WHOLE))


def test_generic_as_planned_for_dense_missingness_matches_oracle():
    """n = 10 240 with 40 % NA in every trait: (40, 4), one SNP column staged at a time, no hook; whole run."""
    n, p, q, na, (ne, wpt, n_pad, ns) = TW_DENSE
    key = ("plain", n, p, q, na)
    assert missing_of(problem(*key))[0] > MIS_MMAX
    _check_generic("G2", key, ne, wpt, maxit=WHOLE, natural=True)


# ------------------------------------------------------------------------------------------------------------------------------
# G3. determinism

def test_generic_is_deterministic(monkeypatch):
    """The partial dots of a trait's four waves meet in LDS and are added in a fixed order: two runs are bit-identical."""
    ne, wpt, n, hook, n_pad, ns = TW_TWICE
    _setenv(monkeypatch, tw_hooks(hook))
    key = ("plain", n, P, Q, TW_NA)
    a = _check_generic("G3", key, ne, wpt)
    b = _check_generic("G3", key, ne, wpt)
    np.testing.assert_array_equal(a["gam_vb"], b["gam_vb"])
    np.testing.assert_array_equal(a["mu_beta_vb"], b["mu_beta_vb"])


# ------------------------------------------------------------------------------------------------------------------------------
# M1. every (NT, C) of the masked kernel

@pytest.mark.parametrize("kind", ["na", "one_nan"])
@pytest.mark.parametrize("nt,c", MIS_GRID, ids=[f"NT{nt}-C{c}" for nt, c in MIS_GRID])
def test_masked_every_instance_and_part_count_matches_oracle(nt, c, kind, monkeypatch):
    """NT x C with a ragged last sample tile: 5 % NA, and a single NaN (all index lists but one are empty): the ladder and two
    ELBO evaluations.  (16, 5 ... 8) share n = 10 235 and its oracle run: with C = 6, 7, 8 whole parts are padding."""
    _setenv(monkeypatch, mis_hooks(c))
    key = ("plain", mis_n(nt, c), P, Q, MIS_NA) if kind == "na" else ("one_nan", mis_n(nt, c), P, Q, 0.0)
    mm = missing_of(problem(*key))[0]
    assert 1 <= mm <= MIS_MMAX, mm      # beyond it the planner rightly leaves this kernel
    if kind == "one_nan":
        assert int(np.isnan(problem(*key)["Y"]).sum()) == 1
    _check_masked("M1", key, nt, c)


# ------------------------------------------------------------------------------------------------------------------------------
# M2. whole runs at the corners

@pytest.mark.parametrize("nt,c", MIS_WHOLE, ids=[f"NT{nt}-C{c}" for nt, c in MIS_WHOLE])
def test_masked_corner_whole_run_matches_oracle(nt, c, monkeypatch):
    _setenv(monkeypatch, mis_hooks(c))
    key = ("plain", mis_n(nt, c), P, Q, MIS_NA)
    assert missing_of(problem(*key))[0] <= MIS_MMAX
    _check_masked("M2", key, nt, c, maxit=WHOLE)


# ------------------------------------------------------------------------------------------------------------------------------
# M3. chained segments at every NT

@pytest.mark.parametrize("chain", CHAIN_S)
@pytest.mark.parametrize("nt", MIS_NT)
def test_masked_chained_segments_every_instance_matches_oracle(nt, chain, monkeypatch):
    """Seven SNP blocks in 2, 3 (uneven) and 7 (one block each) chained segments, unsplit: the ladder and two ELBO evaluations."""
    _setenv(monkeypatch, mis_hooks(1, chain))
    key = ("plain", mis_n(nt, 1), CHAIN_P, Q, MIS_NA)
    assert problem(*key)["p"] == CHAIN_P
    _check_masked("M3", key, nt, 1, chain=chain)


# ------------------------------------------------------------------------------------------------------------------------------
# M4. the index lists at their limits

@pytest.mark.parametrize("n,c,nt", LISTS, ids=[f"n{n}-C{c}" for n, c, nt in LISTS])
def test_masked_full_empty_and_single_index_lists_match_oracle(n, c, nt, monkeypatch):
    """One trait tile holds a list of AQ_MIS_MMAX samples (the LDS list is full), an empty one and a list of one: whole run."""
    _setenv(monkeypatch, mis_hooks(c))
    key = ("lists", n, P, Q, MIS_NA)
    m = np.isnan(problem(*key)["Y"]).sum(axis=0)
    assert (m[LIST_FULL], m[LIST_EMPTY], m[LIST_ONE]) == (MIS_MMAX, 0, 1) and m.max() == MIS_MMAX
    _check_masked("M4", key, nt, c, maxit=WHOLE)


# ------------------------------------------------------------------------------------------------------------------------------
# M5. the masked kernel as planned

@pytest.mark.parametrize("n", sorted(MIS_NATURAL))
def test_masked_as_planned_matches_oracle(n, monkeypatch):
    """What a user gets by default when the per-trait Gram blocks of the MASK instances do not fit: whole runs."""
    monkeypatch.setenv("AQ_GK_MAX_GB", GK_MAX_GB)
    c, nt = MIS_NATURAL[n]
    key = ("plain", n, P, Q, MIS_NA)
    assert missing_of(problem(*key))[0] <= MIS_MMAX
    if T._pin_256_cus(monkeypatch):
        _check_masked("M5", key, nt, c, maxit=WHOLE)
    else:   # fewer CUs than the table assumes: whatever the planner picks must still be the masked kernel

        def assert_kernel(run):
            assert run.status()["core_kernel"] == 3

        T._check("M5", problem(*key), (), maxit=WHOLE, assert_instance=assert_kernel, reference=_reference(key, WHOLE))


# ------------------------------------------------------------------------------------------------------------------------------
# M6. determinism

def test_masked_exchange_is_deterministic(monkeypatch):
    """Every part adds the eight partial S in the same order: two runs are bit-identical."""
    nt, c = MIS_TWICE
    _setenv(monkeypatch, mis_hooks(c))
    key = ("plain", mis_n(nt, c), P, Q, MIS_NA)
    a = _check_masked("M6", key, nt, c)
    b = _check_masked("M6", key, nt, c)
    np.testing.assert_array_equal(a["gam_vb"], b["gam_vb"])
    np.testing.assert_array_equal(a["mu_beta_vb"], b["mu_beta_vb"])
