"""Host: ranks.RankGroup and postproc.fdr_cutoff over three gloo processes on CPU tensors -- no device, no shared library.
One spawn serves all tests of the file: every rank writes what each collective returned to it, the tests compare that
with numpy on the per-rank inputs and with the oracle's assign_bFDR on the whole matrix."""
import os

import numpy as np
import pytest

from tests.util import gloo_rank, spawn_ranks

WORLD = 3
CUTS = [0, 16, 32, 50]
THRES = (1e-9, 0.002, 0.02, 0.05, 0.2, 0.6, 0.9999)
ROW_LENGTHS = {"some": (0, 3, 1), "none": (0, 0, 0)}
ORDERED = (1e16, 1.0, -1e16)            # left to right: 0.0; any order that cancels the large terms first: 1.0


def _sum_inputs(rank):
    rng = np.random.default_rng(100 + rank)
    return {"i5": rng.integers(-2**40, 2**40, size=5, dtype=np.int64),
            "i3x256": rng.integers(0, 2**50, size=(3, 256), dtype=np.int64),
            "f4": rng.integers(-2**20, 2**20, size=4) / 1024.0}       # dyadic: their sum is exact in whatever order


def _rows(rank, lengths):
    """A (m, 4) table as VbRun.associations sends it: two index columns (up to 2^31 - 1) and two doubles."""
    m = lengths[rank]
    rng = np.random.default_rng(7 + rank)
    rows = np.column_stack([rng.integers(0, 2**31, size=m), rng.integers(0, 2**31, size=m), rng.random(m),
                            rng.normal(size=m)]).astype(np.float64).reshape(m, 4)
    if m:
        rows[0, 0] = rows[-1, 1] = 2**31 - 1
    return rows


def _fdr_matrix(ties):
    from tests.test_gpu_postproc import _fdr_ppi
    return _fdr_ppi(ties, 57, 50)


def _shard_query(shard):
    """aq_vb_bfdr_query (include/atlasqtl_hip.h) served by numpy from one shard: the keys in decreasing order, the running
    sum of 1 - key along them; for a value c
      { #{ppi >= c}, sum(1 - ppi : ppi >= c), #{ppi > c}, sum(1 - ppi : ppi > c), largest ppi < c (or -1) }."""
    desc = np.sort(shard.reshape(-1, order="F"))[::-1]
    run = np.concatenate([[0.0], np.cumsum(1.0 - desc)])

    def query(c):
        n_ge = int(np.searchsorted(-desc, -c, side="right"))
        n_gt = int(np.searchsorted(-desc, -c, side="left"))
        return [n_ge, run[n_ge], n_gt, run[n_gt], desc[n_ge] if n_ge < desc.size else -1.0]
    return query


def _worker(rank, world, port, outdir):
    dist = gloo_rank(rank, world, port)
    from atlasqtl_amd.postproc import fdr_cutoff
    from atlasqtl_amd.ranks import RankGroup
    ranks = RankGroup(dist.group.WORLD, 0)
    out = {"rank_world": np.array([ranks.rank, ranks.world])}
    for k, a in _sum_inputs(rank).items():
        keep = a.copy()
        out["sum_" + k] = ranks.sum(a)
        assert np.array_equal(a, keep)                         # the caller's array is not the reduction buffer
    out["max"] = np.array([ranks.max(-1.0)])
    out["ordered"] = np.array([ranks.sum_in_rank_order(ORDERED[rank])])
    for name, lengths in ROW_LENGTHS.items():
        for r, tab in enumerate(ranks.gather_rows(_rows(rank, lengths))):
            out[f"rows_{name}_{r}"] = tab
    for ties in (False, True):
        gam = _fdr_matrix(ties)
        query = _shard_query(gam[:, CUTS[rank]:CUTS[rank + 1]])
        for thres in THRES:
            cut = fdr_cutoff(query, ranks, thres)
            out[f"cut_{int(ties)}_{thres}"] = np.array([-1, -1, -1] if cut is None else cut, dtype=np.int64)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def per_rank(tmp_path_factory):
    outdir = tmp_path_factory.mktemp("ranks")
    spawn_ranks(_worker, WORLD, str(outdir))
    return [dict(np.load(outdir / f"rank{r}.npz")) for r in range(WORLD)]


def test_rank_and_world_are_the_group_s(per_rank):
    for r, got in enumerate(per_rank):
        assert got["rank_world"].tolist() == [r, WORLD]


def test_sum_keeps_shape_and_dtype(per_rank):
    inputs = [_sum_inputs(r) for r in range(WORLD)]
    for k, shape, dtype in (("i5", (5,), np.int64), ("i3x256", (3, 256), np.int64), ("f4", (4,), np.float64)):
        want = np.sum([inp[k] for inp in inputs], axis=0)
        for got in per_rank:
            assert got["sum_" + k].shape == shape and got["sum_" + k].dtype == dtype
            np.testing.assert_array_equal(got["sum_" + k], want)


def test_max_of_negative_values(per_rank):
    for got in per_rank:
        assert got["max"][0] == -1.0


def test_sum_in_rank_order_adds_left_to_right(per_rank):
    for got in per_rank:
        assert got["ordered"][0] == 0.0
        assert got["ordered"].tobytes() == per_rank[0]["ordered"].tobytes()


@pytest.mark.parametrize("name", sorted(ROW_LENGTHS))
def test_gather_rows_returns_every_table_in_rank_order(name, per_rank):
    lengths = ROW_LENGTHS[name]
    for got in per_rank:
        for r in range(WORLD):
            want = _rows(r, lengths)
            tab = got[f"rows_{name}_{r}"]
            assert tab.shape == (lengths[r], 4) and tab.dtype == np.float64
            assert tab.tobytes() == want.tobytes()
            np.testing.assert_array_equal(tab[:, :2].astype(np.int32), want[:, :2].astype(np.int64))   # indices exactly
    if name == "some":
        assert per_rank[0]["rows_some_1"][0, 0] == 2**31 - 1 == per_rank[2]["rows_some_2"][-1, 1]


def test_fdr_cutoff_selects_the_oracle_s_set_on_every_shard(per_rank):
    """For every (matrix, threshold, rank): the first `upto` positions of the shard's stable decreasing order plus `take`
    from `tie_first` are exactly the shard's part of {assign_bFDR(whole matrix) < thres}."""
    from oracle import atlasqtl_oracle as O
    nothing = everything = split_ties = 0
    for ties in (False, True):
        gam = _fdr_matrix(ties)
        fdr = O.assign_bFDR(gam)
        for thres in THRES:
            cuts = [tuple(int(v) for v in got[f"cut_{int(ties)}_{thres}"]) for got in per_rank]
            empty = [c == (-1, -1, -1) for c in cuts]
            assert all(empty) or not any(empty)                 # None on one rank is None on all
            takes = []
            for r, (upto, tie_first, take) in enumerate(cuts):
                k0, k1 = CUTS[r], CUTS[r + 1]
                order = np.argsort(-gam[:, k0:k1].reshape(-1, order="F"), kind="stable")
                chosen = [] if empty[r] else np.concatenate([order[:upto], order[tie_first:tie_first + take]])
                want = np.flatnonzero(fdr[:, k0:k1].reshape(-1, order="F") < thres)
                print(f"ties {ties} thres {thres} rank {r}: upto {upto} tie_first {tie_first} take {take}, {want.size} qualify")
                assert len(chosen) == len(set(chosen)) == want.size
                np.testing.assert_array_equal(np.sort(chosen), want)
                takes.append(0 if empty[r] else take)
            n_in = int((fdr < thres).sum())
            nothing += n_in == 0
            everything += n_in == gam.size
            split_ties += all(t > 0 for t in takes)
    assert nothing >= 2 and everything >= 2 and split_ties >= 1
