"""Every route from an input to a prepare handle, and every entry on a finished handle, against the parent commit on the GPU:
tests/golden/prepare_routes_parent.json holds SHA-256 digests of the raw bytes that the library of the commit before
aq_prepare.hip was split into units (its "parent_commit") returned on an MI355X, recorded by tools/record_prepare_routes.py;
the library at hand must return the same bytes.  The split moved host code and changed neither a kernel nor the order of the
launches, and every sum in those kernels is taken in a fixed order, so equality is exact.

Routes (tests/prep_golden_util.py): {dense fp64, dense int8, .bed, .bed with missing genotypes imputed, .bed with a sample
subset} x {no covariates, 2 covariates} x {no transform, rank-based inverse normal}, n = 203 (odd, not a multiple of 16: lead,
full vectors and tail in every column of the decode; the unaligned kernel instances), p = 37 (not a multiple of the decode's 4
variants per workgroup), q = 3, with constant, duplicated and covariate-absorbed columns and 10 % NaN in Y; the int8 and .bed
routes again at n = 204 (the aligned instances).  On the plain int8 and .bed handles also aq_prep_grm, aq_prep_grm_apply at two
padded widths, aq_prep_ld_band, aq_prep_ld_prune with aq_prep_ld_info and the pruned X; and aq_rank_int on the same Y."""
import json
import os
import re

import pytest

from tests import prep_golden_util as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prepare_routes_parent.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_table_covers_the_routes():
    doc = _golden()
    routes = doc["routes"]
    assert re.fullmatch(r"[0-9a-f]{40}", doc["parent_commit"]) and doc["source"] and doc["device"]
    want = {f"n203/{s}/cov{d}/yt{m}" for s in ("f64", "i8", "bed", "bed_missing", "bed_subset") for d in (0, 2) for m in (0, 1)}
    want |= {"n204/i8/cov0/yt0", "n204/bed/cov0/yt0", "n203/aq_rank_int", "n204/aq_rank_int"}
    assert set(routes) == want
    for name, r in routes.items():
        if "/cov" not in name:
            continue
        assert 1 <= r["p_kept"] <= U.P - 3 and r["n_cov"] == int(name.split("/cov")[1][0]) and r["yt_method"] == int(name[-1])
        assert r["n_absorbed"] == (1 if r["n_cov"] else 0)
        assert r["genotype_counts_rc"] == (0 if "/bed" in name else 1)
        if name.endswith(("/i8/cov0/yt0", "/bed/cov0/yt0")):
            assert 1 <= r["ld_p_kept"] < r["p_kept"] and {"grm", "grm_trace", "grm_apply_5", "grm_apply_17", "ld_band", "ld_X"} <= set(r)
    assert routes["n203/i8/cov0/yt0"]["X"] == routes["n203/bed/cov0/yt0"]["X"] != routes["n203/f64/cov0/yt0"]["X"]
    assert routes["n203/bed_missing/cov0/yt0"]["X"] != routes["n203/bed/cov0/yt0"]["X"]
    assert routes["n203/i8/cov0/yt0"]["Y"] != routes["n203/i8/cov0/yt1"]["Y"] != routes["n203/i8/cov2/yt1"]["Y"]


@pytest.mark.gpu
def test_every_route_returns_the_bytes_of_the_parent(hiplib):
    want = _golden()["routes"]
    got = U.route_digests(hiplib)
    assert set(got) == set(want)
    bad = [(name, key, want[name].get(key), got[name].get(key)) for name in want for key in sorted(set(want[name]) | set(got[name]))
           if want[name].get(key) != got[name].get(key)]
    assert not bad, (len(bad), bad[:8])
