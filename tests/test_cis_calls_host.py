"""Host: cis_screen(), cis_independent() and cis_finemap(), and the handle-level functions under them, hand the library the
calls, return the results and refuse with the texts that the commit before the split of cis.py did --
tests/golden/cis_calls_parent.json, recorded there by tools/record_screen_calls.py (table `cis`) on the stub library and the
stubbed preparation of tests/cis_calls_util.py (no GPU, no shared object), replayed here.  Exact: the sequence of library calls
with every argument, how often the preparation ran, every error text, and every whole number, key, dtype and shape of what
comes back.  Real numbers to 1e-12 relative, for the reason tests/test_screen_calls_host.py gives."""
import json
import os

import pytest

from tests import cis_calls_util as CU
from tests import screen_calls_util as U

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cis_calls_parent.json")) as f:
    GOLDEN = json.load(f)
CASES = GOLDEN["cases"]


@pytest.fixture(scope="module")
def replayed():
    return json.loads(json.dumps(CU.record()))


def _entries(name):
    return [call[0] for call in CASES[name]["calls"]]


def _text(name):
    return CASES[name]["result"]["dict"]["text"]


def test_the_recording_covers_the_three_entries():
    assert len(GOLDEN["parent_commit"]) == 40 and len(CASES) >= 250
    assert {call[0] for case in CASES.values() for call in case["calls"]} == {
        "aq_prep_cis", "aq_prep_cis_perm", "aq_prep_cis_cond", "aq_prep_cis_int", "aq_prep_cis_finemap", "aq_prep_set_purity",
        "aq_prep_destroy", "aq_last_error"}
    # the two-call protocol at each of its sites, the re-cut with the k_eff reported before it
    assert _entries("cis_finemap_handle/second_call") == ["aq_prep_cis_finemap"] * 2 + ["aq_prep_set_purity"]
    assert _entries("cis_finemap_handle/max_rows/too_small") == ["aq_prep_cis_finemap"] and "max_rows = 4" in _text("cis_finemap_handle/max_rows/too_small")
    assert _entries("cis_screen/second_call") == ["aq_prep_cis"] * 2 + ["aq_prep_destroy"]
    assert _entries("cis_screen/condition_on/k_eff_below") == ["aq_prep_cis_cond"] * 3 + ["aq_prep_destroy"]
    assert _entries("cis_screen/interaction/second_call") == ["aq_prep_cis_int"] * 2 + ["aq_prep_destroy"]
    assert _entries("cis_independent") == ["aq_prep_cis", "aq_prep_cis_perm"] + ["aq_prep_cis_cond"] * 3 + ["aq_prep_destroy"]
    # the fine-mapping takes every branch: the duplicate of trait 0's set and its effect with V = 0 are gone, trait 2's second
    # set is impure
    fm = CASES["cis_finemap"]["result"]["dict"]
    assert fm["n_impure"] == 1 and fm["n_cs"]["values"] == [1, 0, 1] and fm["cs"]["dict"]["cs"]["values"] == [0, 0, 0]
    assert fm["window"][0]["values"] == U.LO and fm["window"][1]["values"] == U.HI        # from the kept columns' coordinates
    assert CASES["cis_finemap"]["prepared"] == 1 and all(CASES[k]["prepared"] == 0 for k in CASES if "_handle/" in k)


def test_what_is_refused_before_anything_is_prepared_or_computed():
    """The refusals are as early as the parent's were: the recording says which ran neither the preparation nor a library
    entry, and the replay below holds every case to its record.  cis_independent() is the one entry that learns of a bad
    window only from cis_windows, on the prepared handle."""
    refused = [k for k in CASES if k.startswith("refused/")]
    assert len(refused) >= 200 and all(CASES[k]["result"]["dict"]["raises"] == "AtlasqtlError" for k in refused)
    early = {k for k in refused if CASES[k]["prepared"] == 0 and CASES[k]["calls"] == []}
    late = set(refused) - early
    assert all(CASES[k]["prepared"] == 1 and _entries(k) == ["aq_prep_destroy"] for k in late)
    assert all(k in early for k in refused if "_handle/" in k or ("/window/" in k and "cis_independent" not in k))
    assert all(f"refused/cis_independent/window/{i}" in late and _text(f"refused/cis_independent/window/{i}").startswith("cis_windows:")
               for i in range(4))
    for group in ("no_coordinates", "snp_pos_length", "both", "max_signals_six", "permutations_none", "condition_on_permutations",
                  "interaction_permutations", "interaction_condition_on", "missing_y/condition_on", "missing_y/interaction",
                  "interaction/constant", "interaction/inside_the_span", "interaction/covariates_rank"):
        hit = [k for k in refused if k.endswith("/" + group) and "_handle/" not in k]
        assert hit and set(hit) <= early, group
    # the lists of condition_on= and the trait count need the kept names: after the preparation, before any scan
    assert all(k in late for k in refused if k.startswith("refused/cis_screen/condition_on/") or k.endswith("/trait_count"))
    # the permutation messages of the cis entries speak of marginal_screen
    assert _text("refused/cis_screen/permutations_zero").startswith("marginal_screen:")


def test_the_same_cases_are_replayed(replayed):
    assert list(replayed) == list(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_calls_results_and_refusals_are_the_parents(replayed, name):
    diff = U.differences(CASES[name], replayed[name], name)
    assert not diff, "\n".join(diff[:20])
