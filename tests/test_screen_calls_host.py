"""Host: the screen family's Python hands the library the calls, and returns the results, that the commit before the split of
prepare.py did -- tests/golden/screen_calls_parent.json, recorded there by tools/record_screen_calls.py on the stub library of
tests/screen_calls_util.py (no GPU, no shared object), replayed here.  Exact: the sequence of library calls with every
argument, and every whole number, key, dtype and shape of what comes back.  Real numbers to 1e-12 relative: t, p-values,
q-values, cutoffs and beta shapes pass through scipy, whose libm may differ from the recording machine's; any change of formula
moves them by orders of magnitude more."""
import json
import os

import pytest

from tests import screen_calls_util as U

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "screen_calls_parent.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def replayed():
    return json.loads(json.dumps(U.record()))


def test_the_recording_covers_the_family():
    assert len(GOLDEN["parent_commit"]) == 40 and len(GOLDEN["cases"]) >= 45
    entries = {call[0] for case in GOLDEN["cases"].values() for call in case["calls"]}
    assert entries == {"aq_prep_marginal", "aq_prep_marginal_perm", "aq_prep_cis", "aq_prep_cis_perm", "aq_prep_cis_cond",
                       "aq_prep_cis_int", "aq_prep_destroy", "aq_last_error", "aq_rank_int", "aq_prep_ld_prune"}
    calls = {name: [call[0] for call in case["calls"]] for name, case in GOLDEN["cases"].items()}
    assert calls["screen_handle/second_call"] == ["aq_prep_marginal"] * 2 and calls["cis_handle/second_call"] == ["aq_prep_cis"] * 2
    assert calls["cis_handle/condition_on/k_eff_below"] == ["aq_prep_cis_cond"] * 2          # the re-cut with the k_eff reported
    assert calls["cis_handle/condition_on/second_call"] == ["aq_prep_cis_cond"] * 3
    assert calls["cis_independent_handle"] == ["aq_prep_cis", "aq_prep_cis_perm"] + ["aq_prep_cis_cond"] * 3   # forward, backward x 2
    assert GOLDEN["cases"]["rank_normalize/code1"]["result"]["dict"]["raises"] == "AtlasqtlError"
    assert GOLDEN["cases"]["rank_normalize/code2"]["result"]["dict"]["raises"] == "AtlasqtlHipError"


def test_the_same_cases_are_replayed(replayed):
    assert list(replayed) == list(GOLDEN["cases"])


@pytest.mark.parametrize("name", list(GOLDEN["cases"]))
def test_calls_and_results_are_the_parents(replayed, name):
    diff = U.differences(GOLDEN["cases"][name], replayed[name], name)
    assert not diff, "\n".join(diff[:20])
