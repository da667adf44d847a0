"""The argument errors of the five aq_prepare_data* entries, on the CPU: tests/golden/prepare_errors_parent.json -- the error
code and the whole aq_last_error() text of every error raised before aq_need_device, through every entry that can reach it,
recorded by tools/record_prepare_errors.py from the commit before aq_prepare.hip was split into units (its "parent_commit") --
reproduces row by row.  The cases are those of tests/prep_golden_util.py; every one names device -1, so none reaches a device."""
import json
import os
import re

from tests import prep_golden_util as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prepare_errors_parent.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_table_covers_the_cases():
    doc = _golden()
    rows = doc["rows"]
    assert re.fullmatch(r"[0-9a-f]{40}", doc["parent_commit"]) and doc["source"]
    assert {r[0] for r in rows} == {"aq_prepare_data", "aq_prepare_data_cov", "aq_prepare_data_bed", "aq_prepare_data_bed_cov",
                                    "aq_prepare_data_opt"}
    assert len({(r[0], r[1]) for r in rows}) == len(rows) >= 300
    text = "\n".join(sorted({r[3] for r in rows}))
    for prefix in ("aq_prepare_data: ", "aq_prepare_data_cov: ", "aq_prepare_data_opt: ", "aq_prepare_data_bed: ", "aq_prepare_data_bed_cov: "):
        assert ("\n" + prefix) in ("\n" + text), prefix
    for part in ("NULL argument", "n >= 2, p >= 1, q >= 1 required", "NULL data pointer", "rows asked of a file with n_file", "sample_idx is NULL",
                 "is out of range [0, 6)", "count_a2 and missing must be 0 or 1", "unknown transform of Y", "the offset c must lie in [0, 1/2]",
                 "exceeds the largest supported sample count", "NULL covariate pointer", "between 1 and 96 columns are supported, 97 given",
                 "columns and the intercept need more than", "covariates must be a numeric matrix", "is collinear with the intercept",
                 "exactly one of in and bed must be non-NULL"):
        assert part in text, part
    reached = [r for r in rows if (r[2], r[3]) == U.NO_DEVICE]
    assert len(reached) >= 20 and any("cov:d_0" in r[1] for r in reached)      # the cases that pass every check end in aq_need_device
    assert all(r[2] == 1 for r in rows if r not in reached)


def test_every_parent_error_reproduces(hiplib):
    """rc and the whole message, not a substring.  Where a device is visible, aq_need_device refuses device -1 instead of
    reporting that there is none: the one difference a machine can make."""
    reach = U.BAD_DEVICE if hiplib.aq_device_count() > 0 else U.NO_DEVICE
    want = [r[:2] + list(reach) if (r[2], r[3]) == U.NO_DEVICE else r for r in _golden()["rows"]]
    got = U.error_rows(hiplib)
    assert [r[:2] for r in got] == [r[:2] for r in want]
    bad = [(w, g[2:]) for w, g in zip(want, got) if w != g]
    assert not bad, (len(bad), bad[:5])
