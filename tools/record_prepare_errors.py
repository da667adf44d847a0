"""Record tests/golden/prepare_errors_parent.json: the error code and the whole aq_last_error() text of every argument error
that the five aq_prepare_data* entries raise before aq_need_device (tests/prep_golden_util.py: error_rows).  No GPU needed.

    AQ_LIB=/path/to/parent/libatlasqtl_hip.so python tools/record_prepare_errors.py OUT.json COMMIT

AQ_LIB names the library that is recorded (default: the one of this checkout); COMMIT is stored in the table.  The table in
tests/golden was recorded from the commit before aq_prepare.hip was split into units; tests/test_prepare_errors_host.py replays
it."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atlasqtl_amd import _lib  # noqa: E402
from tests import prep_golden_util as U  # noqa: E402


def main():
    out, commit = sys.argv[1], sys.argv[2]
    rows = U.error_rows(_lib.lib())
    with open(out, "w") as f:
        f.write('{"parent_commit": %s, "source": "tools/record_prepare_errors.py, on a machine without a HIP device",\n"rows": [\n' % json.dumps(commit))
        f.write(",\n".join(json.dumps(r) for r in rows))
        f.write("\n]}\n")
    print("recorded", len(rows), "rows;", sum(1 for r in rows if (r[2], r[3]) == U.NO_DEVICE), "reach aq_need_device")
    return 0


if __name__ == "__main__":
    sys.exit(main())
