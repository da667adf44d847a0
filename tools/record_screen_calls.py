"""Record tests/golden/screen_calls_parent.json, with no GPU: every library call the screen family's Python makes, with its
arguments, and everything it returns, on the stub library and the cases of tests/screen_calls_util.py.

    python tools/record_screen_calls.py OUT.json COMMIT

Run from a checkout of COMMIT with this file and tests/screen_calls_util.py copied into it; COMMIT is stored in the table.  The
table in tests/golden was recorded from the commit before prepare.py was split by concern;
tests/test_screen_calls_host.py replays it."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import screen_calls_util as U  # noqa: E402


def main():
    out, commit = sys.argv[1], sys.argv[2]
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    table = U.record()
    with open(out, "w") as f:
        f.write('{"parent_commit": ' + json.dumps(commit) + ', "source": "tools/record_screen_calls.py",\n"cases": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in table.items()))
        f.write("\n}}\n")
    print("recorded", len(table), "cases,", sum(len(v["calls"]) for v in table.values()), "library calls")
    return 0


if __name__ == "__main__":
    sys.exit(main())
