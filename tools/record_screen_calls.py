"""Record a golden table of tests/golden, with no GPU: every library call the screen family's Python makes, with its
arguments, and everything it returns, on the stub library and the cases of a helper module under tests/.

    python tools/record_screen_calls.py OUT.json COMMIT [screen | cis]

Run from a checkout of COMMIT with this file and the helper copied into it (tests/screen_calls_util.py; for `cis`,
tests/cis_calls_util.py as well); COMMIT is stored in the table.
  screen (the default): tests/golden/screen_calls_parent.json, recorded from the commit before prepare.py was split by concern;
    tests/test_screen_calls_host.py replays it.
  cis: tests/golden/cis_calls_parent.json, the three cis entries and their refusals, recorded from the commit before cis.py was
    split by concern; tests/test_cis_calls_host.py replays it."""
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HELPERS = {"screen": "tests.screen_calls_util", "cis": "tests.cis_calls_util"}


def main():
    out, commit = sys.argv[1], sys.argv[2]
    helper = importlib.import_module(HELPERS[sys.argv[3] if len(sys.argv) > 3 else "screen"])
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    table = helper.record()
    with open(out, "w") as f:
        f.write('{"parent_commit": ' + json.dumps(commit) + ', "source": "tools/record_screen_calls.py",\n"cases": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in table.items()))
        f.write("\n}}\n")
    print("recorded", len(table), "cases,", sum(len(v["calls"]) for v in table.values()), "library calls")
    return 0


if __name__ == "__main__":
    sys.exit(main())
