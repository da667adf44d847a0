"""Record tests/golden/prepare_routes_parent.json on the GPU: SHA-256 digests of everything the prepare entries return, per
route from the input to the handle, and of the entries on a finished handle (tests/prep_golden_util.py: route_digests).  One
process, ending at the first entry that fails.

    AQ_LIB=/path/to/parent/libatlasqtl_hip.so python tools/record_prepare_routes.py OUT.json COMMIT

AQ_LIB names the library that is recorded (default: the one of this checkout); COMMIT is stored in the table.  The table in
tests/golden was recorded from the commit before aq_prepare.hip was split into units; tests/test_gpu_prepare_routes.py replays
it."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from atlasqtl_amd import _lib  # noqa: E402
from tests import prep_golden_util as U  # noqa: E402


def main():
    out, commit = sys.argv[1], sys.argv[2]
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    table = U.route_digests(_lib.lib())
    head = dict(parent_commit=commit, source="tools/record_prepare_routes.py", device=torch.cuda.get_device_properties(0).name)
    with open(out, "w") as f:
        f.write("{" + ", ".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(head.items())) + ',\n"routes": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in table.items()))
        f.write("\n}}\n")
    print("recorded", len(table), "routes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
