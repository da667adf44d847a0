"""Record the launch-plan table tests/golden/plan_table_parent.json from live handles on the GPU.

One VbRun per case of the grid below (the handle is created, no sweep runs): aq_vb_get_status, aq_vb_get_overrides, or the
error code and text where aq_vb_create refuses; plus the device's CU count and total memory.  One process, ending at the first
unexpected failure.  tests/test_plan_host.py replays the table through aq_plan_query on the CPU.

    python tools/record_plan_table.py OUT.json COMMIT [TREE]

COMMIT is stored in the table; TREE (default: this checkout) is the built checkout whose atlasqtl_amd is imported -- the table
in tests/golden was recorded from the commit before the planner moved into atlasqtl_amd/csrc/aq_plan.h."""
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, sys.argv[3] if len(sys.argv) > 3 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from atlasqtl_amd._lib import AtlasqtlHipError  # noqa: E402
from atlasqtl_amd.core import VbRun  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else "plan_table.json"
COMMIT = sys.argv[2] if len(sys.argv) > 2 else "unknown"
PLAN_KEYS = ("core_kernel", "split_parts", "tiles_per_group", "chain_segments", "tiles_matrix", "tiles_matrix2", "tiles_recurrence",
             "instance_flags", "n_pad")
N_LIST = [2, 16, 17, 500, 800, 900, 1000, 1056, 1057, 1500, 2048, 2049, 5000, 5120, 8448, 8449, 10240, 10241, 16384, 16385, 20480,
          50000, 82943, 82944]
N_NA = [16, 17, 500, 900, 1000, 1056, 1057, 1500, 2048, 2049, 5000, 8448, 8449, 10240, 10241, 16384, 16385, 20480, 50000, 82944]
Q_LIST = [3, 17, 33, 1030, 2500, 5000, 7168, 10000]


def cases():
    c = []
    for i, n in enumerate(N_LIST):
        c.append(dict(n=n, p=16 + 8 * (i % 9), q=17, na="none", env={}))
    c.append(dict(n=82945, p=16, q=17, na="none", env={}))
    for i, n in enumerate(N_NA):
        c.append(dict(n=n, p=16 + 8 * (i % 9), q=17, na="5pct", env={}))
    for n in (2000, 5000, 10240, 16384):                      # one trait misses more than AQ_MIS_MMAX = 1024 samples
        c.append(dict(n=n, p=24, q=17, na="heavy", env={}))
        c.append(dict(n=n, p=24, q=17, na="heavy", env={"AQ_KERNEL": "3"}))
    for n in (12000, 30000):                                  # ... and one misses more than it has (the observed list is shorter)
        c.append(dict(n=n, p=24, q=17, na="mostly", env={}))
    for ncu in (None, 8, 64, 256):
        env = {} if ncu is None else {"AQ_NCU": str(ncu)}
        for q in Q_LIST:
            for n, na in ((1000, "none"), (1000, "5pct"), (800, "none")):
                c.append(dict(n=n, p=48, q=q, na=na, env=dict(env)))
        for q in (17, 1030, 5000):
            for n, na in ((1500, "none"), (5000, "none"), (3000, "5pct"), (12000, "none")):
                c.append(dict(n=n, p=48, q=q, na=na, env=dict(env)))
            for n, na, k in ((1500, "5pct", "3"), (3000, "none", "3"), (3000, "5pct", "2"), (12000, "5pct", "2")):
                c.append(dict(n=n, p=48, q=q, na=na, env=dict(env, AQ_KERNEL=k)))
    hooks = [("AQ_KERNEL", v) for v in (2, 3)] + [("AQ_TT", v) for v in (1, 2)] + [("AQ_NT3", v) for v in (0, 3, 6, 9)]
    hooks += [("AQ_CHAIN", v) for v in (0, 3, 40)] + [("AQ_LA_C", v) for v in (2, 3, 8, 9, 29, 48, 49)]
    hooks += [("AQ_LA_XHELPER", v) for v in (0, 1)] + [("AQ_LA_NOSPLIT", 1)] + [("AQ_MIS_C", v) for v in (1, 2, 8)]
    hooks += [("AQ_TW_WPT", v) for v in (2, 4)] + [("AQ_STAGGER", v) for v in (0, 2)] + [("AQ_HPRIO", v) for v in (0, 2)]
    hooks += [("AQ_MPRIO", 0), ("AQ_XTOUCH", 0), ("AQ_GK_MAX_GB", 0)]
    bases = [(1000, 33, "none"), (1000, 33, "5pct"), (900, 7168, "none"), (1000, 7168, "none"), (1000, 7168, "5pct"), (1500, 33, "none"),
             (5000, 33, "5pct"), (12000, 17, "none"), (12000, 17, "5pct")]
    for name, v in hooks:
        for n, q, na in bases:
            c.append(dict(n=n, p=32, q=q, na=na, env={name: str(v)}))
    # combinations the tests use together
    for n, q, na in bases:
        c.append(dict(n=n, p=32, q=q, na=na, env={"AQ_LA_C": "2", "AQ_LA_XHELPER": "1"}))
        c.append(dict(n=n, p=32, q=q, na=na, env={"AQ_KERNEL": "3", "AQ_MIS_C": "2"}))
        c.append(dict(n=n, p=32, q=q, na=na, env={"AQ_KERNEL": "3", "AQ_CHAIN": "3", "AQ_NCU": "8"}))
        c.append(dict(n=n, p=32, q=q, na=na, env={"AQ_KERNEL": "2", "AQ_TW_WPT": "4"}))
        c.append(dict(n=n, p=32, q=q, na=na, env={"AQ_TT": "2", "AQ_NT3": "9"}))
        c.append(dict(n=n, p=32, q=q, na=na, env={"AQ_TT": "2", "AQ_NT3": "6", "AQ_CHAIN": "3"}))
        c.append(dict(n=n, p=32, q=q, na=na, env={"AQ_NCU": "64", "AQ_CHAIN": "40"}))
    for n in (800, 900, 1000, 1056):
        for v in (0, 3, 6, 9):
            c.append(dict(n=n, p=32, q=2500, na="none", env={"AQ_NT3": str(v)}))
            c.append(dict(n=n, p=32, q=7168, na="none", env={"AQ_NT3": str(v)}))
    # the tables of tests/test_gpu_split_instances.py, a sample of each, at 256 CUs
    for k in (23, 30, 36):
        for na in ("none", "5pct"):
            c.append(dict(n=96 * k - 5, p=32, q=33, na=na, env={"AQ_LA_C": "2", "AQ_NCU": "256"}))
    for nt in (1, 7, 12, 18):
        for na in ("none", "5pct"):
            c.append(dict(n=864 * nt - 7, p=32, q=33, na=na, env={"AQ_LA_C": "9", "AQ_NCU": "256"}))
    for C in range(9, 49):
        c.append(dict(n=4000, p=32, q=21, na="none", env={"AQ_LA_C": str(C), "AQ_NCU": "256"}))
    for n in (8449, 9000, 9300, 9700, 10240, 65000):
        c.append(dict(n=n, p=32, q=33, na="none", env={"AQ_NCU": "256"}))
    c.append(dict(n=5000, p=40, q=1030, na="none", env={"AQ_NCU": "256"}))
    # refused combinations
    c.append(dict(n=12000, p=16, q=17, na="none", env={"AQ_LA_C": "8"}))
    c.append(dict(n=12000, p=16, q=17, na="none", env={"AQ_LA_C": "49"}))
    c.append(dict(n=1000, p=16, q=17, na="none", env={"AQ_LA_C": "49"}))
    c.append(dict(n=12000, p=16, q=17, na="none", env={"AQ_KERNEL": "2"}))
    c.append(dict(n=12000, p=16, q=17, na="5pct", env={"AQ_KERNEL": "3"}))
    c.append(dict(n=12000, p=16, q=17, na="5pct", env={"AQ_GK_MAX_GB": "0"}))
    c.append(dict(n=1000, p=16, q=17, na="5pct", env={"AQ_GK_MAX_GB": "0"}))
    c.append(dict(n=12000, p=16, q=17, na="none", env={"AQ_NCU": "8"}))
    c.append(dict(n=82944, p=16, q=17, na="none", env={"AQ_NCU": "32"}))
    return c


_cache = {}


def problem(n, p, q, na):
    key = (n, p, q, na)
    if key not in _cache:
        _cache.clear()
        rng = np.random.default_rng(n * 7 + q * 3 + p)
        X = np.asfortranarray(rng.normal(size=(n, p)))
        Y = np.asfortranarray(rng.normal(size=(n, q)))
        if na == "5pct" and n >= 16:
            Y[rng.random((n, q)) < 0.05] = np.nan
            Y[0, :] = 0.5
        elif na == "heavy":
            Y[rng.random((n, q)) < 0.02] = np.nan
            Y[5:5 + 1100, q // 2] = np.nan
        elif na == "mostly":
            Y[rng.random((n, q)) < 0.02] = np.nan
            Y[10:10 + (9 * n) // 10, 1] = np.nan
        lh = dict(A2_inv=1.0, m0=0.0, nu=1.0, rho=1.0, t02=0.1, eta=np.ones(q), kappa=np.ones(q), n0=-np.ones(q))
        li = dict(gam_vb=np.full((p, q), 0.05, order="F"), mu_beta_vb=np.full((p, q), 0.01, order="F"), sig02_inv_vb=1.0,
                  sig2_beta_vb=np.full(q, 0.1), sig2_theta_vb=np.full(p, 0.1), tau_vb=np.ones(q), theta_vb=np.zeros(p),
                  zeta_vb=-np.ones(q))
        miss = np.isnan(Y).sum(axis=0)
        _cache[key] = (X, Y, lh, li, int(miss.max()), int(np.minimum(miss, n - miss).max()))
    return _cache[key]


def write_table(path, head, rows):
    """One row per line."""
    with open(path, "w") as f:
        f.write("{" + ", ".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(head.items())) + ',\n"rows": [\n')
        f.write(",\n".join(json.dumps(r, sort_keys=True) for r in rows))
        f.write("\n]}\n")


def main():
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    for k in list(os.environ):
        if k.startswith("AQ_") and k != "AQ_LIB":
            del os.environ[k]
    prop = torch.cuda.get_device_properties(0)
    free_b, tot_b = torch.cuda.mem_get_info(0)
    rows = []
    cs = list({json.dumps(c, sort_keys=True): c for c in cases()}.values())      # each case once
    cs.sort(key=lambda c: (c["n"], c["p"], c["q"], c["na"], sorted(c["env"].items())))      # one problem serves its neighbours
    t0 = time.time()
    for i, c in enumerate(cs):
        X, Y, lh, li, mm, ms = problem(c["n"], c["p"], c["q"], c["na"])
        for k, v in c["env"].items():
            os.environ[k] = v
        row = dict(n=c["n"], p=c["p"], q=c["q"], na=c["na"], max_missing=mm, max_short_list=ms, env=c["env"])
        try:
            run = VbRun(Y, X, lh, li, (1, 2, 10), 0.1, 12, True, True)
            try:
                st = run.status()
            finally:
                run.close()
            row.update(rc=0, error="", overrides=st["overrides"], plan={k: st[k] for k in PLAN_KEYS})
        except AtlasqtlHipError as e:
            m = re.match(r"aq_vb_create: \[(-?\d+)\] (.*)$", str(e), flags=re.S)
            if not m or int(m.group(1)) not in (1, 3):
                print("STOP: unexpected failure", c, e, flush=True)
                return 1
            row.update(rc=int(m.group(1)), error=m.group(2), overrides=None, plan=None)
        finally:
            for k in c["env"]:
                del os.environ[k]
        rows.append(row)
        if i % 20 == 0:
            print(f"{i}/{len(cs)} {time.time() - t0:.0f}s {row}", flush=True)
    write_table(OUT, dict(parent_commit=COMMIT, source="aq_vb_get_status and aq_vb_get_overrides of live handles, tools/record_plan_table.py",
                          device=prop.name, ncu=int(prop.multi_processor_count), total_bytes=int(tot_b), free_bytes_at_start=int(free_b)),
                rows)
    print("recorded", len(rows), "rows,", sum(1 for r in rows if r["rc"]), "refused, in", f"{time.time() - t0:.0f}s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
