#!/usr/bin/env python3
"""Compare the device code of two builds, kernel by kernel: what a refactor of a kernel did to the code that ships.

    tools/compare_isa.py OLD_BUILD_DIR NEW_BUILD_DIR [--glob 'aq_launch_la*'] [--diff]

Reads only the `*-hip-amdgcn-amd-amdhsa-gfx950.s` listings that `make` leaves in a build directory (-save-temps=obj), pairs
them by file name and their kernels by symbol, and puts every kernel symbol into one of three tiers:

  tier 1   the kernel's text is identical (lines naming `__hip_cuid_` ignored);
  tier 2   registers renamed and independent instructions reordered, nothing else: equal .vgpr_count, .sgpr_count,
           .agpr_count, .private_segment_fixed_size and .group_segment_fixed_size; equal multiset of instruction mnemonics;
           equal number of s_waitcnt instructions and equal multiset of their operands; equal number of instructions whose
           mnemonic begins with `scratch_`; equal number of basic-block labels.  Reported with the number of text lines
           that differ and how many of those differ in code, i.e. outside the listing's `;` comments;
  beyond   anything else -- each term that differs is printed with both values.

All mnemonics count alike: none is looked for in particular.  Exit status 0 when every symbol is in tier 1 or 2 and both
builds hold the same symbols, 1 otherwise.
"""
import argparse
import collections
import difflib
import glob
import os
import re
import sys

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
META_KEYS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
BLOCK = re.compile(r"^\.LBB\d+_\d+:")
MNEMONIC = re.compile(r"^\s+([a-z][a-z0-9_]*)\b(.*)$")


def parse_listing(text):
    """{kernel symbol: {"lines": [...], "meta": {...}}} of one listing: the body from the symbol's label to its .Lfunc_end, and
    the kernel's entry in the amdhsa.kernels metadata."""
    lines = text.splitlines()
    meta, cur = {}, None
    in_meta = False
    for ln in lines:
        if ln.startswith("amdhsa.kernels:"):
            in_meta = True
            continue
        if not in_meta:
            continue
        if ln.startswith("  - ."):          # a new kernel entry (argument entries are nested deeper)
            cur = {}
            ln = "    " + ln[4:]
        elif not ln.startswith("    "):
            if ln.strip() and not ln.startswith(" "):
                in_meta = False
            continue
        m = re.match(r"^    (\.\w+):\s*(\S*)\s*$", ln)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == ".name":
                meta[m.group(2)] = cur
    kernels = {}
    name, body = None, None
    for ln in lines:
        if name is None:
            m = LABEL.match(ln)
            if m and m.group(1) in meta:
                name, body = m.group(1), []
            continue
        if ln.startswith(".Lfunc_end"):
            kernels[name] = {"lines": body, "meta": meta[name]}
            name = None
            continue
        if "__hip_cuid_" not in ln:
            body.append(ln)
    return kernels


def profile(k):
    """The tier-2 terms of one kernel."""
    mnem, waits, blocks, scratch = collections.Counter(), collections.Counter(), 0, 0
    for ln in k["lines"]:
        code = ln.split(";", 1)[0].rstrip()
        if BLOCK.match(code):
            blocks += 1
            continue
        m = MNEMONIC.match(code)
        if not m:
            continue
        op = m.group(1)
        mnem[op] += 1
        if op == "s_waitcnt":
            waits[" ".join(m.group(2).split())] += 1
        if op.startswith("scratch_"):
            scratch += 1
    p = {key: k["meta"].get(key) for key in META_KEYS}
    p.update({"mnemonics": mnem, "s_waitcnt": sum(waits.values()), "s_waitcnt operands": waits, "scratch_*": scratch,
              "basic-block labels": blocks})
    return p


def code_only(lines):
    """The lines without their comments (`; ...`: block names of the compiler's IR, implicit-def notes), empty ones dropped."""
    out = (ln.split(";", 1)[0].rstrip() for ln in lines)
    return [ln for ln in out if ln]


def diff_lines(a, b):
    return sum(1 for d in difflib.unified_diff(a, b, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))


def counter_delta(a, b):
    return ", ".join("%s %d->%d" % (key, a[key], b[key]) for key in sorted(set(a) | set(b)) if a[key] != b[key])


def compare_kernel(old, new):
    """(tier, detail): tier 1 / 2 / 3 (beyond); detail = diff line count for tier 2, the differing terms for tier 3."""
    if old["lines"] == new["lines"] and all(old["meta"].get(k) == new["meta"].get(k) for k in META_KEYS):
        return 1, ""
    po, pn = profile(old), profile(new)
    bad = []
    for key in po:
        if po[key] != pn[key]:
            if isinstance(po[key], collections.Counter):
                bad.append("%s: %s" % (key, counter_delta(po[key], pn[key])))
            else:
                bad.append("%s: %s -> %s" % (key, po[key], pn[key]))
    ndiff = diff_lines(old["lines"], new["lines"])
    ncode = diff_lines(code_only(old["lines"]), code_only(new["lines"]))      # what is left without the listing's comments
    if not bad:
        return 2, "%d diff lines, %d of them in code" % (ndiff, ncode)
    return 3, "; ".join(bad) + " (%d diff lines, %d of them in code)" % (ndiff, ncode)


def compare_dirs(old_dir, new_dir, pattern="*", show_diff=False, out=sys.stdout):
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(old_dir, pattern + SUFFIX)))
    names_new = sorted(os.path.basename(p) for p in glob.glob(os.path.join(new_dir, pattern + SUFFIX)))
    ok = True
    if names != names_new:
        print("listings differ: only old %s, only new %s" % (sorted(set(names) - set(names_new)), sorted(set(names_new) - set(names))),
              file=out)
        ok = False
    tiers = collections.Counter()
    for name in sorted(set(names) & set(names_new)):
        with open(os.path.join(old_dir, name)) as f:
            old = parse_listing(f.read())
        with open(os.path.join(new_dir, name)) as f:
            new = parse_listing(f.read())
        unit = name[:-len(SUFFIX)]
        for sym in sorted(set(old) ^ set(new)):
            print("%s: %s only in the %s build" % (unit, sym, "old" if sym in old else "new"), file=out)
            ok = False
        t = collections.Counter()
        for sym in sorted(set(old) & set(new)):
            tier, detail = compare_kernel(old[sym], new[sym])
            t[tier] += 1
            if tier == 2:
                print("%s: tier 2  %s  %s" % (unit, sym, detail), file=out)
            elif tier == 3:
                print("%s: BEYOND  %s  %s" % (unit, sym, detail), file=out)
                ok = False
            if tier != 1 and show_diff:
                for d in difflib.unified_diff(old[sym]["lines"], new[sym]["lines"], lineterm="", n=0):
                    print("    " + d, file=out)
        print("%s: %d symbols -- tier 1 (identical) %d, tier 2 %d, beyond %d" % (unit, sum(t.values()), t[1], t[2], t[3]), file=out)
        tiers.update(t)
    print("total: %d symbols -- tier 1 (identical) %d, tier 2 %d, beyond %d" % (sum(tiers.values()), tiers[1], tiers[2], tiers[3]),
          file=out)
    return ok


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_build_dir")
    ap.add_argument("new_build_dir")
    ap.add_argument("--glob", default="*", help="listings to compare, by unit name (default: all)")
    ap.add_argument("--diff", action="store_true", help="print the text diff of every symbol that is not identical")
    args = ap.parse_args(argv)
    return 0 if compare_dirs(args.old_build_dir, args.new_build_dir, args.glob, args.diff) else 1


if __name__ == "__main__":
    sys.exit(main())
