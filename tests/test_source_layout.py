"""The source layout of atlasqtl_amd/csrc -- one owner of device memory, one definition per exported symbol, and no
hand-copied prototypes between translation units (they live in headers, where a mismatch is a compile error) -- and of
the Python package around it: one owner of the rank collectives."""
import os
import re

from atlasqtl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "atlasqtl_amd", "csrc")


def _sources(ext=None):
    out = {}
    for fn in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, fn)
        if os.path.isfile(path) and (ext is None or fn.endswith(ext)):
            with open(path) as f:
                out[fn] = f.read()
    return out


def _without_comments(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


# a function declarator that starts a line at file scope: optional extern "C", a return type, the name, the parameters,
# then `{` (definition) or `;` (prototype).  Calls and local declarations are indented; `static` ones are the unit's own.
_DECL = re.compile(r'^(?:extern\s+"C"\s+)?(?!static\b|return\b|typedef\b|using\b)[A-Za-z_][\w:<>\*&, ]*?[\s\*&](aq_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*([;{])',
                   re.M)


def _declarations(src):
    """(name, is_definition, is_extern_c) of every non-static file-scope function declarator."""
    return [(m.group(1), m.group(3) == "{", m.group(0).startswith("extern")) for m in _DECL.finditer(_without_comments(src))]


def test_device_memory_has_one_owner():
    assert "aq_internal.h" in _sources()
    for fn, src in _sources().items():
        if fn != "aq_internal.h":
            assert "hipMalloc(" not in src and "hipFree(" not in src, fn
    owner = _sources()["aq_internal.h"]
    assert "hipMalloc(" in owner and "hipFree(" in owner


def test_every_exported_symbol_is_defined_by_exactly_one_unit():
    defined = {}
    for fn, src in _sources(".hip").items():
        for name, is_def, ext_c in _declarations(src):
            if is_def and ext_c:
                defined.setdefault(name, []).append(fn)
    assert len(_lib.SYMBOLS) >= 15
    for name in _lib.SYMBOLS:
        assert len(defined.get(name, [])) == 1, (name, defined.get(name))


def test_no_unit_declares_what_another_unit_defines():
    units = {fn: _declarations(src) for fn, src in _sources(".hip").items()}
    assert len(units) >= 8
    definer = {}
    for fn, decls in units.items():
        for name, is_def, _ in decls:
            if is_def:
                definer.setdefault(name, set()).add(fn)
    assert "aq_fail" in definer and "aq_bfdr_device" in definer      # the scan sees plain C++ definitions too
    for fn, decls in units.items():
        for name, is_def, _ in decls:
            if not is_def:
                assert not (definer.get(name, set()) - {fn}), (fn, name, "is defined in", definer[name])


def test_the_rank_collectives_have_one_owner():
    """Among atlasqtl_amd/*.py only ranks.py names torch.distributed, and only ranks.py and _lib.py (the load order of the
    two HIP runtimes) import torch: everything else reaches the ranks through ranks.RankGroup."""
    pkg = os.path.join(ROOT, "atlasqtl_amd")
    naming, importing = set(), set()
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith(".py"):
            with open(os.path.join(pkg, fn)) as f:
                src = f.read()
            if "torch.distributed" in src:
                naming.add(fn)
            if re.search(r"\bimport\s+torch\b|\bfrom\s+torch\b|__import__\(\s*[\"']torch", src):
                importing.add(fn)
    assert naming == {"ranks.py"}
    assert importing == {"ranks.py", "_lib.py"}


def _package():
    pkg = os.path.join(ROOT, "atlasqtl_amd")
    out = {}
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith(".py"):
            with open(os.path.join(pkg, fn)) as f:
                out[fn] = f.read()
    return out


def _code_only(src):
    """Python source without its comments and docstrings (the strings that start a statement), token by token."""
    import io
    import tokenize
    out, starts = [], True
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        if tok.type in (tokenize.COMMENT, tokenize.NL):
            continue
        if tok.type in (tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT):
            starts = True
            continue
        if not (starts and tok.type == tokenize.STRING):
            out.append(tok.string)
        starts = False
    return " ".join(out)


def test_the_screen_entries_shared_steps_have_one_owner():
    """Among atlasqtl_amd/*.py: the size of a scan's first table is marginal.py's alone (initial_cap_ and complete_table_ are
    how the others get at the two-call protocol); on_prepared_ is called by marginal.py and by cis.py, whose on_cis_windows_
    all three cis entries go through; and only prepared.py and _lib.py name an entry of the aq_prep_cis family in their code."""
    src = _package()
    assert {fn for fn, s in src.items() if "INITIAL_CAP" in s} == {"marginal.py"}
    assert {fn for fn, s in src.items() if "on_prepared_(" in _code_only(s).replace(" ", "")} == {"marginal.py", "cis.py"}
    assert {fn for fn, s in src.items() if "aq_prep_cis" in _code_only(s)} == {"prepared.py", "_lib.py"}
    for fn in ("cis_condition.py", "cis_susie.py"):
        assert "on_cis_windows_(" in _code_only(src[fn]).replace(" ", "") and "prepare_data_" not in src[fn], fn


def test_the_cis_modules_import_each_other_without_a_cycle():
    """The `from .x import` lines of the cis* modules, parsed and not imported: a graph without a cycle, in which cis.py is
    below the two entries built on its scan and above the two argument modules."""
    src = {fn[:-3]: s for fn, s in _package().items() if fn.startswith("cis")}
    assert set(src) >= {"cis", "cis_lists", "cis_interaction", "cis_condition", "cis_susie"}
    graph = {m: set(re.findall(r"^\s*from\s+\.(cis\w*)\s+import\b", s, flags=re.M)) for m, s in src.items()}
    assert all(not re.search(r"^\s*(?:from\s+\.\s+import|import\s+atlasqtl_amd|from\s+atlasqtl_amd)", s, flags=re.M) for s in src.values())
    assert graph["cis"] == {"cis_lists", "cis_interaction"} and "cis" in graph["cis_condition"] and "cis" in graph["cis_susie"]
    done = set()
    while len(done) < len(graph):                                 # peel off the modules whose imports are all peeled off
        free = {m for m in graph if m not in done and graph[m] <= done}
        assert free, f"an import cycle among {sorted(set(graph) - done)}"
        done |= free


# ---- the look-ahead sweep kernel: aq_core_sweep_la.h and the aq_la_*.h headers beside it ----

def _la_sources():
    src = {fn: s for fn, s in _sources(".h").items() if fn == "aq_core_sweep_la.h" or fn.startswith("aq_la_")}
    assert {"aq_core_sweep_la.h", "aq_la_stream.h", "aq_la_req.h", "aq_la_flags.h", "aq_la_traits.h"} <= set(src)
    return src


def test_hand_off_counters_are_addressed_by_name():
    """No call of signal( or wait_ge( -- plain or as a member of the counters' struct -- passes a number as the counter: the
    names are aq_la_flags.h's."""
    calls = 0
    for fn, s in _la_sources().items():
        for m in re.finditer(r"\b(?:signal|wait_ge)\s*\(\s*([^,)]*)", _without_comments(s)):
            first = m.group(1).strip()
            if re.match(r"AqLaFlag\s+\w+$", first):                  # the two definitions
                continue
            calls += 1
            assert not first[:1].isdigit(), (fn, m.group(0))
            assert "AQ_FL_" in first or "aq_fl_" in first, (fn, m.group(0))
    assert calls >= 20
    flags = _la_sources()["aq_la_flags.h"]
    assert "static_assert" in flags and "alignof(AqLaFlagWords) == 16" in flags


def test_asm_loads_and_exchange_atomics_stay_where_they_belong():
    """The inline-asm load macros are defined in aq_la_stream.h alone and used only by the matrix and helper roles; a.Pbuf is
    named only by the sample-split exchanges.  All three roles live in aq_core_sweep_la.h: taken out into headers of their
    own they moved the register allocation of shipped instances (profiles/r06_la_split_isa.txt)."""
    roles_file = "aq_core_sweep_la.h"
    for fn, s in _sources().items():
        code = _without_comments(s)
        defines = set(re.findall(r"#\s*define\s+(AQ_LD2I|AQ_LD2|AQ_TOUCH)\b", code))
        assert defines == ({"AQ_LD2", "AQ_LD2I", "AQ_TOUCH"} if fn == "aq_la_stream.h" else set()), fn
        uses = re.findall(r"\b(?:AQ_LD2I|AQ_LD2|AQ_TOUCH)\s*\(", re.sub(r"#\s*define[^\n]*", "", code))
        assert bool(uses) == (fn == roles_file), (fn, len(uses))
        if fn in _la_sources():                                      # (the fallback kernel of aq_core_sweep_mis.h has a Pbuf of its own)
            assert ("a.Pbuf" in code) == (fn == roles_file), fn
    assert "asm volatile(\"global_load" not in _without_comments(_sources()[roles_file])


def test_the_look_ahead_headers_include_each_other_without_a_cycle():
    """The #include lines of aq_core_sweep_la.h and the aq_la_*.h headers, parsed: no cycle among them, and the kernel's header
    reaches every one of them."""
    src = _la_sources()
    graph = {fn: {h for h in re.findall(r'^\s*#\s*include\s+"([^"]+)"', s, flags=re.M) if h in src} for fn, s in src.items()}
    done = set()
    while len(done) < len(graph):                                 # peel off the headers whose includes are all peeled off
        free = {h for h in graph if h not in done and graph[h] <= done}
        assert free, f"an include cycle among {sorted(set(graph) - done)}"
        done |= free
    reach, todo = set(), ["aq_core_sweep_la.h"]
    while todo:
        for h in graph[todo.pop()]:
            if h not in reach:
                reach.add(h)
                todo.append(h)
    assert reach == set(src) - {"aq_core_sweep_la.h"}
    assert graph["aq_la_req.h"] == set() and "hip" not in _without_comments(src["aq_la_req.h"])      # plain C++: a host program includes it
