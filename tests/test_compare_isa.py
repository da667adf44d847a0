"""tools/compare_isa.py, the kernel-by-kernel comparison of two builds' device code that a refactor of a kernel is held to: the
tool itself must sort symbols into the tiers it names.  Two small synthetic listings in the shape hipcc -S emits, written into
two build directories (no GPU, no compiler)."""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import compare_isa as C  # noqa: E402

NAME = "aq_launch_la1" + C.SUFFIX
K1, K2 = "_Z6kern_aILi1EEv10AqCoreArgs", "_Z6kern_bILi2EEv10AqCoreArgs"


def kernel(sym, n, body):
    return (f"\t.globl\t{sym}\n\t.type\t{sym},@function\n{sym}: ; @{sym}\n; %bb.0:\n" + body +
            f"\ts_endpgm\n.Lfunc_end{n}:\n\t.size\t{sym}, .Lfunc_end{n}-{sym}\n")


def meta(sym, vgpr=64, sgpr=32, scratch=0, lds=1024):
    return (f"  - .agpr_count:     0\n    .args:\n      - .address_space:  global\n        .offset:         0\n        .size:           8\n"
            f"    .group_segment_fixed_size: {lds}\n    .name:           {sym}\n    .private_segment_fixed_size: {scratch}\n"
            f"    .sgpr_count:     {sgpr}\n    .symbol:         {sym}.kd\n    .vgpr_count:     {vgpr}\n")


def listing(bodies, metas, cuid="abc"):
    text = "\t.text\n" + "".join(kernel(s, i, b) for i, (s, b) in enumerate(bodies))
    text += f"\t.type\t__hip_cuid_{cuid},@object\n__hip_cuid_{cuid}:\n\t.byte\t0\n"
    return text + "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + "".join(metas) + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n"


BODY = ("\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n\tv_mov_b32_e32 v1, 0\n\ts_waitcnt lgkmcnt(0)\n.LBB0_1: ; =>loop\n"
        "\tglobal_load_dwordx2 v[2:3], v1, s[0:1]\n\tv_add_u32_e32 v4, 1, v4\n\ts_waitcnt vmcnt(0)\n\tv_add_f64 v[6:7], v[2:3], v[6:7]\n"
        "\ts_cbranch_scc1 .LBB0_1\n")
# registers renamed and two independent instructions swapped
RENAMED = BODY.replace("v[2:3]", "v[8:9]").replace("\tglobal_load_dwordx2 v[8:9], v1, s[0:1]\n\tv_add_u32_e32 v4, 1, v4\n",
                                                   "\tv_add_u32_e32 v4, 1, v4\n\tglobal_load_dwordx2 v[8:9], v1, s[0:1]\n")
SPILLED = BODY.replace("\ts_waitcnt vmcnt(0)\n", "\tscratch_store_dwordx2 off, v[6:7], off offset:8\n\ts_waitcnt vmcnt(0)\n")
WAITS = BODY.replace("s_waitcnt vmcnt(0)", "s_waitcnt vmcnt(1)")
BLOCKS = BODY.replace("\tv_add_f64", ".LBB0_2:\n\tv_add_f64")


def test_listing_is_split_into_kernels_with_their_metadata():
    ks = C.parse_listing(listing([(K1, BODY), (K2, SPILLED)], [meta(K1), meta(K2, vgpr=128, scratch=16)]))
    assert set(ks) == {K1, K2}
    assert ks[K1]["meta"][".vgpr_count"] == "64" and ks[K2]["meta"][".private_segment_fixed_size"] == "16"
    assert ks[K1]["meta"][".group_segment_fixed_size"] == "1024"
    p = C.profile(ks[K1])
    assert p["mnemonics"]["s_waitcnt"] == 2 and p["s_waitcnt"] == 2 and p["basic-block labels"] == 1 and p["scratch_*"] == 0
    assert p["s_waitcnt operands"] == {"lgkmcnt(0)": 1, "vmcnt(0)": 1}
    assert C.profile(ks[K2])["scratch_*"] == 1
    assert not any("s_endpgm" not in "".join(k["lines"]) for k in ks.values())


def tier(old_body, new_body, old_meta=None, new_meta=None):
    old = C.parse_listing(listing([(K1, old_body)], [old_meta or meta(K1)]))[K1]
    new = C.parse_listing(listing([(K1, new_body)], [new_meta or meta(K1)], cuid="xyz"))[K1]
    return C.compare_kernel(old, new)


def test_identical_text_is_tier_1_whatever_the_cuid():
    assert tier(BODY, BODY) == (1, "")


def test_renamed_registers_and_reordered_instructions_are_tier_2():
    t, detail = tier(BODY, RENAMED)
    assert t == 2 and detail == "4 diff lines, 4 of them in code"
    t, detail = tier(BODY, BODY.replace("; =>loop", "; =>Loop1234"))                 # a comment alone: no code line differs
    assert t == 2 and detail == "2 diff lines, 0 of them in code"


def test_every_tier_2_term_is_held():
    for new_body, new_meta, word in [(SPILLED, None, "scratch_*"), (WAITS, None, "s_waitcnt operands"), (BLOCKS, None, "basic-block labels"),
                                     (BODY.replace("v_add_f64", "v_mul_f64"), None, "mnemonics"),
                                     (RENAMED, meta(K1, vgpr=65), ".vgpr_count"), (RENAMED, meta(K1, sgpr=33), ".sgpr_count"),
                                     (RENAMED, meta(K1, scratch=8), ".private_segment_fixed_size"),
                                     (RENAMED, meta(K1, lds=2048), ".group_segment_fixed_size")]:
        t, detail = tier(BODY, new_body, None, new_meta)
        assert t == 3 and word in detail, (word, detail)
    assert tier(BODY, BODY, None, meta(K1, vgpr=65))[0] == 3        # identical text, another register count


def test_two_build_directories(tmp_path):
    old, new = tmp_path / "old", tmp_path / "new"
    old.mkdir()
    new.mkdir()
    (old / NAME).write_text(listing([(K1, BODY), (K2, BODY)], [meta(K1), meta(K2)]))
    (new / NAME).write_text(listing([(K1, BODY), (K2, RENAMED)], [meta(K1), meta(K2)], cuid="xyz"))
    (old / "notes.txt").write_text("not a listing")
    out = io.StringIO()
    assert C.compare_dirs(str(old), str(new), out=out)
    assert "total: 2 symbols -- tier 1 (identical) 1, tier 2 1, beyond 0" in out.getvalue() and "tier 2  " + K2 in out.getvalue()
    (new / NAME).write_text(listing([(K1, BODY), (K2, SPILLED)], [meta(K1), meta(K2, scratch=16)], cuid="xyz"))
    out = io.StringIO()
    assert not C.compare_dirs(str(old), str(new), out=out)
    assert "BEYOND  " + K2 in out.getvalue() and "beyond 1" in out.getvalue()
    (new / NAME).write_text(listing([(K1, BODY)], [meta(K1)]))
    out = io.StringIO()
    assert not C.compare_dirs(str(old), str(new), out=out)            # a symbol that left the build is not a pass
    assert K2 + " only in the old build" in out.getvalue()
    assert C.main([str(old), str(old), "--glob", "aq_launch_la*"]) == 0
