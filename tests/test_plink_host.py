"""PLINK 1 filesets on the host: parsing and validation of .bed / .bim / .fam (atlasqtl_amd/plink.py), the selections, and
the argument checks of aq_prepare_data_bed, which need no GPU.  The files are written by tests/bed_util.py, from the format
alone."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from atlasqtl_amd import AtlasqtlError, PlinkBed, _lib
from atlasqtl_amd.plink import make_unique
from tests import bed_util

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY = os.path.join(GOLDEN, "plink_toy")
NA = bed_util.NA
TOY_A1 = np.array([[2, 0, NA, 0, 0, 0], [0, NA, 1, 0, 0, 0], [0, 1, 1, NA, NA, 2]]).T      # 6 samples x 3 variants


def _codes(blocks, n):
    """The 2-bit codes of packed blocks (p x stride): p x n."""
    s = np.arange(n)
    return (blocks[:, s >> 2] >> (2 * (s & 3))) & 3


def _a1_dosage(codes):
    return np.choose(codes, [2, NA, 1, 0])


def test_toy_fixture_parses():
    assert open(TOY + ".bed", "rb").read() == bytes.fromhex("6c1b01dc0fe70f6b01")
    for path in (TOY + ".bed", TOY):
        b = PlinkBed(path)
        assert (b.n, b.p, b.shape, b.n_file, b.p_file, b.stride) == (6, 3, (6, 3), 6, 3, 2)
        assert b.snp_names == ["rs101", "rs202", "rs303"]
        assert b.sample_ids == ["S1", "S2", "S3", "S4", "S5", "S6"]
        assert b.chrom == ["1", "1", "2"] and list(b.pos) == [1000, 2500, 777]
        assert b.a1 == ["A", "C", "G"] and b.a2 == ["G", "T", "A"]
        assert b.count == "A1" and b.missing == "error" and b.sample_index is None
        blocks = b.packed()
        assert blocks.shape == (3, 2) and blocks.dtype == np.uint8
        np.testing.assert_array_equal(_a1_dosage(_codes(blocks, 6)).T, TOY_A1)


def test_writer_reproduces_the_toy_bytes():
    """tests/bed_util.py against the known answer (the fixture's padding bits are zero, as the writer's without pad_rng)."""
    assert bed_util.pack_bed(TOY_A1) == bytes.fromhex("6c1b01dc0fe70f6b01")
    noisy = bed_util.pack_bed(TOY_A1, pad_rng=np.random.default_rng(1))
    mask = bytes([0xFF] * 3 + [0xFF, 0x0F] * 3)             # the high four bits of every second byte are padding
    assert bytes(a & m for a, m in zip(noisy, mask)) == bytes.fromhex("6c1b01dc0fe70f6b01")


def test_make_unique_like_r():
    assert make_unique(["rs1", "rs1", "rs2", "rs1"]) == ["rs1", "rs1.1", "rs2", "rs1.2"]
    assert make_unique([".", ".", "."]) == [".", "..1", "..2"]
    assert make_unique(["a", "a", "a.1"]) == ["a", "a.2", "a.1"]          # a name in use is skipped
    assert make_unique(["x", "y"]) == ["x", "y"]


def test_duplicate_variant_ids(tmp_path):
    rng = np.random.default_rng(0)
    G = rng.integers(0, 3, size=(9, 6))
    bed_util.write_fileset(tmp_path / "d", G, snp_ids=["rs1", ".", "rs1", ".", "rs9", "rs1"])
    b = PlinkBed(tmp_path / "d")
    assert b.snp_names == ["rs1", ".", "rs1.1", "..1", "rs9", "rs1.2"]
    assert len(set(b.snp_names)) == 6
    assert PlinkBed(tmp_path / "d", snps=slice(2, 6)).snp_names == ["rs1", ".", "rs9", "rs1.1"]     # unique after selection


@pytest.fixture
def fileset(tmp_path):
    rng = np.random.default_rng(11)
    n, p = 23, 40
    G = rng.integers(0, 3, size=(n, p))
    G[rng.random(G.shape) < 0.05] = NA
    snp_ids, sample_ids = bed_util.write_fileset(tmp_path / "f", G, pad_rng=rng)
    return str(tmp_path / "f"), G, snp_ids, sample_ids


def _rewrite_bed(prefix, data):
    with open(prefix + ".bed", "wb") as f:
        f.write(data)


def test_file_errors(fileset):
    prefix, G, _, _ = fileset
    good = open(prefix + ".bed", "rb").read()
    assert len(good) == 3 + 40 * 6
    _rewrite_bed(prefix, b"\x6c\x1c\x01" + good[3:])
    with pytest.raises(AtlasqtlError, match=r"f\.bed is not a PLINK 1 \.bed file.*0x6c 0x1c.*magic bytes 0x6c 0x1b"):
        PlinkBed(prefix)
    _rewrite_bed(prefix, b"\x6c\x1b\x00" + good[3:])
    with pytest.raises(AtlasqtlError, match=r"f\.bed is a sample-major .*0x00.*variant-major"):
        PlinkBed(prefix)
    _rewrite_bed(prefix, b"\x6c\x1b\x02" + good[3:])
    with pytest.raises(AtlasqtlError, match=r"not a PLINK 1 \.bed file: mode byte 0x02"):
        PlinkBed(prefix)
    _rewrite_bed(prefix, good[:-7])
    with pytest.raises(AtlasqtlError, match=r"f\.bed has 236 bytes, but 40 variants .* 23 samples .* 3 \+ 40 x 6 = 243 bytes"):
        PlinkBed(prefix)
    _rewrite_bed(prefix, good + b"\x00")
    with pytest.raises(AtlasqtlError, match=r"f\.bed has 244 bytes, but 40 variants .* = 243 bytes"):
        PlinkBed(prefix)
    _rewrite_bed(prefix, good)
    assert PlinkBed(prefix).shape == (23, 40)
    for ext in (".bim", ".fam"):
        shutil.move(prefix + ext, prefix + ext + ".away")
        with pytest.raises(AtlasqtlError, match=rf"f\{ext} not found"):
            PlinkBed(prefix)
        shutil.move(prefix + ext + ".away", prefix + ext)
    with open(prefix + ".bim", "a") as f:
        f.write("1 rsX 0 5\n")
    with pytest.raises(AtlasqtlError, match=r"f\.bim, line 41: 4 fields"):
        PlinkBed(prefix)
    with pytest.raises(AtlasqtlError, match=r"nowhere\.bed not found"):
        PlinkBed(os.path.join(os.path.dirname(prefix), "nowhere"))
    with pytest.raises(AtlasqtlError, match="count must be"):
        PlinkBed(prefix, count="B")
    with pytest.raises(AtlasqtlError, match="missing must be"):
        PlinkBed(prefix, missing="median")


def test_selection(fileset):
    prefix, G, snp_ids, sample_ids = fileset
    n, p = G.shape
    full = PlinkBed(prefix)
    whole = full.packed()
    assert isinstance(whole, np.memmap) and whole.shape == (p, 6)
    np.testing.assert_array_equal(_a1_dosage(_codes(np.asarray(whole), n)).T, G)      # writer and layout agree
    # a contiguous slice: a view of the memory map, no copy
    b = PlinkBed(prefix, snps=slice(5, 17))
    blk = b.packed()
    assert b.shape == (n, 12) and b.snp_names == snp_ids[5:17] and list(b.pos) == [10000 + 13 * j for j in range(5, 17)]
    assert isinstance(blk, np.memmap) and blk.flags["C_CONTIGUOUS"] and blk.shape == (12, 6)
    assert np.shares_memory(blk, b._mm) and blk.ctypes.data == b._mm.ctypes.data + 5 * 6
    np.testing.assert_array_equal(np.asarray(blk), np.asarray(whole)[5:17])
    # a strided slice and an index array: the selected blocks only
    b = PlinkBed(prefix, snps=slice(1, 30, 4))
    assert b.snp_names == snp_ids[1:30:4] and b.p == 8
    np.testing.assert_array_equal(b.packed(), np.asarray(whole)[1:30:4])
    idx = np.array([0, 3, 4, 22, 39])
    b = PlinkBed(prefix, snps=idx)
    assert b.shape == (n, 5) and b.snp_names == [snp_ids[j] for j in idx] and b.a1 == ["ACGT"[j % 4] for j in idx]
    assert b.chrom == [str(1 + j % 22) for j in idx]
    blk = b.packed()
    assert blk.flags["C_CONTIGUOUS"] and not np.shares_memory(blk, b._mm)
    np.testing.assert_array_equal(blk, np.asarray(whole)[idx])
    # samples: rows of the file in the order of the rows of Y
    rows = np.array([7, 0, 22, 3, 11])
    b = PlinkBed(prefix, snps=idx, samples=rows, count="A2", missing="mean")
    assert b.shape == (5, 5) and b.n_file == n and b.sample_ids == [sample_ids[i] for i in rows]
    assert b.sample_index.dtype == np.int32 and list(b.sample_index) == list(rows)
    assert (b.count, b.missing) == ("A2", "mean")
    assert PlinkBed(prefix, snps=[2]).shape == (n, 1)


def test_bad_selections(fileset):
    prefix = fileset[0]
    with pytest.raises(AtlasqtlError, match="samples holds a file row more than once"):
        PlinkBed(prefix, samples=[1, 5, 1])
    with pytest.raises(AtlasqtlError, match=r"samples holds 23, outside \[0, 23\)"):
        PlinkBed(prefix, samples=[0, 23])
    with pytest.raises(AtlasqtlError, match=r"samples holds -1, outside"):
        PlinkBed(prefix, samples=[-1, 2])
    with pytest.raises(AtlasqtlError, match=r"snps holds 40, outside \[0, 40\)"):
        PlinkBed(prefix, snps=[3, 40])
    with pytest.raises(AtlasqtlError, match="snps must be increasing"):
        PlinkBed(prefix, snps=[3, 9, 8])
    with pytest.raises(AtlasqtlError, match="snps must be increasing"):
        PlinkBed(prefix, snps=[3, 3])
    with pytest.raises(AtlasqtlError, match="snps must be increasing"):
        PlinkBed(prefix, snps=slice(10, 2, -1))
    with pytest.raises(AtlasqtlError, match="snps selects no variant"):
        PlinkBed(prefix, snps=slice(7, 7))
    with pytest.raises(AtlasqtlError, match="integer array"):
        PlinkBed(prefix, snps=[0.5, 2.0])
    with pytest.raises(AtlasqtlError, match="integer array"):
        PlinkBed(prefix, samples=[])


def test_bed_argument_errors_need_no_gpu(hiplib):
    """Every argument error of aq_prepare_data_bed is AQ_ERR_ARG before the device is looked for."""
    n_file, p, q = 6, 3, 2
    bed = np.frombuffer(bytes.fromhex("dc0fe70f6b01"), dtype=np.uint8).copy()
    Y = np.asfortranarray(np.arange(12, dtype=np.float64).reshape(6, 2))
    idx = np.array([0, 1, 2, 3, 4, 5], dtype=np.int32)

    def call(out=True, **kw):
        pin = _lib.AqPrepBedInput()
        a = dict(n_file=n_file, n=6, p=p, q=q, bed=bed, sample_idx=None, Y=Y, count_a2=0, missing=0, device=0)
        a.update(kw)
        pin.n_file, pin.n, pin.p, pin.q = a["n_file"], a["n"], a["p"], a["q"]
        pin.bed = None if a["bed"] is None else a["bed"].ctypes.data_as(C.POINTER(C.c_uint8))
        pin.sample_idx = None if a["sample_idx"] is None else _lib.as_ip(a["sample_idx"])
        pin.Y = None if a["Y"] is None else _lib.as_dp(a["Y"])
        pin.count_a2, pin.missing, pin.device = a["count_a2"], a["missing"], a["device"]
        h = C.c_void_p()
        rc = hiplib.aq_prepare_data_bed(C.byref(pin), C.byref(h) if out else None)
        return rc, hiplib.aq_last_error().decode(), h

    assert hiplib.aq_prepare_data_bed(None, None) == 1 and b"NULL" in hiplib.aq_last_error()
    rc, msg, _ = call(out=False)
    assert rc == 1 and "NULL" in msg
    for kw, words in [(dict(bed=None), "NULL data pointer"), (dict(Y=None), "NULL data pointer"),
                      (dict(n=1, sample_idx=idx[:1]), "n >= 2"), (dict(p=0), "p >= 1"), (dict(q=0), "q >= 1"),
                      (dict(n=7, sample_idx=np.zeros(7, dtype=np.int32)), "n = 7 rows asked of a file with n_file = 6"),
                      (dict(n=4), "sample_idx is NULL, so n = 4 must equal n_file = 6"),
                      (dict(n=3, sample_idx=np.array([0, 6, 1], dtype=np.int32)), "sample_idx[1] = 6 is out of range [0, 6)"),
                      (dict(n=3, sample_idx=np.array([0, 2, -1], dtype=np.int32)), "sample_idx[2] = -1 is out of range"),
                      (dict(count_a2=2), "count_a2 and missing must be 0 or 1"),
                      (dict(missing=-1), "count_a2 and missing must be 0 or 1")]:
        rc, msg, h = call(**kw)
        assert rc == 1 and words in msg and msg.startswith("aq_prepare_data_bed:"), (kw, rc, msg)
        assert h.value is None
    assert hiplib.aq_prep_genotype_counts(None, None) == 1 and b"NULL" in hiplib.aq_last_error()
    if hiplib.aq_device_count() < 1:                          # all arguments good: now, and only now, the device is missed
        rc, msg, h = call()
        assert rc == 2 and "no HIP device" in msg and h.value is None
