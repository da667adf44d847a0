"""PLINK 1 binary filesets (.bed / .bim / .fam) as the X of atlasqtl().

The .bed holds 2 bits per genotype, variant-major: after the three header bytes 0x6c 0x1b 0x01 one block of
stride = (n_file + 3) // 4 bytes per variant, in .bim order; sample s of a variant is (block[s >> 2] >> (2 * (s & 3))) & 3
with 0 = homozygous A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2.  Nothing is unpacked here: PlinkBed parses the
two text files, validates the .bed and hands the packed blocks of the selected variants to the library (the .bed input of
aq_prepare_data_opt), which unpacks them on the GPU (csrc/aq_prep_bed.hip).  The .bed is memory-mapped, so only the selected blocks are read.
"""
from __future__ import annotations

import os

import numpy as np

from .checks import AtlasqtlError

BED_MAGIC = (0x6C, 0x1B)


def make_unique(names):
    """R's make.unique(names): the first occurrence keeps its name, a later one takes name.1, name.2, ... skipping every
    name that is already in use."""
    used = set(names)
    seen = set()
    cnt = {}
    out = []
    for nm in names:
        if nm not in seen:
            seen.add(nm)
            out.append(nm)
            continue
        k = cnt.get(nm, 1)
        while f"{nm}.{k}" in used:
            k += 1
        new = f"{nm}.{k}"
        cnt[nm] = k + 1
        used.add(new)
        out.append(new)
    return out


def _read_table(path, what):
    """The lines of a .bim / .fam as lists of six whitespace-separated fields."""
    if not os.path.isfile(path):
        raise AtlasqtlError(f"{path} not found: a PLINK fileset needs its {what} file next to the .bed.")
    rows = []
    with open(path, "r") as f:
        for ln, line in enumerate(f, 1):
            fields = line.split()
            if not fields:
                continue
            if len(fields) != 6:
                raise AtlasqtlError(f"{path}, line {ln}: {len(fields)} fields where a {what} line has 6.")
            rows.append(fields)
    if not rows:
        raise AtlasqtlError(f"{path} holds no {what} line.")
    return rows


class PlinkBed:
    """A PLINK 1 fileset, with a selection of its variants and samples, as input X of atlasqtl() / prepare_on_device().

    path      the fileset prefix or the path of the .bed; the .bim and .fam are found next to it
    snps      None, a slice, or an increasing integer array: the variants (lines of the .bim) used
    samples   None, or an integer array of file rows (lines of the .fam) in the order of the rows of Y, without repeats
    count     "A1" (dosage 2 / 1 / 0 of the .bim's first allele) or "A2"
    missing   "error": a missing genotype among the rows used is refused; "mean": it takes the mean of its variant's
              observed genotypes

    n, p, shape, snp_names (made unique as R's make.unique does), sample_ids (IID), chrom, pos, a1, a2: after selection."""

    def __init__(self, path, snps=None, samples=None, count="A1", missing="error"):
        path = os.fspath(path)
        prefix = path[:-4] if path.lower().endswith(".bed") else path
        self.bed_path, self.bim_path, self.fam_path = prefix + ".bed", prefix + ".bim", prefix + ".fam"
        if count not in ("A1", "A2"):
            raise AtlasqtlError(f'count must be "A1" or "A2", not {count!r}.')
        if missing not in ("error", "mean"):
            raise AtlasqtlError(f'missing must be "error" or "mean", not {missing!r}.')
        self.count, self.missing = count, missing
        if not os.path.isfile(self.bed_path):
            raise AtlasqtlError(f"{self.bed_path} not found.")
        bim = _read_table(self.bim_path, ".bim")
        fam = _read_table(self.fam_path, ".fam")
        self.n_file, self.p_file = len(fam), len(bim)
        self.stride = (self.n_file + 3) // 4
        with open(self.bed_path, "rb") as f:
            head = f.read(3)
        size = os.path.getsize(self.bed_path)
        if len(head) < 3 or (head[0], head[1]) != BED_MAGIC:
            raise AtlasqtlError(f"{self.bed_path} is not a PLINK 1 .bed file: it begins with "
                                f"{' '.join(f'0x{b:02x}' for b in head)}, not with the magic bytes 0x6c 0x1b.")
        if head[2] == 0x00:
            raise AtlasqtlError(f"{self.bed_path} is a sample-major .bed file (mode byte 0x00): only variant-major files "
                                "(mode byte 0x01) are read. Convert it with PLINK (--make-bed).")
        if head[2] != 0x01:
            raise AtlasqtlError(f"{self.bed_path} is not a PLINK 1 .bed file: mode byte 0x{head[2]:02x}, not 0x01.")
        want = 3 + self.p_file * self.stride
        if size != want:
            raise AtlasqtlError(f"{self.bed_path} has {size} bytes, but {self.p_file} variants ({self.bim_path}) of "
                                f"{self.n_file} samples ({self.fam_path}) take 3 + {self.p_file} x {self.stride} = {want} bytes.")

        # variants
        if snps is None:
            snps = slice(None)
        if isinstance(snps, slice):
            start, stop, step = snps.indices(self.p_file)
            if step == 1:
                self._snp_range, self._snp_idx = (start, max(start, stop)), None
                sel = np.arange(start, max(start, stop))
            else:
                sel = np.arange(start, stop, step)
                self._snp_range, self._snp_idx = None, sel
        else:
            sel = self._index_array(snps, "snps", self.p_file)
            self._snp_range, self._snp_idx = None, sel
        if sel.size == 0:
            raise AtlasqtlError("snps selects no variant.")
        if sel.size > 1 and np.any(np.diff(sel) <= 0):
            raise AtlasqtlError("snps must be increasing (the variants keep the order of the .bim).")
        self.snp_index = sel

        # samples
        if samples is None:
            self.sample_index = None
            srows = range(self.n_file)
        else:
            sidx = self._index_array(samples, "samples", self.n_file)
            if np.unique(sidx).size != sidx.size:
                raise AtlasqtlError("samples holds a file row more than once.")
            self.sample_index = np.ascontiguousarray(sidx, dtype=np.int32)
            srows = sidx
        self.sample_ids = [fam[i][1] for i in srows]
        rows = [bim[j] for j in sel]
        self.snp_names = make_unique([r[1] for r in rows])
        self.chrom = [r[0] for r in rows]
        try:
            self.pos = np.array([int(r[3]) for r in rows], dtype=np.int64)
        except ValueError as e:
            raise AtlasqtlError(f"{self.bim_path}: a base-pair position is not an integer ({e}).") from e
        self.a1 = [r[4] for r in rows]
        self.a2 = [r[5] for r in rows]
        self.n, self.p = len(self.sample_ids), len(rows)
        self.shape = (self.n, self.p)
        self._mm = None

    @staticmethod
    def _index_array(x, name, size):
        a = np.asarray(x)
        if a.ndim != 1 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
            raise AtlasqtlError(f"{name} must be a non-empty one-dimensional integer array.")
        a = a.astype(np.int64)
        if a.min() < 0 or a.max() >= size:
            bad = a[(a < 0) | (a >= size)][0]
            raise AtlasqtlError(f"{name} holds {bad}, outside [0, {size}).")
        return a

    def packed(self):
        """The blocks of the selected variants, p x stride uint8, C-contiguous: a view of the memory map for a contiguous
        range of variants (nothing is read before the upload), else a copy of the selected blocks only."""
        if self._mm is None:
            self._mm = np.memmap(self.bed_path, dtype=np.uint8, mode="r", offset=3, shape=(self.p_file, self.stride))
        if self._snp_range is not None:
            return self._mm[self._snp_range[0]:self._snp_range[1]]
        return np.ascontiguousarray(self._mm[self._snp_idx])

    def __repr__(self):
        return (f"PlinkBed({self.bed_path!r}: {self.n} of {self.n_file} samples, {self.p} of {self.p_file} variants, "
                f"count={self.count!r}, missing={self.missing!r})")
