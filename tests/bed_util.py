"""A writer of PLINK 1 binary filesets for the tests, from the format alone and independent of atlasqtl_amd/plink.py.

.bed: 0x6c 0x1b 0x01, then per variant (n + 3) // 4 bytes; sample s sits in bits 2 (s & 3) .. 2 (s & 3) + 1 of byte s >> 2;
code 0 = homozygous A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2.  The unused high bits of a variant's last byte are
padding of unspecified value: `pad_rng` fills them with random bits."""
import numpy as np

NA = -1                                    # a missing genotype in the dosage matrices handed to write_fileset
_CODE_OF_A1_DOSAGE = {2: 0, NA: 1, 1: 2, 0: 3}


def pack_bed(G_a1, pad_rng=None):
    """G_a1: n x p integers, the A1 dosages 0 / 1 / 2 or NA.  Returns the bytes of the .bed file."""
    G_a1 = np.asarray(G_a1)
    n, p = G_a1.shape
    codes = np.empty((n, p), dtype=np.uint8)
    for dosage, code in _CODE_OF_A1_DOSAGE.items():
        codes[G_a1 == dosage] = code
    assert np.isin(G_a1, list(_CODE_OF_A1_DOSAGE)).all()
    stride = (n + 3) // 4
    full = np.zeros((4 * stride, p), dtype=np.uint8)
    full[:n] = codes
    if pad_rng is not None and 4 * stride > n:
        full[n:] = pad_rng.integers(0, 4, size=(4 * stride - n, p), dtype=np.uint8)
    quad = full.reshape(stride, 4, p)
    blocks = (quad[:, 0] | (quad[:, 1] << 2) | (quad[:, 2] << 4) | (quad[:, 3] << 6)).astype(np.uint8)   # stride x p
    return bytes([0x6C, 0x1B, 0x01]) + np.ascontiguousarray(blocks.T).tobytes()


def write_fileset(prefix, G_a1, snp_ids=None, sample_ids=None, pad_rng=None):
    """Writes prefix.bed / .bim / .fam for the A1 dosages G_a1 (n x p, NA = missing); returns (snp_ids, sample_ids)."""
    G_a1 = np.asarray(G_a1)
    n, p = G_a1.shape
    snp_ids = [f"rs{1000 + 7 * j}" for j in range(p)] if snp_ids is None else list(snp_ids)
    sample_ids = [f"ind{i + 1}" for i in range(n)] if sample_ids is None else list(sample_ids)
    prefix = str(prefix)
    with open(prefix + ".bed", "wb") as f:
        f.write(pack_bed(G_a1, pad_rng))
    with open(prefix + ".bim", "w") as f:
        for j, rs in enumerate(snp_ids):
            f.write(f"{1 + j % 22}\t{rs}\t0\t{10000 + 13 * j}\t{'ACGT'[j % 4]}\t{'CGTA'[j % 4]}\n")
    with open(prefix + ".fam", "w") as f:
        for i, iid in enumerate(sample_ids):
            f.write(f"fam{i // 3 + 1} {iid} 0 0 {1 + i % 2} -9\n")
    return snp_ids, sample_ids
