"""GPU: PLINK .bed input (aq_prepare_data_bed: the 2-bit genotypes are unpacked on the device) against the int8 / fp64 paths
of aq_prepare_data on the same dosages.  Both sides run the same device arithmetic on the same doubles, so every comparison
is exact (np.array_equal on bits): no tolerance.  The filesets are written by tests/bed_util.py with random padding bits."""
import io
import os

import numpy as np
import pytest

from tests import bed_util

pytestmark = pytest.mark.gpu

NA = bed_util.NA
TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plink_toy")
TOY_A1 = np.array([[2, 0, NA, 0, 0, 0], [0, NA, 1, 0, 0, 0], [0, 1, 1, NA, NA, 2]]).T      # 6 samples x 3 variants
REF_SENTENCE = "X must be a non-empty a numeric matrix, finite without missing value."


def _case(n, p, q, seed):
    """As tests/test_gpu_prepare.py::_case: two constant columns and three duplicates, one of them a third copy."""
    rng = np.random.default_rng(seed)
    maf = rng.uniform(0.05, 0.5, size=p)
    G = rng.binomial(2, maf[None, :], size=(n, p)).astype(np.int8)
    G[:, 3] = 1
    G[:, p - 2] = 2
    G[:, 7] = G[:, 1]
    G[:, p - 1] = G[:, 4]
    G[:, 11] = G[:, 1]
    return G, rng.normal(size=(n, q)), rng


def _counts(G_a1):
    """4 x p: homozygous A1, heterozygous, homozygous A2, missing, from A1 dosages."""
    return np.stack([(G_a1 == 2).sum(0), (G_a1 == 1).sum(0), (G_a1 == 0).sum(0), (G_a1 == NA).sum(0)]).astype(np.int32)


def _prepared(Y, X):
    """prepare_on_device(Y, X) brought to the host: (bool_cst, bool_coll, dup_of, standardised X, centred Y, counts)."""
    from atlasqtl_amd.prepare import prepare_on_device
    prep, cst, coll, dup = prepare_on_device(Y, X)
    try:
        return cst, coll, dup, prep.X_host(), prep.Y.copy(), prep.genotype_counts
    finally:
        prep.close()


def _assert_same_bits(got, want):
    for name, a, b in zip(("bool_cst", "bool_coll", "dup_of", "X", "Y"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                              b.view(np.uint64) if b.dtype == np.float64 else b), name


def test_toy_fixture_counts_and_error():
    from atlasqtl_amd import AtlasqtlError, PlinkBed
    Y = np.random.default_rng(0).normal(size=(6, 2))
    want = _counts(TOY_A1)
    assert want.tolist() == [[1, 0, 1], [0, 1, 2], [4, 4, 1], [1, 1, 2]]
    for count, G in (("A1", TOY_A1), ("A2", np.where(TOY_A1 == NA, NA, 2 - TOY_A1))):
        *_, Xs, _, counts = _prepared(Y, PlinkBed(TOY, count=count, missing="mean"))
        assert counts.dtype == np.int32 and counts.shape == (4, 3)
        np.testing.assert_array_equal(counts, want)                    # the counts are of genotypes, whichever allele is counted
        obs = np.where(G == NA, np.nan, G.astype(float))
        G_imp = np.where(G == NA, np.nansum(obs, 0) / (G != NA).sum(0), obs)
        _assert_same_bits(_prepared(Y, PlinkBed(TOY, count=count, missing="mean"))[:5], _prepared(Y, G_imp)[:5])
        assert Xs.shape == (6, 3)
    with pytest.raises(AtlasqtlError) as e:
        _prepared(Y, PlinkBed(TOY, missing="error"))
    msg = str(e.value)
    assert msg.startswith(REF_SENTENCE)
    assert "4 genotype(s) in 3 variant(s) are missing" in msg and "index 0" in msg and 'missing = "mean"' in msg
    with pytest.raises(AtlasqtlError, match="2 genotype.s. in 2 variant.s. are missing.*index 0"):
        _prepared(Y[:3], PlinkBed(TOY, samples=[0, 1, 2]))
    # the missing calls of rows 1, 2, 3, 4 are not among the rows used: nothing to refuse
    cst, *_ = _prepared(Y[:2], PlinkBed(TOY, samples=[5, 0], snps=[0, 2]))
    assert not cst.any()


@pytest.mark.parametrize("n,p,q", [(50, 16, 3), (203, 100, 7), (1001, 257, 5), (4099, 20000, 2)])
def test_bed_equals_int8_path(n, p, q, tmp_path):
    from atlasqtl_amd import PlinkBed
    G, Y, rng = _case(n, p, q, seed=n + p)
    snp_ids, _ = bed_util.write_fileset(tmp_path / "g", G, pad_rng=rng)
    want = _prepared(Y, G)
    assert want[5] is None
    got = _prepared(Y, PlinkBed(tmp_path / "g"))
    _assert_same_bits(got[:5], want[:5])
    assert set(np.where(got[1])[0]) == {7, 11, p - 1} and set(np.where(got[0])[0]) == {3, p - 2}
    assert got[2][7] == 1 and got[2][11] == 1 and got[2][p - 1] == 4
    np.testing.assert_array_equal(got[5], _counts(G))
    assert got[5][3].sum() == 0 and (got[5].sum(0) == n).all()
    if p < 20000:
        from oracle import prepare_oracle as PO
        Xs_ref, Yc_ref, cst_ref, coll_ref = PO.prepare_xy(Y, G.astype(np.float64))
        rm_ref = cst_ref.copy()
        rm_ref[~cst_ref] = coll_ref
        np.testing.assert_array_equal(got[0], cst_ref)
        np.testing.assert_array_equal(got[0] | got[1], rm_ref)
        np.testing.assert_allclose(got[3], Xs_ref, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(got[4], Yc_ref, rtol=1e-12, atol=1e-14)
    # the dosage of the other allele
    got2 = _prepared(Y, PlinkBed(tmp_path / "g", count="A2"))
    _assert_same_bits(got2[:5], _prepared(Y, (2 - G).astype(np.int8))[:5])
    np.testing.assert_array_equal(got2[5], got[5])
    # other padding bits (here: zero): nothing moves
    bed_util.write_fileset(tmp_path / "z", G, pad_rng=None)
    if n % 4:
        assert open(tmp_path / "z.bed", "rb").read() != open(tmp_path / "g.bed", "rb").read()
    _assert_same_bits(_prepared(Y, PlinkBed(tmp_path / "z"))[:5], want[:5])


@pytest.mark.parametrize("n_file,p_file", [(203, 120), (1001, 257)])
def test_selection_on_the_device(n_file, p_file, tmp_path):
    from atlasqtl_amd import PlinkBed
    G, _, rng = _case(n_file, p_file, 1, seed=3 * n_file)
    bed_util.write_fileset(tmp_path / "s", G, pad_rng=rng)
    perm = rng.permutation(n_file)
    subset = rng.permutation(n_file)[:int(0.6 * n_file)]
    idx = np.sort(rng.choice(p_file, size=p_file // 2, replace=False))
    for samples in (perm, subset):
        Y = rng.normal(size=(samples.size, 4))
        for snps, cols in ((slice(1, 90), np.arange(1, 90)), (idx, idx), (None, np.arange(p_file))):
            for count in ("A1", "A2"):
                Gs = np.ascontiguousarray(G[samples][:, cols])
                got = _prepared(Y, PlinkBed(tmp_path / "s", snps=snps, samples=samples, count=count))
                _assert_same_bits(got[:5], _prepared(Y, Gs if count == "A1" else (2 - Gs).astype(np.int8))[:5])
                np.testing.assert_array_equal(got[5], _counts(Gs))


@pytest.mark.parametrize("n,p,q,use_subset", [(203, 100, 7, False), (1001, 257, 5, False), (333, 64, 3, True)])
def test_missing_genotypes_take_the_mean(n, p, q, use_subset, tmp_path):
    from atlasqtl_amd import AtlasqtlError, PlinkBed
    G, _, rng = _case(n, p, q, seed=5 * n)
    G = G.astype(np.int64)
    samples = rng.permutation(n)[:int(0.6 * n)] if use_subset else None
    used = np.arange(n) if samples is None else samples
    G[rng.random(G.shape) < 0.03] = NA
    a, b, c = 20, 21, 22
    G[used, a] = NA                                       # missing in all rows used (observed in the others, if any)
    G[used, b] = NA
    G[used[5], b] = 1                                     # missing in all rows used but one
    G[used, c] = 2                                        # constant among its observed calls
    G[used[::7], c] = NA
    bed_util.write_fileset(tmp_path / "m", G, pad_rng=rng)
    Y = rng.normal(size=(used.size, q))
    Gu = G[used]
    for count in ("A1", "A2"):
        D = Gu if count == "A1" else np.where(Gu == NA, NA, 2 - Gu)
        n_het, n_hom, n_obs = (D == 1).sum(0), (D == 2).sum(0), (D != NA).sum(0)
        with np.errstate(invalid="ignore", divide="ignore"):
            fill = np.where(n_obs > 0, np.float64(n_het + 2 * n_hom) / np.float64(n_obs), 0.0)
        G_imp = np.where(D == NA, fill[None, :], D.astype(np.float64))
        got = _prepared(Y, PlinkBed(tmp_path / "m", samples=samples, count=count, missing="mean"))
        _assert_same_bits(got[:5], _prepared(Y, G_imp)[:5])
        assert got[0][a] and got[0][c] and got[0][b]       # all missing; constant among the observed; one observed call
        assert got[0][3] and got[0][p - 2]
        np.testing.assert_array_equal(got[5], _counts(Gu))
        assert got[5][3, a] == used.size and got[5][3, b] == used.size - 1
    n_mis, p_mis = int((Gu == NA).sum()), int((Gu == NA).any(0).sum())
    first = int(np.where((Gu == NA).any(0))[0][0])
    with pytest.raises(AtlasqtlError) as e:
        _prepared(Y, PlinkBed(tmp_path / "m", samples=samples))
    assert str(e.value).startswith(REF_SENTENCE)
    assert f"{n_mis} genotype(s) in {p_mis} variant(s) are missing" in str(e.value) and f"index {first} " in str(e.value)


def test_whole_run_from_a_fileset(tmp_path):
    import atlasqtl_amd as A
    from atlasqtl_amd import synth
    n, p, q = 203, 300, 20
    d = synth.simulate(n, p, q, p_act=10, seed=21, maf=0.25, prob_assoc=0.6)
    G = d["X"].astype(np.int8)
    act = [int(j) for j in d["act_x"] if j not in (40, 41, 250)]
    groups = [sorted([act[0], 40, 250]), sorted([act[1], 41])]      # copies of active predictors: removed, then added back
    for grp, src in zip(groups, act):
        G[:, grp] = d["X"][:, [src]]
    snp_ids = [f"rs{5000 + 3 * j}" for j in range(p)]
    snp_ids[17] = snp_ids[16] = "."                       # real .bim files hold "." IDs: made unique
    bed_util.write_fileset(tmp_path / "w", G, snp_ids=snp_ids, pad_rng=np.random.default_rng(2))
    names = list(snp_ids)
    names[17] = "..1"
    bed = A.PlinkBed(tmp_path / "w")
    assert bed.snp_names == names
    for sparse in (None, {"thres": 0.3}):
        kw = dict(p0=(3, 9), user_seed=7, verbose=0, add_collinear_back=True, sparse_output=sparse)
        a = A.atlasqtl(d["Y"], bed, **kw)
        b = A.atlasqtl(d["Y"], G, **kw)
        assert a.converged and a.it == b.it and a.lb_opt == b.lb_opt
        np.testing.assert_array_equal(a.theta_vb, b.theta_vb)
        np.testing.assert_array_equal(a.genotype_counts, _counts(G))
        assert "genotype_counts" not in b
        removed = {names[j] for grp in groups for j in grp[1:]}   # the first column of a group of copies is kept
        assert set(a.rmvd_coll_x) == removed
        assert all(a.rmvd_coll_x[names[j]] == names[grp[0]] for grp in groups for j in grp[1:])
        assert a.names_x == [nm for nm in names if nm not in removed] and a.rmvd_cst_x is None
        assert a.names_x_all == names and b.names_x_all == [f"Cov_x_{j + 1}" for j in range(p)]
        if sparse is None:
            np.testing.assert_array_equal(a.gam_vb, b.gam_vb)
            np.testing.assert_array_equal(a.beta_vb, b.beta_vb)
            assert a.gam_vb.shape == (p, q)
            sa, sb = A.summary(a, file=io.StringIO()), A.summary(b, file=io.StringIO())
            assert sa["top"] and [sz for _, sz in sa["top"]] == [sz for _, sz in sb["top"]]
            assert all(nm in names for nm, _ in sa["top"]) and all(nm.startswith("Cov_x_") for nm, _ in sb["top"])
            assert [nm for nm, _ in sa["top"]] == [names[int(nm[6:]) - 1] for nm, _ in sb["top"]]
            text = io.StringIO()
            A.summary(a, file=text)
            assert f"Top hotspots: \n{sa['top'][0][0]} (size {sa['top'][0][1]})" in text.getvalue()
        else:
            assert a.assoc["n_pairs"] == b.assoc["n_pairs"] > 0
            for k in ("snp", "trait", "ppi", "beta", "fdr"):
                np.testing.assert_array_equal(a.assoc[k], b.assoc[k])
            assert list(a.assoc["snp_name"]) == [names[j] for j in a.assoc["snp"]]
            assert not any(str(nm).startswith("Cov_x_") for nm in a.assoc["snp_name"])
            for grp in groups:                            # copies share their rows of the table
                assert len({names[j] in set(a.assoc["snp_name"]) for j in grp}) == 1
            np.testing.assert_array_equal(a.rs_thres, b.rs_thres)
