"""GPU: the radix select and moments of the p x q values (aq_order_stats / aq_vb_order_stats / aq_vb_radix_hist /
aq_vb_moments, VbRun.value_summary, value_summary) and summary() on top of them, against the restatement of
tests/test_summary_host.py: np.sort for order statistics, R's type-7 formula for quartiles, math.fsum for the sum.
Order statistics and quartiles are compared with ==; the mean, whose reduction order is the kernel's own, within
mean_bound (1e-13 sum|x| on the sum)."""
import ctypes as C
import io
import math

import numpy as np
import pytest

from tests.test_summary_host import assert_six_equal, value_families, wanted_ranks

pytestmark = pytest.mark.gpu

SIX = ("min", "q1", "median", "mean", "q3", "max")
I64P = C.POINTER(C.c_int64)


def _moments_dict(m):
    return {k: getattr(m, k) for k in ("count", "n_nan", "min", "max", "sum")}


def _check_sum(mom, x, what):
    v = np.asarray(x, dtype=np.float64).reshape(-1)
    v = v[~np.isnan(v)]
    err, bound = abs(mom["sum"] - math.fsum(v)), 1e-13 * math.fsum(np.abs(v))
    print(f"{what}: sum err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


def _array_order_stats(x, ranks):
    """aq_order_stats on the flattened array: (values at the ranks, moments)."""
    from atlasqtl_amd import _lib
    v = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    r = np.asarray(ranks, dtype=np.int64)
    out, mom = np.zeros(r.size), _lib.AqMoments()
    _lib.check(_lib.lib().aq_order_stats(_lib.as_dp(v), v.size, r.size, r.ctypes.data_as(I64P), _lib.as_dp(out), C.byref(mom), 0),
               "aq_order_stats")
    return out, _moments_dict(mom)


def _handle_order_stats(run, which, ranks):
    from atlasqtl_amd import _lib
    r = np.asarray(ranks, dtype=np.int64)
    out, mom = np.zeros(r.size), _lib.AqMoments()
    _lib.check(_lib.lib().aq_vb_order_stats(run.h, which, r.size, r.ctypes.data_as(I64P), _lib.as_dp(out), C.byref(mom)),
               "aq_vb_order_stats")
    return out, _moments_dict(mom)


def _check_handle(run, gam, beta, what):
    """Both value sources of a handle against the dense matrices they stand for."""
    for which, name, dense in ((0, "gam_vb", gam), (1, "beta_vb", beta)):
        s = np.sort(dense.reshape(-1))
        ranks = wanted_ranks(s.size)
        got, mom = _handle_order_stats(run, which, ranks)
        np.testing.assert_array_equal(got, s[ranks], err_msg=f"{what} {name}")
        assert (mom["count"], mom["n_nan"], mom["min"], mom["max"]) == (s.size, 0, s[0], s[-1]), (what, name, mom)
        _check_sum(mom, dense, f"{what} {name}")
        assert_six_equal(run.value_summary(name), dense, f"{what} {name}")


# ---- 5. the operator on host arrays ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (7, 3), (130, 49), (2000, 300)])
def test_operator_on_host_arrays_equals_sort(shape):
    import atlasqtl_amd as A
    n = shape[0] * shape[1]
    for name, flat in value_families(n).items():
        x = np.asfortranarray(flat.reshape(shape))
        s = np.sort(flat)
        ranks = wanted_ranks(n)
        got, mom = _array_order_stats(x, ranks)
        np.testing.assert_array_equal(got, s[ranks], err_msg=f"{shape} {name}")
        assert (mom["count"], mom["n_nan"], mom["min"], mom["max"]) == (n, 0, s[0], s[-1]), (shape, name, mom)
        _check_sum(mom, flat, f"{shape} {name}")
        assert_six_equal(A.value_summary(x), flat, f"{shape} {name}")
    if n > 5:
        # a few NaN are not values: counted, left out of the ranks and of the sum
        x = value_families(n)["ppi_x_normal"].copy()
        x[[0, n // 2, n - 1]] = np.nan
        six = A.value_summary(x.reshape(shape))
        assert six["n_nan"] == 3 and six["count"] == n - 3
        assert_six_equal(six, x, f"{shape} with NaN")
        # every rank of a short array in one call, equal ranks allowed
    x = value_families(12)["alphabet"]
    ranks = sorted(list(range(12)) + [0, 5, 11, 11])
    got, _ = _array_order_stats(x, ranks)
    np.testing.assert_array_equal(got, np.sort(x)[ranks])


def test_rank_beyond_the_count_is_an_argument_error():
    from atlasqtl_amd import _lib
    x = np.array([3.0, np.nan, 1.0, 2.0])
    out, mom = np.zeros(1), _lib.AqMoments()
    r = np.array([3], dtype=np.int64)                  # 3 values: ranks 0 ... 2
    assert _lib.lib().aq_order_stats(_lib.as_dp(x), 4, 1, r.ctypes.data_as(I64P), _lib.as_dp(out), C.byref(mom), 0) == 1
    assert b"aq_order_stats" in _lib.lib().aq_last_error()
    r[0] = 2
    assert _lib.lib().aq_order_stats(_lib.as_dp(x), 4, 1, r.ctypes.data_as(I64P), _lib.as_dp(out), C.byref(mom), 0) == 0
    assert out[0] == 3.0 and mom.count == 3 and mom.n_nan == 1


# ---- 6. the values resident in a handle --------------------------------------------------------------------------------
@pytest.mark.parametrize("na_frac", [0.0, 0.05])
def test_converged_run_equals_its_dense_result(na_frac):
    """p = 130 pads to 144 rows per tile, q = 49 leaves 15 padding traits in the last tile: none of them is a value."""
    from tests.test_gpu_associations import _converged_run
    run = _converged_run(na_frac)
    dense = run.result()
    assert dense["gam_vb"].shape == (130, 49)
    _check_handle(run, dense["gam_vb"], dense["beta_vb"], f"converged na {na_frac}")
    run.close()


def _planted_run(p_want, q, gam_of, n=100, p_act=6):
    """A handle whose resident gam_vb / mu_beta_vb are crafted initial values (no sweep has run)."""
    from atlasqtl_amd.core import VbRun
    from tests.util import make_problem
    prob = make_problem(n, p_want, q, p_act=p_act, prob_assoc=0.5)
    p = prob["p"]
    rng = np.random.default_rng(17)
    gam = np.asfortranarray(gam_of(rng, (p, q)))
    mu = np.asfortranarray(rng.standard_normal((p, q)))
    mu[rng.random((p, q)) < 0.2] = 0.0                # exact zeros and a tie block in beta
    li = dict(prob["list_init"])
    li["gam_vb"], li["mu_beta_vb"] = gam, mu
    run = VbRun(prob["Y"], prob["X"], prob["list_hyper"], li, None, 0.1, 5, True, False)
    run.run_sweeps(0)
    return run, gam, mu


def _tie_alphabet(rng, shape):
    return rng.choice([0.9995, 0.99, 0.9, 0.5, 0.01, 1e-4], size=shape, p=[0.02, 0.03, 0.05, 0.1, 0.3, 0.5])


def _all_positive(rng, shape):
    return 0.01 + 0.98 * rng.random(shape)


@pytest.mark.parametrize("craft", [_tie_alphabet, _all_positive])
def test_planted_values_and_padding_is_not_counted(craft):
    """gam everywhere positive with its minimum strictly above 0: a kernel that counts the zero padding rows / traits
    shows up as min == 0, a larger count and a shifted first quartile."""
    from atlasqtl_amd import _lib
    run, gam, mu = _planted_run(130, 49, craft)
    p, q = gam.shape
    assert p % 16 != 0 and q % 16 != 0 and gam.min() > 0
    got = run.result()
    np.testing.assert_array_equal(got["gam_vb"], gam)
    _check_handle(run, gam, gam * mu, craft.__name__)
    six = run.value_summary("gam_vb")
    assert six["min"] == gam.min() > 0 and six["count"] == p * q
    # two calls on one handle: identical bits, the sum included
    for which, name in ((0, "gam_vb"), (1, "beta_vb")):
        a, b = _lib.AqMoments(), _lib.AqMoments()
        assert _lib.lib().aq_vb_moments(run.h, which, C.byref(a)) == 0 and _lib.lib().aq_vb_moments(run.h, which, C.byref(b)) == 0
        assert bytes(a) == bytes(b)
        assert _handle_order_stats(run, which, [0, p * q - 1])[1] == _moments_dict(a)
        first, second = run.value_summary(name), run.value_summary(name)
        assert first == second and np.float64(first["mean"]).tobytes() == np.float64(second["mean"]).tobytes()
    # a rank is below the count; the count is the p q values, not the padded storage
    out, r = np.zeros(1), np.array([p * q], dtype=np.int64)
    assert _lib.lib().aq_vb_order_stats(run.h, 0, 1, r.ctypes.data_as(I64P), _lib.as_dp(out), None) == 1
    assert b"aq_vb_order_stats" in _lib.lib().aq_last_error()
    run.close()


def test_one_histogram_step_of_a_handle():
    """aq_vb_radix_hist, the primitive of the sharded driver: top digit, then two prefixes in one pass."""
    from atlasqtl_amd import _lib
    from tests.test_summary_host import keys_of
    run, gam, mu = _planted_run(130, 49, _tie_alphabet)
    for which, dense in ((0, gam), (1, gam * mu)):
        k = keys_of(dense.reshape(-1))
        hist = np.zeros((1, 256), dtype=np.int64)
        assert _lib.lib().aq_vb_radix_hist(run.h, which, 1, None, 56, hist.ctypes.data_as(I64P)) == 0
        np.testing.assert_array_equal(hist[0], np.bincount((k >> np.uint64(56)).astype(np.int64), minlength=256))
        pre = np.unique(k >> np.uint64(56))[:2]
        hist = np.zeros((pre.size, 256), dtype=np.int64)
        assert _lib.lib().aq_vb_radix_hist(run.h, which, pre.size, pre.ctypes.data_as(C.POINTER(C.c_uint64)), 48,
                                           hist.ctypes.data_as(I64P)) == 0
        for i, pf in enumerate(pre):
            sel = (k >> np.uint64(56)) == pf
            np.testing.assert_array_equal(hist[i], np.bincount(((k[sel] >> np.uint64(48)) & np.uint64(255)).astype(np.int64),
                                                               minlength=256))
        assert hist.sum() > 0
    run.close()


def test_expired_in_kernel_wait_is_reported():
    from atlasqtl_amd import _lib
    from tests.test_gpu_associations import _converged_run
    run = _converged_run()
    assert run.value_summary("gam_vb")["count"] == 130 * 49
    assert _lib.lib().aq_vb_debug_raise_errflag(run.h) == 0
    with pytest.raises(_lib.AtlasqtlHipError, match=r"\[2\].*bounded wait"):
        run.value_summary("gam_vb")
    mom = _lib.AqMoments()
    assert _lib.lib().aq_vb_moments(run.h, 1, C.byref(mom)) == 2
    run.close()


# ---- 7. several workgroups per digit, heavy contention on one bin ------------------------------------------------------
def test_five_million_values_over_65_tiles():
    def craft(rng, shape):
        g = rng.beta(0.05, 1.0, size=shape)
        u = rng.random(shape)
        g[u < 0.3] = 1e-4                              # tie blocks: whole waves on one bin down to the last digit
        g[u > 0.98] = 0.97
        return g
    run, gam, mu = _planted_run(5000, 1030, craft, p_act=10)
    p, q = gam.shape
    assert q == 1030 and p * q > 4_500_000 and (q + 15) // 16 == 65
    _check_handle(run, gam, gam * mu, f"p {p} q {q}")
    run.close()


# ---- 8. three trait shards ---------------------------------------------------------------------------------------------
def _summary_shard_worker(rank, world, port, outdir, ties):
    import os
    from tests.util import gloo_rank, shard_lists
    dist = gloo_rank(rank, world, port)
    from atlasqtl_amd.core import VbRun
    from tests.test_gpu_postproc import _fdr_problem
    prob, gam, cuts = _fdr_problem(ties)
    q = gam.shape[1]
    k0, k1 = cuts[rank], cuts[rank + 1]
    lh, li = shard_lists(prob["list_hyper"], prob["list_init"], k0, k1)
    li["gam_vb"] = np.asfortranarray(gam[:, k0:k1])
    run = VbRun(prob["Y"][:, k0:k1], prob["X"], lh, li, None, 0.1, 5, True, False, q_total=q, process_group=dist.group.WORLD,
                trait_offset=k0)
    run.run_sweeps(0)                       # the values resident on the device are the crafted initial values
    out = {}
    for name in ("gam_vb", "beta_vb"):
        six = run.value_summary(name)
        out[name] = np.array([six[k] for k in SIX])
        out[name + "_n"] = np.array([six["count"], six["n_nan"]])
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
    run.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("ties", [False, True])
def test_three_trait_shards_return_the_numbers_of_the_whole_matrix(ties, tmp_path):
    """Three processes on the one GPU over gloo, trait cuts [0, 16, 32, 50]: the shards' digit histograms add, so every
    rank's six numbers are those of the whole p x q matrix, and the ranks agree bit for bit."""
    from tests.test_gpu_postproc import _fdr_problem
    from tests.util import spawn_ranks
    spawn_ranks(_summary_shard_worker, 3, str(tmp_path), ties)
    prob, gam, _ = _fdr_problem(ties)
    beta = gam * np.asarray(prob["list_init"]["mu_beta_vb"])
    res = [np.load(tmp_path / f"rank{r}.npz") for r in range(3)]
    for name, dense in (("gam_vb", gam), ("beta_vb", beta)):
        for r in res:
            six = dict(zip(SIX, r[name].tolist()), count=int(r[name + "_n"][0]), n_nan=int(r[name + "_n"][1]))
            assert_six_equal(six, dense, f"ties {ties} {name}")
            assert r[name].tobytes() == res[0][name].tobytes()


# ---- 9. end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fdr,thres", [(False, 0.5), (True, 0.2)])
def test_summary_of_the_sparse_result_equals_summary_of_the_dense_result(fdr, thres):
    import atlasqtl_amd as A
    from tests.test_gpu_api import _data
    X, Y, _ = _data(100, 75, 20, seed=123)
    dense = A.atlasqtl(Y=Y, X=X, p0=(5, 25), user_seed=1, verbose=0)
    vb = A.atlasqtl(Y=Y, X=X, p0=(5, 25), user_seed=1, verbose=0,
                    sparse_output={"thres": thres, "fdr_adjust": fdr, "summary": True})
    pq = dense.p * dense.q
    assert not {"gam_vb", "beta_vb", "mu_beta_vb"} & set(vb)
    assert all(np.size(v) < pq for k, v in vb.items() if isinstance(v, np.ndarray))
    assert vb.sparse_output == {"thres": thres, "fdr_adjust": fdr, "max_pairs": None, "summary": True}
    for name in ("gam_vb", "beta_vb"):
        assert_six_equal(vb.value_summary[name], dense[name], f"sparse {name}")
    txt_d, txt_s = io.StringIO(), io.StringIO()
    out_d = A.summary(dense, thres=thres, fdr_adjust=fdr, file=txt_d)
    out_s = A.summary(vb, thres=thres, fdr_adjust=fdr, file=txt_s)
    print(txt_s.getvalue())
    assert set(out_d) == set(out_s) == {"gam_vb", "beta_vb", "theta_vb", "nb_pairwise", "n_active", "hotspot_sizes", "top",
                                        "rs_thres"}
    for name in ("gam_vb", "beta_vb"):
        for out in (out_d, out_s):
            assert_six_equal(dict(out[name], count=pq, n_nan=0), dense[name], f"summary() {name}")
        assert {k: v for k, v in out_d[name].items() if k != "mean"} == {k: v for k, v in out_s[name].items() if k != "mean"}
    assert out_d["theta_vb"] == out_s["theta_vb"] and out_d["hotspot_sizes"] == out_s["hotspot_sizes"]
    assert out_d["nb_pairwise"] == out_s["nb_pairwise"] == vb.assoc["n_pairs"] > 0
    assert out_d["n_active"] == out_s["n_active"] > 0 and out_d["top"] == out_s["top"]
    assert out_s["top"][0][0] in vb.names_x
    np.testing.assert_array_equal(out_d["rs_thres"], out_s["rs_thres"])
    assert txt_d.getvalue() == txt_s.getvalue()
    assert ("FDR control" if fdr else "PPI threshold") in txt_s.getvalue()
    # the matrices of a sparse run are gone: another threshold cannot be summarised, a run without "summary" neither
    with pytest.raises(ValueError, match="matrices are gone"):
        A.summary(vb, thres=thres / 2, fdr_adjust=fdr, file=io.StringIO())
    buf = io.StringIO()
    A.print_atlasqtl(vb, file=buf)
    assert f"Successful convergence after {vb.it} iterations" in buf.getvalue() and "(default)" in buf.getvalue()


def test_sparse_output_without_the_key_is_unchanged():
    import atlasqtl_amd as A
    from tests.test_gpu_api import _data
    X, Y, _ = _data(100, 75, 20, seed=123)
    vb = A.atlasqtl(Y=Y, X=X, p0=(5, 25), user_seed=1, verbose=0, sparse_output={"thres": 0.5})
    assert "value_summary" not in vb and "sparse_output" not in vb
    assert set(vb) == {"assoc", "rs_thres", "nb_pairwise", "theta_vb", "zeta_vb", "n", "p", "q", "anneal", "converged", "it",
                       "maxit", "tol", "lb_opt", "diff_lb", "p0", "rmvd_cst_x", "rmvd_coll_x", "names_x", "names_y"}
    with pytest.raises(ValueError, match="summary"):
        A.summary(vb, file=io.StringIO())
