"""summary.atlasqtl / print.atlasqtl (R/summarise_output.R:14-137) and the radix select behind the p q quartiles: the parts
that need no GPU -- the digit loop over histograms (trait shards summed), R's type-7 quartiles from order statistics,
argument errors of the C entries, and the printed text on hand-made results.

The expectations are restated here: np.sort for order statistics, the type-7 formula of stats::quantile.default for
quartiles, math.fsum for sums."""
import ctypes as C
import io
import math

import numpy as np
import pytest

from atlasqtl_amd import _lib

BITS = 8
QUARTILES = (("q1", 0.25), ("median", 0.5), ("q3", 0.75))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def keys_of(x):
    """Order-preserving map of IEEE doubles to uint64: negative -> all bits flipped, otherwise sign bit set."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def wanted_ranks(N):
    want = {0, N - 1}
    for _, prob in QUARTILES:
        index = (N - 1) * prob
        want.update((math.floor(index), math.ceil(index)))
    return sorted(want)


def expected_six(x):
    """R's summary.default on the non-NaN entries: sorted values, type-7 quartiles, fsum / N."""
    v = np.asarray(x, dtype=np.float64).reshape(-1)
    s = np.sort(v[~np.isnan(v)])
    N = s.size
    out = {"min": s[0], "max": s[-1], "mean": math.fsum(s) / N, "count": N, "n_nan": int(np.isnan(v).sum())}
    for name, prob in QUARTILES:
        index = (N - 1) * prob
        lo, hi = math.floor(index), math.ceil(index)
        qs = s[lo]
        if index > lo and s[hi] != qs:
            h = index - lo
            qs = (1 - h) * qs + h * s[hi]
        out[name] = qs
    return out


def mean_bound(x):
    """|sum_dev - fsum(x)| <= 1e-13 fsum(|x|), as a bound on the mean: about 30 x the worst case of a tree sum,
    log2(N) 2^-53 sum|x| with log2 N <= 32; a sum that loses more is serial or in reduced precision."""
    v = np.asarray(x, dtype=np.float64).reshape(-1)
    v = v[~np.isnan(v)]
    return 1e-13 * math.fsum(np.abs(v)) / v.size


def assert_six_equal(got, x, what=""):
    """Order statistics and quartiles exactly, counts exactly, the mean within mean_bound."""
    ref = expected_six(x)
    print(f"{what}: N {ref['count']} got {got} | mean err {abs(got['mean'] - ref['mean']):.3e} bound {mean_bound(x):.3e}")
    for k in ("min", "q1", "median", "q3", "max", "count", "n_nan"):
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    assert abs(got["mean"] - ref["mean"]) <= mean_bound(x), (what, got["mean"], ref["mean"], mean_bound(x))


def value_families(n, seed=3):
    """The arrays every select is tried on (n entries each; the constant and the alphabet are tie blocks)."""
    rng = np.random.default_rng(seed)
    ppi = rng.beta(0.05, 1.0, size=n)
    alphabet = np.array([0.0, -0.0, 5e-324, -1.5, 0.25, 0.9995])
    return {
        "ppi": ppi,
        "ppi_x_normal": ppi * rng.standard_normal(n),
        "alphabet": rng.choice(alphabet, size=n),
        "last_byte": 0.25 + rng.integers(0, 200, size=n) * 2.0 ** -54,
        "constant": np.full(n, 0.3),
    }


def sharded_hist_fn(x, cuts, calls=None):
    """hist_fn of radix_select_ from NumPy histograms of the keys, summed over the shards x[cuts[i]:cuts[i+1]]."""
    shards = [keys_of(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]

    def hist_fn(prefixes, shift):
        assert list(prefixes) == sorted(set(prefixes)) and 1 <= len(prefixes) <= 16
        if calls is not None:
            calls.append((list(prefixes), shift))
        out = np.zeros((len(prefixes), 1 << BITS), dtype=np.int64)
        for k in shards:
            digit = ((k >> np.uint64(shift)) & np.uint64((1 << BITS) - 1)).astype(np.int64)
            for i, pf in enumerate(prefixes):
                if shift + BITS >= 64:
                    sel = np.ones(k.size, dtype=bool)
                else:
                    sel = (k >> np.uint64(shift + BITS)) == np.uint64(pf)
                out[i] += np.bincount(digit[sel], minlength=1 << BITS)
        return out
    return hist_fn


# ---- 1. the digit loop -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 1000, 4099])
def test_radix_select_equals_sort_over_three_shards(n):
    from atlasqtl_amd.core import radix_select_
    for name, x in value_families(n).items():
        s = np.sort(x)
        for cuts in ([0, n // 5, n // 5, n], [0, n // 3, (2 * n) // 3, n]):      # one shard empty / three unequal shards
            calls = []
            ranks = wanted_ranks(n)
            got = radix_select_(sharded_hist_fn(x, cuts, calls), ranks, BITS)
            assert len(calls) == 64 // BITS and [c[1] for c in calls] == list(range(56, -1, -8))
            assert calls[0][0] == [0]
            for r, g in zip(ranks, got):
                assert g == s[r], (name, n, r, g, s[r])
        # every rank of a small array, duplicates among the ranks allowed
        if n <= 7:
            ranks = sorted(list(range(n)) + [0, n - 1])
            got = radix_select_(sharded_hist_fn(x, [0, 0, n, n]), ranks, BITS)
            assert got == [s[r] for r in ranks], name


def test_radix_select_last_digit_decides_and_signed_zero():
    from atlasqtl_amd.core import radix_select_
    x = 0.25 + np.arange(200)[::-1] * 2.0 ** -54
    got = radix_select_(sharded_hist_fn(x, [0, 10, 10, 200]), [0, 57, 199], BITS)
    assert got == [0.25, 0.25 + 57 * 2.0 ** -54, 0.25 + 199 * 2.0 ** -54]
    z = np.array([0.0, -0.0, 0.0, -0.0, 5e-324, -5e-324])
    got = radix_select_(sharded_hist_fn(z, [0, 2, 4, 6]), [0, 1, 2, 3, 4, 5], BITS)
    assert got == list(np.sort(z)) and math.copysign(1, got[1]) == -1 and math.copysign(1, got[4]) == 1


def test_radix_select_counts_beyond_32_bits():
    """Hand-made histograms: 3 * 2^32 values 0.25, 5 * 2^32 values 0.5, one value 1.0."""
    from atlasqtl_amd.core import radix_select_
    vals = {float(v): c for v, c in ((0.25, 3 << 32), (0.5, 5 << 32), (1.0, 1))}
    keys = {int(keys_of(np.array([v]))[0]): c for v, c in vals.items()}

    def hist_fn(prefixes, shift):
        out = np.zeros((len(prefixes), 256), dtype=np.int64)
        for i, pf in enumerate(prefixes):
            for k, c in keys.items():
                if shift + BITS >= 64 or (k >> (shift + BITS)) == pf:
                    out[i, (k >> shift) & 255] += c
        return out
    N = sum(vals.values())
    ranks = [0, (3 << 32) - 1, 3 << 32, (1 << 32) * 7 + 12345, N - 2, N - 1]
    assert radix_select_(hist_fn, ranks, BITS) == [0.25, 0.25, 0.5, 0.5, 0.5, 1.0]
    with pytest.raises(ValueError, match="not below"):
        radix_select_(hist_fn, [N], BITS)
    with pytest.raises(ValueError, match="ascending"):
        radix_select_(hist_fn, [5, 4], BITS)


# ---- 2. type-7 quartiles -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 9, 1000, 4099])
def test_product_quartiles_equal_the_restated_type7(n):
    from atlasqtl_amd.core import quantile_ranks_, six_numbers_, six_numbers_host_
    assert quantile_ranks_(n) == wanted_ranks(n) and len(quantile_ranks_(n)) <= 8
    for name, x in value_families(n).items():
        ref = expected_six(x)
        got = six_numbers_host_(x)
        assert got == {k: ref[k] for k in got}, (name, n)
        s = np.sort(x)
        again = six_numbers_(n, {r: s[r] for r in wanted_ranks(n)}, math.fsum(x))
        assert again == got


def test_type7_integer_index_and_equal_neighbours():
    from atlasqtl_amd.core import six_numbers_host_
    x = np.array([5.0, 1.0, 4.0, 2.0, 3.0])                     # (N - 1) prob = 1, 2, 3: the order statistics themselves
    got = six_numbers_host_(x)
    assert (got["q1"], got["median"], got["q3"]) == (2.0, 3.0, 4.0) and got["mean"] == 3.0
    x = np.array([1.0, 2.0, 4.0, 8.0])                          # index 0.75, 1.5, 2.25
    got = six_numbers_host_(x)
    assert (got["q1"], got["median"], got["q3"]) == (0.25 * 1.0 + 0.75 * 2.0, 3.0, 0.75 * 4.0 + 0.25 * 8.0)
    x = np.array([0.1, 0.1, 0.1, 0.7])                          # x[hi] == x[lo] at q1 and the median: no interpolation
    got = six_numbers_host_(x)
    assert got["q1"] == 0.1 and got["median"] == 0.1 and got["q3"] == (1 - 0.25) * 0.1 + 0.25 * 0.7
    with_nan = six_numbers_host_(np.array([np.nan, 2.0, 1.0, np.nan, 3.0]))
    assert with_nan["count"] == 3 and with_nan["n_nan"] == 2 and with_nan["median"] == 2.0


# ---- 3. argument errors need no device ---------------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_call(hiplib):
    ARG = 1
    i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))   # the handle is not looked at before the arguments are
    x = np.arange(5.0)
    out = np.full(4, -7.0)
    mom = _lib.AqMoments()
    mom.count = -5
    ranks = lambda *r: np.array(r, dtype=np.int64).ctypes.data_as(i64p)
    xs, outp = _lib.as_dp(x), _lib.as_dp(out)
    nul_d, nul_r = C.cast(None, _lib.dp), C.cast(None, i64p)

    op = hiplib.aq_order_stats
    assert op(nul_d, 5, 2, ranks(0, 4), outp, C.byref(mom), 0) == ARG
    assert op(xs, 0, 2, ranks(0, 4), outp, C.byref(mom), 0) == ARG
    assert op(xs, 5, 0, ranks(0, 4), outp, C.byref(mom), 0) == ARG
    assert op(xs, 5, 17, ranks(*range(17)), outp, C.byref(mom), 0) == ARG
    assert op(xs, 5, 2, ranks(4, 0), outp, C.byref(mom), 0) == ARG
    assert op(xs, 5, 2, ranks(-1, 3), outp, C.byref(mom), 0) == ARG
    assert op(xs, 5, 2, nul_r, outp, C.byref(mom), 0) == ARG
    assert op(xs, 5, 2, ranks(0, 4), nul_d, C.byref(mom), 0) == ARG
    assert b"aq_order_stats" in hiplib.aq_last_error()

    vb = hiplib.aq_vb_order_stats
    assert vb(None, 0, 2, ranks(0, 4), outp, C.byref(mom)) == ARG
    assert vb(fake, 2, 2, ranks(0, 4), outp, C.byref(mom)) == ARG
    assert vb(fake, -1, 2, ranks(0, 4), outp, C.byref(mom)) == ARG
    assert vb(fake, 0, 0, ranks(0, 4), outp, C.byref(mom)) == ARG
    assert vb(fake, 0, 17, ranks(*range(17)), outp, C.byref(mom)) == ARG
    assert vb(fake, 1, 2, ranks(4, 0), outp, C.byref(mom)) == ARG
    assert vb(fake, 1, 2, ranks(-2, 0), outp, C.byref(mom)) == ARG
    assert vb(fake, 1, 2, ranks(0, 4), nul_d, C.byref(mom)) == ARG
    assert b"aq_vb_order_stats" in hiplib.aq_last_error()

    assert hiplib.aq_vb_moments(None, 0, C.byref(mom)) == ARG
    assert hiplib.aq_vb_moments(fake, 2, C.byref(mom)) == ARG
    assert hiplib.aq_vb_moments(fake, 0, None) == ARG
    assert b"aq_vb_moments" in hiplib.aq_last_error()

    hist = np.full((16, 256), -3, dtype=np.int64)
    hp = hist.ctypes.data_as(i64p)
    pre = lambda *v: np.array(v, dtype=np.uint64).ctypes.data_as(u64p)
    rh = hiplib.aq_vb_radix_hist
    assert rh(None, 0, 1, pre(0), 56, hp) == ARG
    assert rh(fake, 2, 1, pre(0), 56, hp) == ARG
    assert rh(fake, 0, 0, pre(0), 48, hp) == ARG
    assert rh(fake, 0, 17, pre(*range(17)), 48, hp) == ARG
    assert rh(fake, 0, 2, pre(0, 1), 56, hp) == ARG              # the top digit has one (empty) prefix
    assert rh(fake, 0, 2, pre(3, 3), 48, hp) == ARG              # not strictly ascending
    assert rh(fake, 0, 2, pre(4, 3), 48, hp) == ARG
    assert rh(fake, 0, 1, C.cast(None, u64p), 48, hp) == ARG
    assert rh(fake, 0, 1, pre(0), 48, C.cast(None, i64p)) == ARG
    for shift in (-8, 4, 60, 64, 72):
        assert rh(fake, 0, 1, pre(0), shift, hp) == ARG
    assert b"aq_vb_radix_hist" in hiplib.aq_last_error()
    assert mom.count == -5 and np.all(out == -7.0) and np.all(hist == -3)


def test_valid_value_summary_call_needs_a_device(hiplib):
    """No quiet host path: without a HIP device the valid call fails loudly; with one it answers."""
    import atlasqtl_amd as A
    x = np.arange(12.0).reshape(4, 3)
    if hiplib.aq_device_count() > 0:
        assert A.value_summary(x)["median"] == 5.5
    else:
        with pytest.raises(_lib.AtlasqtlHipError, match="no HIP device"):
            A.value_summary(x)
    with pytest.raises(ValueError):
        A.value_summary(np.zeros((0, 3)))


# ---- 4. the printed summary --------------------------------------------------------------------------------------------
def _six(x):
    ref = expected_six(x)
    return {k: float(ref[k]) if k not in ("count", "n_nan") else ref[k] for k in ("min", "q1", "median", "mean", "q3", "max", "count", "n_nan")}


def sparse_result(rs_thres, thres=0.5, fdr_adjust=False, **over):
    """What atlasqtl(..., sparse_output={"thres": thres, "fdr_adjust": fdr_adjust, "summary": True}) returns, hand-made."""
    rng = np.random.default_rng(1)
    rs = np.asarray(rs_thres, dtype=np.int64)
    gam = rng.beta(0.05, 1.0, size=rs.size * 9)
    res = dict(theta_vb=rng.standard_normal(rs.size), zeta_vb=np.zeros(9), rs_thres=rs, nb_pairwise=int(rs.sum()),
               value_summary={"gam_vb": _six(gam), "beta_vb": _six(gam * rng.standard_normal(gam.size))},
               sparse_output={"thres": thres, "fdr_adjust": fdr_adjust, "max_pairs": None, "summary": True},
               names_x=[f"snp_{j}" for j in range(rs.size)], n=50, p=rs.size, q=9, p0=(2, 10), anneal=(1, 2, 10), tol=0.1, it=17,
               maxit=1000, diff_lb=0.01234, converged=True, lb_opt=-1.0)
    res.update(over)
    return res


BANNER = ("****************************************************** \n"
          "* ATLASQTL: posterior summary for variable selection *\n"
          "****************************************************** \n\n")
LABELS = ["Min.", "1st", "Qu.", "Median", "Mean", "3rd", "Qu.", "Max."]


@pytest.mark.parametrize("rs,top_lines", [
    ([0, 0, 0, 0], None),
    ([0, 4, 0, 2], "\nTop hotspots: \nsnp_1 (size 4), snp_3 (size 2). \n"),
    ([1, 0, 7, 1], "\nTop hotspots: \nsnp_2 (size 7), snp_0 (size 1), snp_3 (size 1). \n"),
    ([2, 9, 2, 0, 5, 2, 1, 3, 8], "\nTop hotspots: \nsnp_1 (size 9), snp_8 (size 8), snp_4 (size 5), \n"
                                  "snp_7 (size 3), snp_0 (size 2), snp_2 (size 2)"),
])
def test_summary_text_and_returned_dict(rs, top_lines):
    import atlasqtl_amd as A
    res = sparse_result(rs)
    buf = io.StringIO()
    out = A.summary(res, file=buf)
    txt = buf.getvalue()
    assert txt.startswith(BANNER)
    for s in ("Posterior probabilities pairwise association, pr(gamma_st = 1 | y)\n",
              "\nPosterior mean of pairwise regression coefficients, E(beta_st | y)\n",
              "\nPosterior mean of hotspot propensities, E(theta_s | y)\n ",
              "Using a PPI threshold of 0.5:\n------------------------------\n",
              f"\nNb of pairwise (predictor-response) associations: {sum(rs)} \n",
              "\nNb of predictors associated with at least one response \n"
              f"(active predictors): {sum(r > 0 for r in rs)} \n",
              "\nHotspot sizes (nb of responses associated with each \nactive predictor):\n"):
        assert s in txt, s
    assert [ln.split() for ln in txt.splitlines()].count(LABELS) == 4
    if top_lines is None:
        assert "Top hotspots" not in txt and out["top"] == [] and out["hotspot_sizes"] is None
        assert txt.rstrip().endswith("NA")
    else:
        assert txt.endswith(top_lines)
    rs = np.asarray(rs)
    n_top = min(6, int((rs > 0).sum()))
    order = np.argsort(-rs, kind="stable")[:n_top]
    assert out["top"] == [(f"snp_{j}", int(rs[j])) for j in order]
    assert out["nb_pairwise"] == rs.sum() and out["n_active"] == (rs > 0).sum()
    np.testing.assert_array_equal(out["rs_thres"], rs)
    six = ("min", "q1", "median", "mean", "q3", "max")
    for k in ("gam_vb", "beta_vb"):
        assert out[k] == {s: res["value_summary"][k][s] for s in six}
    ref = expected_six(res["theta_vb"])
    assert out["theta_vb"] == {s: ref[s] for s in six}
    if n_top:
        ref = expected_six(rs[rs > 0])
        assert out["hotspot_sizes"] == {s: ref[s] for s in six}
    # four significant digits under R's labels
    row = txt.splitlines()[txt.splitlines().index("Posterior probabilities pairwise association, pr(gamma_st = 1 | y)") + 2]
    assert [float(v) for v in row.split()] == [float(f"{res['value_summary']['gam_vb'][s]:.4g}") for s in six]


def test_summary_fdr_wording_and_short_form():
    import atlasqtl_amd as A
    res = sparse_result([0, 3, 1], thres=0.2, fdr_adjust=True)
    buf = io.StringIO()
    out = A.summary(res, thres=0.2, fdr_adjust=True, full_summary=False, file=buf)
    txt = buf.getvalue()
    assert txt.startswith(BANNER + "Using a 20% FDR control:\n-----------------------\n")
    assert "Posterior" not in txt and "PPI threshold" not in txt
    assert "gam_vb" not in out and "theta_vb" not in out and out["n_active"] == 2
    assert txt.endswith("\nTop hotspots: \nsnp_1 (size 3), snp_2 (size 1). \n")
    buf = io.StringIO()
    A.summary(sparse_result([1], thres=0.05, fdr_adjust=True), thres=0.05, fdr_adjust=True, file=buf)
    assert "Using a 5% FDR control:\n" in buf.getvalue()


def test_summary_prints_to_stdout_by_default(capsys):
    import atlasqtl_amd as A
    A.summary(sparse_result([2, 0]))
    assert capsys.readouterr().out.startswith(BANNER)


def test_summary_value_errors():
    import atlasqtl_amd as A
    res = sparse_result([0, 3, 1])
    plain = {k: v for k, v in res.items() if k not in ("value_summary", "sparse_output")}
    with pytest.raises(ValueError, match=r'sparse_output=\{.*"summary": True\}'):
        A.summary(plain, file=io.StringIO())
    with pytest.raises(ValueError, match="matrices are gone"):
        A.summary(res, thres=0.9, file=io.StringIO())
    with pytest.raises(ValueError, match="matrices are gone"):
        A.summary(res, thres=0.5, fdr_adjust=True, file=io.StringIO())
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((30, 8)), rng.standard_normal((30, 4))
    with pytest.raises(ValueError, match="summary"):
        A.atlasqtl(Y, X, (2, 4), verbose=0, add_collinear_back=True, sparse_output={"summary": True})
    from atlasqtl_amd.core import SPARSE_OUTPUT_DEFAULTS, sparse_output_options
    assert SPARSE_OUTPUT_DEFAULTS["summary"] is False
    assert sparse_output_options({"thres": 0.3}) == {"thres": 0.3, "fdr_adjust": False, "max_pairs": None, "summary": False}
    with pytest.raises(ValueError, match="'summary'"):
        sparse_output_options({"quartiles": True})


def test_print_atlasqtl_both_branches():
    import atlasqtl_amd as A

    def text(**over):
        buf = io.StringIO()
        A.print_atlasqtl(sparse_result([1, 0], **over), file=buf)
        return buf.getvalue()
    head = ("****************************************************** \n"
            "Successful convergence after 17 iterations, using a\n"
            "tolerance of 0.1 on the absolute changes in the ELBO.\n"
            "****************************************************** \n\n")
    body = ("Number of samples: 50;\n"
            "Number of (non-redundant) candidate predictors: 2;\n"
            "Number of responses: 9;\n"
            "Prior expectation for the number of predictors\n"
            "associated with each response: 2 (sd: 3.2).\n\n"
            "The posterior quantities inferred by ATLASQTL can\n"
            "be accessed as list elements from the `atlasqtl` S3\n"
            "object, and a summary can obtained using the\n"
            "`summary` function.\n\n")
    anneal = ("{} annealing on the inverse temperature was\n"
              "applied for the first {} iterations, with initial\n"
              "temperature of {}{}\n\n")
    assert text() == head + anneal.format("Geometric", 10, 2, " (default).") + body
    assert text(anneal=(2, 5, 20)) == head + anneal.format("Harmonic", 20, 5, ".") + body
    assert text(anneal=(3, 2.5, 10)) == head + anneal.format("Linear", 10, 2.5, ".") + body
    assert text(anneal=None) == head + body
    assert text(converged=False) == ("************************************************ \n"
                                     "Unsuccessful convergence after 1000 iterations. \n"
                                     "Difference between last two consecutive values\n"
                                     "of the ELBO: 0.0123.\n\n"
                                     "Try increasing:\n"
                                     "- the maximum number of iterations (maxit) or\n"
                                     "- the convergence threshold (tol). \n"
                                     "************************************************ \n\n")
    # AtlasqtlResult keeps the dict's own repr: nothing that existing code prints has changed
    from atlasqtl_amd.api import AtlasqtlResult
    assert repr(AtlasqtlResult(a=1)) == repr({"a": 1}) and str(AtlasqtlResult(a=1)) == str({"a": 1})
