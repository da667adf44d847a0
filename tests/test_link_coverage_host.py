"""CPU: the inputs of tests/test_gpu_link_range.py do what they claim -- on the oracle alone.

tests/util.make_link_problem lays theta_vb and zeta_vb out so that u = theta_j + zeta_k meets every table interval of the probit
link on both signs, the interval boundaries, +-12 and their floating-point neighbours, 0 and both tails, with helper waves
(16 SNPs x 16 traits) entirely inside the tables, mixed, and entirely outside.  These are conditions on the inputs: they are
asserted here for every distinct input the GPU file uses, so that an edit to the builder or to the case table cannot quietly
shrink what the GPU tests cover.  The state that goes into every later sweep comes from the oracle (run for 0 ... S - 1 sweeps)."""
import warnings

import numpy as np
import pytest

from tests import test_gpu_link_range as T
from tests.util import LINK_EDGES, LINK_GROUP, LINK_NI, LINK_R, LINK_W, link_interval, link_wave_classes, make_problem

INPUTS = sorted(T.all_inputs().items(), key=str)
EVERY = set(range(-LINK_NI - 1, LINK_NI + 2))            # signed classes: 0 (u = 0), +-1 ... +-24 (intervals), +-25 (tails)
STATE = ("theta_vb", "zeta_vb", "mu_beta_vb", "gam_vb", "beta_vb", "tau_vb", "lam2_inv_vb", "sig2_theta_vb", "sig2_beta_vb",
         "sig02_inv_vb", "sig2_inv_vb", "lb_opt")


def _id(item):
    (shape, na, axis, anneal, df, scheme, fine_scale), sweeps = item
    return f"n{shape[0]}-na{na}-{axis}-{anneal}-df{df}-{scheme}-f{fine_scale}"


def _c_of_sweep(anneal, k):
    """Inverse temperature of sweep k + 1."""
    from oracle import atlasqtl_oracle as O
    if anneal is None:
        return 1.0
    ladder = O.get_annealing_ladder_(anneal)
    return float(ladder[k]) if k < len(ladder) else 1.0


def _states(inputs, n_sweeps):
    """(theta, zeta) going into sweeps 1 ... n_sweeps, and the oracle's results after 1 ... n_sweeps sweeps."""
    from oracle import atlasqtl_oracle as O
    shape, na, axis, anneal, df, scheme, fine_scale = inputs
    prob = T.problem(inputs)
    li = prob["list_init"]
    states, results = [(np.asarray(li["theta_vb"]), np.asarray(li["zeta_vb"]))], []
    for k in range(1, n_sweeps + 1):
        r = O.atlasqtl_global_local_core_(prob["Y"], prob["X"], shape[2], anneal, df, 0.1, k, prob["list_hyper"], li,
                                          thinned_elbo_eval=False, debug=T.debug_of(inputs), full_output=True, scheme=scheme)
        results.append(r)
        states.append((r["theta_vb"], r["zeta_vb"]))
    return states[:n_sweeps], results


@pytest.mark.parametrize("item", INPUTS, ids=[_id(i) for i in INPUTS])
def test_builder_changes_theta_and_zeta_only(item):
    inputs, _ = item
    shape, na, axis = inputs[:3]
    prob = T.problem(inputs)
    base = make_problem(*shape, p_act=8, prob_assoc=0.3, na_frac=na)
    np.testing.assert_array_equal(prob["X"], base["X"])
    np.testing.assert_array_equal(prob["Y"], base["Y"])
    assert set(prob["list_init"]) == set(base["list_init"])
    for k, v in base["list_init"].items():
        if k not in ("theta_vb", "zeta_vb"):
            np.testing.assert_array_equal(np.asarray(prob["list_init"][k]), np.asarray(v), err_msg=k)
    for k, v in base["list_hyper"].items():
        np.testing.assert_array_equal(np.asarray(prob["list_hyper"][k]), np.asarray(v), err_msg=k)


@pytest.mark.parametrize("item", INPUTS, ids=[_id(i) for i in INPUTS])
def test_initial_u_covers_the_link(item):
    """The laid-out grid, as the first sweep reads it."""
    inputs, _ = item
    shape, na, axis, anneal, df, scheme, fine_scale = inputs
    li = T.problem(inputs)["list_init"]
    th, ze = np.asarray(li["theta_vb"]), np.asarray(li["zeta_vb"])
    small = th if axis == "zeta" else ze
    assert np.max(np.abs(small)) <= 0.5 * fine_scale
    u = th[:, None] + ze[None, :]
    sqrt_c = np.sqrt(_c_of_sweep(anneal, 0))
    # every interval on both signs, both tails, for A (at u) and for b and d (at sqrt(c) u)
    for x in (u, sqrt_c * u):
        hit = set(np.unique(link_interval(x)))
        if fine_scale == 1.0:
            assert hit >= EVERY - ({0} if sqrt_c != 1.0 else set()), sorted(EVERY - hit)
        else:
            # the shrunk fine part (df > 1: the reference's formulas allow no more) leaves gaps between neighbours of
            # the positive side's coarser grid: every negative-side interval and both tails still, and all but a few positive ones.
            # These cases run the same kernels as the full ones; what they add is the other p-vector update behind the same link.
            # (Of sqrt(c) u one interval on either side falls into a gap of the near tail as well.)
            if x is u:
                assert hit >= {i for i in EVERY if i < 0}, sorted(EVERY - hit)
            assert hit >= {-LINK_NI - 1, LINK_NI + 1} and len(EVERY - {0} - hit) <= 4, sorted(EVERY - hit)
    assert u.min() <= -38.0 and u.max() >= 38.0
    # most points inside [-13, 13], the negative side denser
    assert np.mean(np.abs(u) <= 13.0) > 0.5
    assert np.sum((u < 0) & (u >= -13.0)) > np.sum((u > 0) & (u <= 13.0))
    if fine_scale == 1.0:
        have = set(u.ravel().tolist())
        want = [k * LINK_W for k in range(-LINK_NI, LINK_NI + 1)]                      # every boundary k/2: 0 and +-12 among them
        want += [np.nextafter(s * e, t) for e in LINK_EDGES for s in (-1.0, 1.0) for t in (-np.inf, np.inf)]
        want += [np.nextafter(LINK_R, 0.0), np.nextafter(-LINK_R, 0.0)]
        missing = [w for w in want if float(w) not in have]
        assert not missing, missing
    # helper waves: a whole trait tile (spread in zeta) or SNP block (spread in theta) of each class
    cls = link_wave_classes(th, ze, sqrt_c)
    along = cls if axis == "zeta" else cls.T              # rows: the fine axis' groups, columns: the spread axis' groups
    full = (len(ze) if axis == "zeta" else len(th)) // LINK_GROUP
    for c, what in ((0, "inside"), (1, "mixed"), (2, "outside")):
        assert any(np.all(along[:, g] == c) for g in range(full)), f"no full group of the spread axis is {what} in every wave"
    # the upper half of the last interval, 11.75 <= |u| < 12, inside a wave that is not redone, on both signs (the first pass of the
    # look-ahead kernel clamped exactly these lanes to the interval's centre until this test existed)
    if fine_scale == 1.0:
        wave_of = cls[np.arange(len(th))[:, None] // LINK_GROUP, np.arange(len(ze))[None, :] // LINK_GROUP]
        for s in (-1.0, 1.0):
            assert np.any((wave_of == 0) & (s * u >= LINK_R - 0.5 * LINK_W) & (s * u < LINK_R)), s
    assert cls.shape[1 if axis == "zeta" else 0] >= 4 and (len(ze) if axis == "zeta" else len(th)) % LINK_GROUP != 0   # ragged end


@pytest.mark.parametrize("item", INPUTS, ids=[_id(i) for i in INPUTS])
def test_every_sweep_of_every_case_stays_spread_and_finite(item):
    """The state going into each sweep of each run of the GPU file: finite in the oracle, still on both tails and still with waves
    of all three classes; and the logit comparison of gam_vb keeps its coverage."""
    inputs, sweeps_list = item
    shape, na, axis, anneal, df, scheme, fine_scale = inputs
    n_max = max(T.maxit_of(inputs, s) for s in sweeps_list)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)         # a NaN or an overflow on the way is an error, not a warning
        warnings.filterwarnings("ignore", message="divide by zero encountered in log")      # (log of gam_vb = 0 in logit())
        states, results = _states(inputs, n_max)
    for k, ((th, ze), r) in enumerate(zip(states, results)):
        sqrt_c = np.sqrt(_c_of_sweep(anneal, k))
        u = th[:, None] + ze[None, :]
        hit = set(np.unique(link_interval(u)))
        assert {-LINK_NI - 1, LINK_NI + 1} <= hit, f"sweep {k + 1}: a tail is empty"
        cls = set(np.unique(link_wave_classes(th, ze, sqrt_c)))
        if k < 3:       # the 1- and 3-sweep runs: waves of all three classes in every sweep, a quarter of all u beyond the tables
            assert cls == {0, 1, 2}, f"sweep {k + 1}"
            assert np.mean(np.abs(u) >= LINK_R) > 0.25, f"sweep {k + 1}"
        else:           # the longer runs: the tails thin out, but every sweep still sends waves through the second pass
            assert 0 in cls and cls & {1, 2}, f"sweep {k + 1}"
        for f in STATE:
            if r.get(f) is not None and not (f == "lb_opt" and r[f] == -np.inf):
                assert np.all(np.isfinite(r[f])), f"sweep {k + 1}: {f} is not finite"
        if df > 1:
            # beyond, the reference's formulas for df > 1 cancel to noise, the annealed one soonest
            assert r["L_vb"].max() < (10.0 if anneal is not None else 20.0)
    for s in sweeps_list:
        m = T.maxit_of(inputs, s)
        th, ze = states[m - 1]
        with np.errstate(divide="ignore"):
            cov = T.logit_coverage(inputs, s, results[m - 1], th[:, None] + ze[None, :])
        assert T.coverage_holds(s, cov), (s, cov)
        if s == T.ELBO:
            assert sum(1 for r in results[:m] if np.isfinite(r["lb_opt"])) >= 1


def test_case_table_covers_the_instances_of_the_issue():
    """Plain-data check of the case table: every kernel, launch form, ladder, df and scheme it is meant to hold."""
    cases = T.CASES
    kern = {(e["core_kernel"], e["instance_flags"], e["split_parts"], e["tiles_per_group"], x.get("AQ_LA_XHELPER"))
            for (i, x, e) in cases.values()}
    for mask in (0, T.MASK):
        assert (0, mask, 1, 1, None) in kern and (0, mask | T.SEG, 1, 1, None) in kern
        for C in (2, 3):
            for xh in ("0", "1"):
                assert (0, mask, C, 1, xh) in kern
        assert any(k[0] == 0 and k[1] == (T.WIDE | mask) and k[2] >= 9 for k in kern)
    assert (0, 0, 1, 2, None) in kern
    assert {(2, False), (2, True), (3, True)} <= {(e["core_kernel"], i[1] > 0) for (i, x, e) in cases.values()}
    assert {None, (1, 2, 10), (2, 3, 5), (3, 2, 4)} <= {i[3] for (i, x, e) in cases.values()}
    assert {(3, True), (3, False), (5, False), (7, False)} <= {(i[4], i[3] is not None) for (i, x, e) in cases.values()}
    assert {("global", True), ("global", False)} <= {(i[5], i[3] is not None) for (i, x, e) in cases.values()}
    assert {"zeta", "theta"} <= {i[2] for (i, x, e) in cases.values() if i[3] is None}
    assert all(i[2] == "zeta" for (i, x, e) in cases.values() if i[3] is not None)      # annealed: the spread stays in zeta
    assert any(T.ELBO in T.sweep_counts(n) for n in cases)
