"""GPU: the sweep kernels' probit link over all its table intervals and both tails, against the CPU oracle.

Every other whole-run parity test starts from make_problem's automatic init, where u = theta_j + zeta_k stays in about
[-2.7, -0.6]: five of the 24 table intervals, the negative side only, never the tail series, never the second pass of the
look-ahead kernel's helper wave (aq_core_sweep_la.h: `if (!__all(inr))` -> emit2, complete Y and MASK).  The cases below start
from tests/util.make_link_problem instead: u meets every interval on both signs, the boundaries k/2, +-12 and their
floating-point neighbours, 0, and the tails out to +-39; the helper waves of one launch are inside the tables, mixed and
outside them.  tests/test_link_coverage_host.py asserts, on the oracle alone, that the inputs of every case here do that.

Each case runs 1 and 3 sweeps (ELBO cases: the ladder and four ELBO evaluations, thinned_elbo_eval = False), proves the
launched kernel instance from aq_vb_status, and holds theta_vb, zeta_vb, mu_beta_vb, tau_vb, lam2_inv_vb, the ELBO trace and
gam_vb -- absolutely, and on the logit scale log g - log1p(-g) over the entries where the oracle's g is strictly inside
(0, 1): at u = -8 g is e^-34 and an absolute bar sees nothing -- to the bars below.  On the logit scale two units in the last
place of g are not counted (logit_grain): next to 1, and among the subnormal numbers, that is all a double carries of its logit.
The test counts, from the oracle alone, the compared entries that carry their logit in full, per negative-side table interval and
in the negative tail, and fails unless the comparison still covers them (coverage_holds).

What the file found when it was written, both fixed with it:
  * the first pass of the look-ahead kernel clamped t = 2 |u| at NI - 0.5, so in a wave that is not redone the lanes with
    11.75 <= |u| < 12 were evaluated at the centre of the last interval (gam_vb wrong by a factor of up to 4.7 where it is 1e-19);
    wide-c12 after 3 sweeps met such lanes (aq_core_sweep_la.h, locate; the grid now holds such lanes from the first sweep on);
  * aq_k_gram_blocks summed x_i' x_j over the samples in a plain running sum, about sqrt(n) ulp: with missing values the diagonal
    is X_norm_sq(j, k), and at n = 4000 mu_beta_vb was off by 5.7e-14 relative, tau_vb by 5.9e-15 and gam_vb by 1.9e-14 after
    one sweep -- the same figures for 12, 24, 48 parts and the medium split, so not an order effect of the split -- against a
    bar of 1.5e-14 (wide-c12-na); with compensated summation 5e-15, 6e-16 and 3e-15.

The bars come from the reference side only.  For every case, field and sweep count
    (a) the oracle as it is (SciPy log_ndtr, double-precision inv_mills_ratio_) against the same oracle with these two replaced
        by 40-digit mpmath evaluations rounded to double -- and with them the reference's formulas behind the same link that
        cancel in double: the annealed update of lam2_inv_vb (R/update_vb.R:70-81: for df = 1 a quotient near 1 less 1, about
        L_vb ulp, 6e-11 at L_vb = 590; for df = 3 about e^L_vb ulp) and compute_integral_hs_ for df = 5, 7, at 60 digits --, and
    (b) the oracle's Gram-space driver against its n-space form (oracle.sharded_oracle.run_sharded; it states the horseshoe with
        df = 1, so (b) covers those cases)
were measured on the CPU with
    python tests/tools/measure_link_bars.py
and the bar of a field is 10 x max(a, b) over all cases, capped by the bar the rest of the suite holds that field to (CAP).
MEASURED holds what that command printed: {sweeps: {field: (a, b)}}."""
import numpy as np
import pytest

from tests.test_gpu_split_instances import MASK, WIDE, SEG, _assert_instance

pytestmark = pytest.mark.gpu

ELBO = "elbo"        # the sweep count of an ELBO case: its ladder + ELBO_EVALS sweeps, every one of the latter with an ELBO
ELBO_EVALS = 4

# the bars of tests/test_gpu_parity.py::_check_state and the ELBO bar of the suite: upper caps, not loosened here
CAP = dict(theta_vb=1e-6, zeta_vb=1e-6, mu_beta_vb=1e-6, tau_vb=1e-8, lam2_inv_vb=1e-6, gam_vb=1e-8, gam_logit=np.inf, elbo=1e-5)
FLOOR = dict(theta_vb=1e-6, zeta_vb=1e-6, mu_beta_vb=1e-8, tau_vb=1e-8, lam2_inv_vb=1e-6)   # as _check_state

# python tests/tools/measure_link_bars.py  ->  (a), (b) per sweep count and field, maxima over all cases
MEASURED = {
    1: dict(theta_vb=(9.0e-10, 6.0e-13), zeta_vb=(4.2e-12, 4.1e-13), mu_beta_vb=(1.6e-11, 2.4e-10), tau_vb=(0.0e+00, 6.1e-16), lam2_inv_vb=(1.0e-09, 0.0e+00), gam_vb=(5.6e-16, 1.5e-15), gam_logit=(2.3e-13, 1.1e-13), elbo=(2.3e-12, 0.0e+00)),
    3: dict(theta_vb=(1.4e-09, 3.6e-11), zeta_vb=(6.1e-12, 6.7e-13), mu_beta_vb=(2.5e-10, 8.4e-11), tau_vb=(1.1e-13, 1.1e-14), lam2_inv_vb=(6.7e-10, 2.2e-10), gam_vb=(1.7e-12, 3.0e-13), gam_logit=(1.6e-10, 2.8e-11), elbo=(2.3e-12, 7.2e-15)),
    ELBO: dict(theta_vb=(1.1e-10, 6.0e-12), zeta_vb=(2.4e-12, 1.4e-13), mu_beta_vb=(4.9e-10, 5.2e-11), tau_vb=(2.9e-13, 1.6e-14), lam2_inv_vb=(1.9e-10, 1.8e-10), gam_vb=(1.7e-11, 9.0e-13), gam_logit=(4.7e-10, 2.5e-11), elbo=(1.0e-14, 5.6e-15)),
}


def bar(sweeps, field):
    a, b = MEASURED[sweeps][field]
    return min(10.0 * max(a, b), CAP[field])


# ------------------------------------------------------------------------------------------------------------------------------
# The cases: plain data.  inputs = (shape, na_frac, spread_axis, anneal, df, scheme, fine_scale); env = launch-plan hooks;
# expect = what aq_vb_status must report: core_kernel, instance_flags, split_parts, tiles_per_group, chain_segments and, for a
# sample split, the geometry (NT, NT2) of the parts.

SHAPE = (300, 130, 81)       # 19 sample tiles; 9 SNP blocks, the last of 2; 6 trait tiles, the last of 1
SHAPE_WIDE = (4000, 110, 81)
NA = 0.06
LADDER = (1, 2, 10)


def _inp(shape=SHAPE, na=0.0, axis="zeta", anneal=LADDER, df=1, scheme="global_local", fine_scale=1.0):
    return (shape, na, axis, anneal, df, scheme, fine_scale)


def _exp(kernel=0, flags=0, parts=1, tt=1, chain=0, geom=None):
    return dict(core_kernel=kernel, instance_flags=flags, split_parts=parts, tiles_per_group=tt, chain_segments=chain, geom=geom)


# n = 300 -> 19 sample tiles.  AQ_LA_C = 2: 10 per part -> the smallest geometry 3 (NT + NT2) >= 10 is 2 / 2; AQ_LA_C = 3: 7 per part
# -> 2 / 1 (aq_vb_create, "smallest geometry that holds ntiles").  n = 4000 in 12 parts: 21 per part -> 6 NT >= 21: NT = 4.
_SPLIT_FORMS = [(f"c{C}-x{x}", {"AQ_LA_C": str(C), "AQ_LA_XHELPER": str(x)}, C, geom)
                for C, geom in ((2, (2, 2)), (3, (2, 1))) for x in (0, 1)]

CASES = {}
# look-ahead kernel, complete Y
CASES["la-host"] = (_inp(), {}, _exp())
CASES["la-tt2"] = (_inp(), {"AQ_TT": "2"}, _exp(tt=2))
CASES["la-chain3"] = (_inp(), {"AQ_CHAIN": "3"}, _exp(flags=SEG, chain=3))
for name, env, C, geom in _SPLIT_FORMS:
    CASES[f"la-{name}"] = (_inp(), env, _exp(parts=C, geom=geom))
# look-ahead kernel, MASK (a MASK workgroup always holds one trait tile: there is no two-tile form)
CASES["mask-host"] = (_inp(na=NA), {}, _exp(flags=MASK))
CASES["mask-chain3"] = (_inp(na=NA), {"AQ_CHAIN": "3"}, _exp(flags=MASK | SEG, chain=3))
for name, env, C, geom in _SPLIT_FORMS:
    CASES[f"mask-{name}"] = (_inp(na=NA), env, _exp(flags=MASK, parts=C, geom=geom))
# wide split forced at moderate n
CASES["wide-c12"] = (_inp(shape=SHAPE_WIDE), {"AQ_LA_C": "12"}, _exp(flags=WIDE, parts=12, geom=(4, 4)))
CASES["wide-c12-na"] = (_inp(shape=SHAPE_WIDE, na=0.08), {"AQ_LA_C": "12"}, _exp(flags=WIDE | MASK, parts=12, geom=(4, 4)))
# the generic and the masked two-barrier kernel
CASES["generic"] = (_inp(), {"AQ_KERNEL": "2"}, _exp(kernel=2))
CASES["generic-na"] = (_inp(na=NA), {"AQ_KERNEL": "2"}, _exp(kernel=2))
CASES["masked-na"] = (_inp(na=NA), {"AQ_KERNEL": "3"}, _exp(kernel=3))
# ladders; without annealing also with the spread in theta (SNP blocks inside / mixed / outside)
CASES["noanneal-zeta"] = (_inp(anneal=None), {}, _exp())
CASES["noanneal-theta"] = (_inp(anneal=None, axis="theta"), {}, _exp())
CASES["noanneal-theta-na"] = (_inp(anneal=None, axis="theta", na=NA), {}, _exp(flags=MASK))
CASES["harmonic"] = (_inp(anneal=(2, 3, 5)), {}, _exp())
CASES["linear"] = (_inp(anneal=(3, 2, 4)), {}, _exp())
# degrees of freedom.  The reference's formulas for df > 1 lose digits to cancellation as L_vb (which grows like theta_j^2) grows:
# Kummer's 1F1 in the annealed update of lam2_inv_vb (R/update_vb.R:76-81) about e^L_vb ulp (noise from L_vb of about 20 on), the
# closed form for df = 3 (R/atlasqtl_global_local_core.R:258) about L_vb^2 ulp, the quotients of compute_integral_hs_ for df = 5, 7
# (R/utils.R:425-568) more; with theta in +-40 df = 7 is not finite in the oracle.  So for df > 1 the spread stays in zeta and
# |theta_j| is shrunk to 3/32, which keeps L_vb below 10: an oracle that is itself only good to 1e-6 could hold the link to nothing.
SMALL = 0.1875
CASES["df3-annealed"] = (_inp(df=3, fine_scale=SMALL), {}, _exp())
CASES["df3"] = (_inp(df=3, anneal=None, fine_scale=SMALL), {}, _exp())
CASES["df5"] = (_inp(df=5, anneal=None, fine_scale=SMALL), {}, _exp())
CASES["df7"] = (_inp(df=7, anneal=None, fine_scale=SMALL), {}, _exp())
# the global-only scheme
CASES["global-annealed"] = (_inp(scheme="global"), {}, _exp())
CASES["global-noanneal"] = (_inp(scheme="global", anneal=None), {}, _exp())      # (its one global scale pulls a spread in theta in)

# cases that also run to a handful of ELBO evaluations after the ladder, so that the ELBO pass sees the same u
ELBO_CASES = ("la-host", "noanneal-theta", "mask-host", "generic-na", "masked-na")


def sweep_counts(name):
    return (1, 3, ELBO) if name in ELBO_CASES else (1, 3)


def debug_of(inputs):
    """The reference checks that the ELBO does not decrease only under debug.  Its ELBO for df = 7 does decrease on these inputs (in
    the oracle: from +1.0e6 to -1.2e5 between the first two sweeps), so that case runs without the check, on both sides."""
    return inputs[4] != 7


def maxit_of(inputs, sweeps):
    anneal = inputs[3]
    return sweeps if sweeps != ELBO else (0 if anneal is None else int(anneal[2])) + ELBO_EVALS


def all_inputs():
    """The distinct inputs of the file with the sweep counts they run for (what the CPU-side checks and the measurement of the
    bars iterate over)."""
    out = {}
    for name, (inputs, env, expect) in CASES.items():
        out.setdefault(inputs, set()).update(sweep_counts(name))
    return {k: sorted(v, key=str) for k, v in out.items()}


_problems = {}


def problem(inputs):
    from tests.util import make_link_problem
    shape, na, axis, fine_scale = inputs[:3] + inputs[6:]
    key = (shape, na, axis, fine_scale)
    if key not in _problems:
        n, p, q = shape
        _problems[key] = make_link_problem(n, p, q, spread_axis=axis, fine_scale=fine_scale, p_act=8, prob_assoc=0.3, na_frac=na)
    return _problems[key]


def run_oracle(inputs, sweeps, O=None):
    """(result, ELBO trace) of the oracle's Gram-space driver for `sweeps` sweeps."""
    if O is None:
        from oracle import atlasqtl_oracle as O
    shape, na, axis, anneal, df, scheme, fine_scale = inputs
    prob = problem(inputs)
    tr = []
    ref = O.atlasqtl_global_local_core_(prob["Y"], prob["X"], shape[2], anneal, df, 0.1, maxit_of(inputs, sweeps), prob["list_hyper"],
                                        prob["list_init"], thinned_elbo_eval=sweeps != ELBO, debug=debug_of(inputs), trace=tr,
                                        full_output=True, scheme=scheme)
    return ref, np.array([r["lb"] for r in tr if r["lb"] is not None])


def logit(g):
    return np.log(g) - np.log1p(-g)


def compared(g_ref):
    """The entries of the logit comparison: the oracle's gam_vb strictly inside (0, 1)."""
    return (g_ref > 0.0) & (g_ref < 1.0)


def logit_grain(g):
    """What two units in the last place of the double g are worth on the logit scale (d logit / dg = 1 / (g (1 - g))): one unit for
    the last rounding of either side.  About 4e-16 / (1 - g) for a normal g; it takes over where a double cannot carry the logit
    -- g within a few ulp of 1 (u from about 8 on), and the subnormal g below 2.2e-308 (u below about -37)."""
    return 2.0 * np.spacing(g) / (g * (1.0 - g))


RESOLVED = 1e-15     # an entry whose logit_grain is below this carries its logit to full precision (every normal g <= 1/2 does)


def deviations(ref, lref, got, lgot):
    """Every compared field's deviation of `got` from `ref`, in the metric of its bar.  gam_logit: the largest excess of
    |logit(got) - logit(ref)| over logit_grain(ref) on the compared entries."""
    out = {}
    for f, floor in FLOOR.items():
        if ref.get(f) is None or got.get(f) is None:
            continue
        out[f] = float(np.max(np.abs(got[f] - ref[f]) / np.maximum(np.abs(ref[f]), floor)))
    out["gam_vb"] = float(np.max(np.abs(got["gam_vb"] - ref["gam_vb"])))
    m = compared(ref["gam_vb"])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = np.abs(logit(got["gam_vb"][m]) - logit(ref["gam_vb"][m])) - logit_grain(ref["gam_vb"][m])
    out["gam_logit"] = float(np.max(np.where(np.isnan(d), np.inf, np.maximum(d, 0.0))))
    if lref.size:
        out["elbo"] = float(np.max(np.abs(lgot - lref) / np.abs(lref))) if lgot.shape == lref.shape else np.inf
    return out


def logit_coverage(inputs, sweeps, ref, u_in):
    """How many compared entries that carry their logit to full precision each negative-side class holds: {signed interval: count}
    over -1 ... -(NI + 1), the last being the tail.  u_in is theta + zeta going into the last sweep, the u that the returned gam_vb
    was computed from."""
    from tests.util import link_interval, LINK_NI
    g = ref["gam_vb"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ok = compared(g) & (logit_grain(g) <= RESOLVED)
    idx = link_interval(u_in)[ok]
    return {-i: int(np.sum(idx == -i)) for i in range(1, LINK_NI + 2)}


def u_into_last_sweep(inputs, sweeps):
    """theta_j + zeta_k as the last of the sweeps reads it."""
    prob = problem(inputs)
    k = maxit_of(inputs, sweeps) - 1
    if k == 0:
        th, ze = prob["list_init"]["theta_vb"], prob["list_init"]["zeta_vb"]
    else:
        shape, na, axis, anneal, df, scheme, fine_scale = inputs
        from oracle import atlasqtl_oracle as O
        r = O.atlasqtl_global_local_core_(prob["Y"], prob["X"], shape[2], anneal, df, 0.1, k, prob["list_hyper"], prob["list_init"],
                                          thinned_elbo_eval=sweeps != ELBO, debug=debug_of(inputs), full_output=True, scheme=scheme)
        th, ze = r["theta_vb"], r["zeta_vb"]
    return np.asarray(th)[:, None] + np.asarray(ze)[None, :]


MIN_COMPARED = 8     # compared entries in every negative-side interval and in the negative tail
MIN_CLASSES_ELBO = 20


def coverage_holds(sweeps, cov):
    """The coverage condition of the logit comparison.  After 1 and 3 sweeps: at least MIN_COMPARED entries in every negative-side
    interval and in the negative tail.  An ELBO run is there for the ELBO pass, 8 to 14 sweeps on: by then the u of a trait's column
    have drawn together and where the columns lie is the model's doing, not the grid's -- the negative tail and at least
    MIN_CLASSES_ELBO of the 25 classes still hold MIN_COMPARED entries."""
    from tests.util import LINK_NI
    if sweeps != ELBO:
        return min(cov.values()) >= MIN_COMPARED
    return cov[-LINK_NI - 1] >= MIN_COMPARED and sum(v >= MIN_COMPARED for v in cov.values()) >= MIN_CLASSES_ELBO


def _prove_instance(run, expect, n):
    st = run.status()
    flags, parts = expect["instance_flags"], expect["split_parts"]
    assert st["core_kernel"] == expect["core_kernel"], st
    if expect["core_kernel"] != 0:
        return st
    if parts > 1:
        _assert_instance(run, flags, parts, *expect["geom"])
    got = {k: st[k] for k in ("instance_flags", "split_parts", "tiles_per_group", "chain_segments")}
    want = {k: expect[k] for k in got}
    assert got == want, f"the handle launches {got}, the case is written for {want}"
    assert st["n_pad"] >= n
    return st


@pytest.mark.parametrize("name,sweeps", [(name, s) for name in sorted(CASES) for s in sweep_counts(name)])
def test_link_range_matches_oracle(name, sweeps, monkeypatch):
    """Every run prints its deviations and their fractions of the bars before it asserts (pytest -s)."""
    from atlasqtl_amd.core import VbRun
    inputs, env, expect = CASES[name]
    shape, na, axis, anneal, df, scheme, fine_scale = inputs
    for k, v in env.items():
        monkeypatch.setenv(k, v)       # read by aq_vb_create
    prob = problem(inputs)
    ref, lref = run_oracle(inputs, sweeps)
    # the coverage condition of the logit comparison, from the oracle alone
    cov = logit_coverage(inputs, sweeps, ref, u_into_last_sweep(inputs, sweeps))
    assert coverage_holds(sweeps, cov), cov
    maxit = maxit_of(inputs, sweeps)
    run = VbRun(prob["Y"], prob["X"], prob["list_hyper"], prob["list_init"], anneal, 0.1, maxit, sweeps != ELBO, debug_of(inputs),
                scheme=scheme, df=df)
    try:
        st = _prove_instance(run, expect, shape[0])
        run.run()
        it = run.status()["it"]
        got = run.result(full_output=True)
        lgot = run.elbo_trace()[1]
    finally:
        run.close()
    assert it == ref["it"] == maxit
    if sweeps == ELBO:
        assert lref.size >= ELBO_EVALS      # (the last sweep of a ladder already runs at c = 1 and evaluates the ELBO too)
    dev = deviations(ref, lref, got, lgot)
    print(f"\nLINK case={name} sweeps={sweeps} kernel={st['core_kernel']} flags={st['instance_flags']} C={st['split_parts']} "
          f"TT={st['tiles_per_group']} chain={st['chain_segments']} NT={st['tiles_matrix']}/{st['tiles_matrix2']}/{st['tiles_recurrence']} "
          f"n_pad={st['n_pad']} compared={int(compared(ref['gam_vb']).sum())} "
          + " ".join(f"{f}={v:.3e}({v / bar(sweeps, f):.2f})" for f, v in dev.items()))
    for f in ("theta_vb", "zeta_vb", "mu_beta_vb", "tau_vb", "lam2_inv_vb", "gam_vb"):
        assert np.all(np.isfinite(got[f])), f
    assert lgot.shape == lref.shape
    over = {f: (v, bar(sweeps, f)) for f, v in dev.items() if not v <= bar(sweeps, f)}
    assert not over, f"beyond the bar (deviation, bar): {over}"
