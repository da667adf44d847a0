"""The truth for the transform_y tests: the definition of the rank-based inverse normal transform (include/atlasqtl_hip.h,
aq_rank_int) restated with scipy, independent of the library: scipy.stats.rankdata(method="average") on the observed rows of
each column, then scipy.special.ndtri.  The doubled ranks are exact integers, so the library's output can be recovered from
them by exact comparison; ndtri itself is the second, looser yardstick."""
import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

N_MAX = 82944
SHAPES = [(2, 3), (63, 5), (64, 5), (65, 5), (1000, 17), (1024, 4), (1025, 4), (16384, 2), (16385, 2), (20000, 3), (82944, 2)]


def ndtri_grid():
    """The points at which Phi^-1 is held to mpmath: 2001 linear in [1e-6, 0.5], the smallest argument of a Blom transform
    of m = 2 ... 82 944 observed values, and 0.5 itself."""
    return np.concatenate([np.linspace(1e-6, 0.5, 2001), [0.625 / (m + 0.25) for m in (2, 10, 100, 1000, N_MAX)], [0.5]])


def ndtri_mp(u):
    """Phi^-1(u) = sqrt(2) erfinv(2 u - 1) with 40 digits, rounded to fp64."""
    import mpmath as mp
    with mp.workdps(40):
        return np.array([float(mp.sqrt(2) * mp.erfinv(2 * mp.mpf(float(v)) - 1)) for v in np.asarray(u).ravel()])


def err_metric(got, ref):
    """max |err| / max(|ref|, 1): relative in the tails, absolute around 0."""
    return float(np.max(np.abs(np.asarray(got) - ref) / np.maximum(np.abs(ref), 1.0)))


def doubled_ranks(Y):
    """(t2, m): t2[i, k] = twice the average rank of Y[i, k] among the observed values of column k (0 where missing), as an
    exact integer; m[k] = the observed values of column k."""
    Y = np.asarray(Y, dtype=np.float64)
    t2 = np.zeros(Y.shape, dtype=np.int64)
    m = np.zeros(Y.shape[1], dtype=np.int64)
    for k in range(Y.shape[1]):
        obs = ~np.isnan(Y[:, k])
        m[k] = obs.sum()
        if m[k]:
            r2 = 2.0 * rankdata(Y[obs, k], method="average")
            assert np.all(r2 == np.round(r2))
            t2[obs, k] = r2.astype(np.int64)
    return t2, m


def folded_argument(t2, m, c):
    """(u, upper) per entry: u = (t - 2 c) / (2 m + 2 - 4 c) with t = min(2 r, 2 m + 2 - 2 r), the one fp64 division the
    kernel makes (u = 0.5 where missing), and whether the entry lies in the upper half (2 r > m + 1)."""
    mirror = 2 * m[None, :] + 2 - t2
    t = np.minimum(t2, mirror)
    u = (t.astype(np.float64) - 2.0 * c) / ((2 * m[None, :] + 2).astype(np.float64) - 4.0 * c)
    return np.where(t2 > 0, u, 0.5), t2 > mirror


def rank_int(Y, c=0.375):
    """The restatement: ndtri((r - c) / (m + 1 - 2 c)) over the observed rows, NaN where missing."""
    Y = np.asarray(Y, dtype=np.float64)
    out = np.full(Y.shape, np.nan)
    for k in range(Y.shape[1]):
        obs = ~np.isnan(Y[:, k])
        m = int(obs.sum())
        if m:
            out[obs, k] = ndtri((rankdata(Y[obs, k], method="average") - c) / (m + 1 - 2 * c))
    return out


def rank_int_folded(Y, c=0.375):
    """The restatement with ndtri asked only below 1/2: -+ ndtri((t - c) / (m + 1 - 2 c)) with t = min(r, m + 1 - r).  The same
    function at the same point, but free of the rounding of an argument next to 1 (argument_allowance)."""
    t2, m = doubled_ranks(Y)
    mirror = 2 * m[None, :] + 2 - t2
    t = np.minimum(t2, mirror) / 2.0
    with np.errstate(invalid="ignore"):
        x = ndtri((t - c) / (m[None, :] + 1 - 2 * c))
    return np.where(np.isnan(np.asarray(Y, dtype=np.float64)), np.nan, np.where(t2 > mirror, -x, x))


def argument_allowance(ref):
    """What rank_int() itself is off by, per entry, in the metric of err_metric: its argument u = (r - c) / (m + 1 - 2 c) is the
    fp64 result of two subtractions and a division, so it is within 3 x 2^-54 of the exact quotient wherever u >= 1/2 (half an
    ulp each, the ulp of [1/2, 1) being 2^-53), and Phi^-1 turns an error du of its argument into du / phi(x): 1.1e-12 at the top
    rank of 82 944 samples.  Below 1/2 the ulp shrinks with u, and the same reasoning gives at most 3 x 2^-54 u / phi(x) <= 2e-16
    there; both halves are covered by the formula for the upper one."""
    ref = np.asarray(ref, dtype=np.float64)
    phi = np.exp(-0.5 * ref * ref) / np.sqrt(2.0 * np.pi)
    return 3.0 * 2.0 ** -54 / (phi * np.maximum(np.abs(ref), 1.0))


def tied_counts(Y):
    """(n_obs, n_tied) per column with numpy: the observed values, and those that share their value with another one."""
    Y = np.asarray(Y, dtype=np.float64)
    n_obs = np.zeros(Y.shape[1], dtype=np.int64); n_tied = np.zeros(Y.shape[1], dtype=np.int64)
    for k in range(Y.shape[1]):
        v = Y[~np.isnan(Y[:, k]), k] + 0.0                   # -0.0 + 0.0 = +0.0: the two zeros are one value
        n_obs[k] = v.size
        _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
        n_tied[k] = int(np.sum(cnt[inv.reshape(-1)] > 1))
    return n_obs, n_tied


FIRST_SOURCE = {16384: 0, 16385: 2, 20000: 1, 82944: 3}     # the shapes with two or three columns still see all four sources


def columns(n, q, seed=0):
    """Y (n x q) whose columns cycle through the sources of the issue, starting at FIRST_SOURCE[n] (else at (a)): (a) continuous
    normals, (b) integers in 0 ... 6, (c) normals with -0.0, +0.0, a denormal and +-1e308 put in, (d) 10 % NaN at random.  With
    q >= 6 the last two columns are one with a single NaN block at the end and one with m = 2 observed values; with q = 5 the
    last column is the first of these for odd n, the second for even n.  Every column has two distinct observed values."""
    rng = np.random.default_rng(seed + 1000003 * n + q)
    Y = np.empty((n, q), order="F")
    for k in range(q):
        src = (k + FIRST_SOURCE.get(n, 0)) % 4
        col = rng.standard_normal(n)
        if src == 1:
            col = rng.integers(0, 7, n).astype(np.float64)
        elif src == 2:
            special = np.array([1e308, -0.0, 0.0, 5e-324, -1e308, 0.0, -0.0])
            idx = rng.permutation(n)[:min(n, special.size)]
            col[idx] = special[:idx.size]
        elif src == 3:
            col[rng.random(n) < 0.1] = np.nan
        if np.unique(col[~np.isnan(col)] + 0.0).size < 2:
            col[:2] = [1.0, -1.0]
        Y[:, k] = col

    def nan_block(k):
        Y[:, k] = rng.standard_normal(n)
        Y[n - n // 3:, k] = np.nan

    def two_observed(k):
        Y[:, k] = np.nan
        Y[rng.permutation(n)[:2], k] = [1.25, -3.0]

    if q >= 6:
        nan_block(q - 2)
        two_observed(q - 1)
    elif q == 5:
        (two_observed if n % 2 == 0 else nan_block)(q - 1)
    return Y
