"""The conditional cis scan restated for the tests, independent of atlasqtl_amd: the statistic of aq_prep_cis_cond in
np.longdouble on a handle's own matrices (prep.X_host() and prep.Y, so that the preparation is not tested again), the
elementwise error bound of an fp64 evaluation, inputs to run it on, and the scan as the callable that
atlasqtl_amd.independent_signals_ takes.

Definition (include/atlasqtl_hip.h, aq_prep_cis_cond).  Complete Y only.  Xs and Yc are the prepared matrices of the handle,
centred and, with covariates, residualised; n_cov as in aq_prep_marginal.  Trait t has a conditioning list C_t of
0 <= k_t <= 4 distinct predictor indices in [0, p1), in the order given, independent of the trait's window.
  Basis.  Go through C_t in order.  v = Xs[:, c].  Project out the basis vectors accepted so far, twice: in each of two
  passes, for every accepted q in the order of acceptance, v <- v - q (q'v) (Gram-Schmidt with one re-orthogonalisation).
  If |v|^2 <= 1e-10 |Xs[:, c]|^2 the column is dropped: a conditioning variant collinear with the earlier ones.  Otherwise
  q = v / |v| is accepted.  k_eff[t] is the number accepted.
  Residual trait.  y~_t = y_t - sum_j q_tj (q_tj' y_t), S~yy_t = sum y~^2.  With k_eff = 0, y~_t is the copy of y_t.
  Per pair with s_lo[t] <= s < s_hi[t]:  a_j = q_tj' x_s;  Vx = (Sxx - Sx^2 / n) - (a_1^2 + ... + a_k^2), the parenthesis
  evaluated first, exactly as the plain scan does;  r = (x_s' y~_t) / sqrt(Vx S~yy_t);  df_t = n - 2 - n_cov - k_eff[t].
  Undefined pairs.  A pair is undefined when Vx <= 1e-10 Sxx, when S~yy_t <= 1e-10 Syy_t, or when df_t < 1.  Its r is NaN;
  it is counted and never selected.  The first condition removes each conditioning variant from its own trait's tests, and
  anything collinear with the list."""
import numpy as np

from tests import mscreen_util as MU

LD = MU.LD
U = MU.U
KMAX = 4


def basis(Xl, cols):
    """(Q [n x k_eff, long double], accepted [the entries of cols that were kept]) by the definition above."""
    n = Xl.shape[0]
    qs, kept = [], []
    for c in cols:
        v = Xl[:, c].copy()
        norm0 = (v * v).sum()
        for _ in range(2):
            for qv in qs:
                v = v - qv * (qv @ v)
        nv = (v * v).sum()
        if nv <= LD(1e-10) * norm0:
            continue
        qs.append(v / np.sqrt(nv))
        kept.append(int(c))
    Q = np.stack(qs, axis=1) if qs else np.zeros((n, 0), dtype=LD)
    return Q, kept


def reference(Xs, Yc, lo, hi, cond, n_cov=0):
    """dict(r [p x q long double; NaN where the pair is undefined or outside the window], bound [p x q], inside [p x q bool],
    defined [p x q bool], ratio [p x q: Vx / Sxx of the in-window pairs, NaN outside], k_eff [q], df [q], syy_ratio [q]).

    bound, to first order in u = 2^-53, for an evaluation that forms every length-n sum in fp64 in any order with one rounding
    per term -- each such sum is within e sum |terms| of the exact sum of ITS OWN terms, e = (n + 2) u, the form of
    mscreen_util.reference -- and builds the basis by the two-pass Gram-Schmidt of the definition:
      the basis.  One projection step v <- v - q (q'v) commits at most (n + 4) u |v| (the dot, e |q| |v| <= e |v|, times |q| = 1,
        and the two roundings of the update); column j goes through 2 (j - 1) <= 2 (k - 1) steps and one normalisation
        (<= (n + 4) u as well), so the computed Q^ R^ reproduces every accepted column c_j within g |c_j|, g = (2 k - 1) (n + 4) u,
        and Q^ is orthonormal to the same order.  With the accepted columns scaled to unit length, C1, this is a perturbation
        of C1 of Frobenius norm <= sqrt(k) g, which turns its column space by sin(theta) <= sqrt(k) g / sigma_min(C1); the
        projector onto it, P = Q Q', moves by that much in the 2-norm, and Q^ Q^' differs from the projector onto span(Q^)
        by the loss of orthogonality, of the same order:   eP = 2 sqrt(k) g / sigma_min(C1)   (0 for k = 0).
      the residual trait.  y~^ = y - sum q^_j d^_j with k dots (each within e |y|) and k updates:
        |y~^ - y~| <= ey |y|,   ey = eP + k (n + 4) u.
      the sums.   dN    <= e sum |x| |y~| + sqrt(Sxx) ey sqrt(Syy)                 (Cauchy-Schwarz on x'(y~^ - y~))
                  dS~yy <= e S~yy + 2 sqrt(S~yy Syy) ey
                  dVx   <= e Sxx + 2 |Sx| e sum |x| / n + sum_j 2 |a_j| e sum |q_j| |x| + eP Sxx
        the last term being x'(Q^ Q^' - P) x; divided by Vx below it carries the factor Sxx / Vx by which a predictor in LD
        with the list loses accuracy.
      r = N (Vx S~yy)^(-1/2):   dr <= dN / sqrt(Vx S~yy) + |r| / 2 (dVx / Vx + dS~yy / S~yy),   times mscreen_util.FACTOR
        (the epilogue's few roundings and second-order terms).
    With k = 0 this is the bound of mscreen_util.reference."""
    Xl = np.asarray(Xs, dtype=LD)
    Yl = np.asarray(Yc, dtype=LD)
    n, p = Xl.shape
    q = Yl.shape[1]
    assert not np.isnan(np.asarray(Yc, dtype=np.float64)).any()
    r = np.full((p, q), np.nan, dtype=LD)
    B = np.full((p, q), np.nan, dtype=LD)
    ratio = np.full((p, q), np.nan)
    inside = np.zeros((p, q), dtype=bool)
    defined = np.zeros((p, q), dtype=bool)
    k_eff = np.zeros(q, dtype=np.int32)
    df = np.zeros(q, dtype=np.int64)
    syy_ratio = np.ones(q)
    e = LD((n + 2) * U)
    aX = np.abs(Xl)
    for t in range(q):
        a, b = int(lo[t]), int(hi[t])
        df[t] = n - 2 - n_cov                                  # k_eff is reported 0 for a trait with an empty window
        if b <= a:
            continue
        inside[a:b, t] = True
        Q, kept = basis(Xl, cond[t])
        k = len(kept)
        k_eff[t] = k
        df[t] = n - 2 - n_cov - k
        y = Yl[:, t]
        syy0 = (y * y).sum()
        yt = y - Q @ (Q.T @ y) if k else y.copy()
        syy = (yt * yt).sum()
        eP = LD(0)
        if k:
            C1 = np.asarray(Xs, dtype=np.float64)[:, kept]
            C1 = C1 / np.sqrt((C1 * C1).sum(axis=0))
            smin = float(np.linalg.svd(C1, compute_uv=False)[-1])
            eP = LD(2.0 * np.sqrt(k) * (2 * k - 1) * (n + 4) * U / smin)
        ey = eP + LD(k * (n + 4) * U)
        x, ax = Xl[:, a:b], aX[:, a:b]
        sxy, axy = yt @ x, np.abs(yt) @ ax
        sx, asx = x.sum(axis=0), ax.sum(axis=0)
        sxx = (x * x).sum(axis=0)
        aj = Q.T @ x                                           # k x w
        lost = (aj * aj).sum(axis=0)
        vx = (sxx - sx * sx / LD(n)) - lost
        syy_ratio[t] = float(syy / syy0) if syy0 > 0 else 0.0
        ok = (vx > LD(1e-10) * sxx) & (syy > LD(1e-10) * syy0) & (df[t] >= 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio[a:b, t] = (vx / sxx).astype(np.float64)
            den = np.sqrt(vx * syy)
            rt = sxy / den
            dn = e * axy + np.sqrt(sxx) * ey * np.sqrt(syy0)
            dsyy = e * syy + 2 * np.sqrt(syy * syy0) * ey
            dvx = e * sxx + 2 * np.abs(sx) * e * asx / LD(n) + (2 * np.abs(aj) * (e * (np.abs(Q).T @ ax))).sum(axis=0) + eP * sxx
            bt = dn / den + np.abs(rt) / 2 * (dvx / vx + dsyy / syy)
        r[a:b, t][ok] = rt[ok]
        B[a:b, t][ok] = LD(MU.FACTOR) * bt[ok]
        defined[a:b, t] = ok
    return dict(r=r, bound=B, inside=inside, defined=defined, ratio=ratio, k_eff=k_eff, df=df, syy_ratio=syy_ratio)


def thresholds_are_clear(ref):
    """No in-window pair sits near the 1e-10 rule: Vx / Sxx is < 1e-13 or > 1e-6 for every one of them, and S~yy / Syy > 1e-6."""
    v = ref["ratio"][ref["inside"]]
    return bool(np.all((v < 1e-13) | (v > 1e-6))) and bool(np.all(ref["syy_ratio"] > 1e-6))


def best(ref):
    """(best_snp [q, -1: none], clear [q bool]): the reference's best predictor per trait (the lowest index of the largest
    r^2) and whether it is clear of every other pair of the trait by the bound: |r_best| - bound_best > |r_s| + bound_s."""
    r = np.abs(np.asarray(ref["r"], dtype=np.float64))
    b = np.asarray(ref["bound"], dtype=np.float64)
    q = r.shape[1]
    bs, clear = np.full(q, -1, dtype=np.int32), np.zeros(q, dtype=bool)
    for t in range(q):
        d = np.nonzero(ref["defined"][:, t])[0]
        if d.size == 0:
            clear[t] = True
            continue
        i = d[int(np.argmax(r[d, t]))]
        bs[t] = i
        others = d[d != i]
        clear[t] = others.size == 0 or bool(r[i, t] - b[i, t] > np.max(r[others, t] + b[others, t]))
    return bs, clear


# ---- inputs ----
PATTERNS = ("all", "band")
LINCOMB = 2                 # predictor 2 = 0.6 predictor 0 - 0.8 predictor 1


def ld_matrix(rng, n, p, block=8):
    """n x p with LD blocks: within a block of `block` columns x_j = rho x_(j-1) + sqrt(1 - rho^2) z, rho^2 in [0.3, 0.9]."""
    X = rng.standard_normal((n, p))
    for j in range(1, p):
        if j % block:
            rho = np.sqrt(rng.uniform(0.3, 0.9)) * (1 if rng.random() < 0.8 else -1)
            X[:, j] = rho * X[:, j - 1] + np.sqrt(1 - rho * rho) * X[:, j]
    return X


def windows(pattern, p, q, seed=0):
    """(s_lo, s_hi) int32.  all: every window is [0, p).  band: seeded random windows; trait 0: [2, p), which holds its own
    conditioning variant 3; trait 1: [0, min(p, 40)), which holds predictor 2; trait 3: [p // 2, p), which leaves out its
    conditioning variant 0; trait 4, where there is one: empty."""
    lo, hi = np.zeros(q, dtype=np.int64), np.full(q, p, dtype=np.int64)
    if pattern == "band":
        rng = np.random.default_rng(1000 * seed + 7 * p + q)
        for t in range(q):
            a = int(rng.integers(0, p))
            lo[t], hi[t] = a, min(p, a + 1 + int(rng.integers(0, max(1, min(p, 90)))))
        lo[0], hi[0] = 2, p
        if q > 1:
            lo[1], hi[1] = 0, min(p, 40)
        if q > 3:
            lo[3], hi[3] = p // 2, p
        if q > 4:
            lo[4], hi[4] = 5, 5
    else:
        assert pattern == "all"
    return lo.astype(np.int32), hi.astype(np.int32)


def case(n, p, q, max_k, seed=0):
    """(X, Y, cond): raw inputs with LD blocks and planted per-trait effects, and conditioning lists whose longest has max_k
    entries (p >= 5), with what the tests look for planted:
      - predictor 2 = 0.6 x_0 - 0.8 x_1: a linear combination of the two conditioning variants of trait 1 (max_k >= 2), undefined
        there, and the third entry of the list [0, 1, 2] of trait 2 (max_k = 4), which must be dropped: k_eff = 2;
      - trait 0 conditions on the first max_k of [3, 4, 0, 1]: variant 3 lies inside its own window under both patterns;
      - trait 3 conditions on variant 0, outside its `band` window;
      - traits >= 4 have lists of every length, (max_k - t) mod (max_k + 1) entries drawn from the predictors >= 3; from trait 64
        on only t mod 2 entries, so that the trait tiles of one launch differ in their longest list.
    Trait t is 0.6 x (the first variant of its list, or predictor t mod p) + 0.5 x (predictor (3 t + 1) mod p) + noise."""
    assert p >= 5 and 1 <= max_k <= KMAX
    rng = np.random.default_rng(seed + 7919 * n + 31 * p + q + 1000003 * max_k)
    X = ld_matrix(rng, n, p)
    X[:, LINCOMB] = 0.6 * X[:, 0] - 0.8 * X[:, 1]
    cond = []
    for t in range(q):
        if t == 0:
            lst = [3, 4, 0, 1][:max_k]
        elif t == 1:
            lst = [0, 1][:min(max_k, 2)]
        elif t == 2 and max_k == KMAX:
            lst = [0, 1, LINCOMB]
        elif t == 3:
            lst = [0]
        else:
            k = (max_k - t) % (max_k + 1) if t < 64 else min(max_k, t % 2)
            k = min(k, p - 3)
            lst = [int(v) for v in 3 + rng.permutation(p - 3)[:k]]
        cond.append(lst)
    Y = rng.standard_normal((n, q))
    for t in range(q):
        first = cond[t][0] if cond[t] else t % p
        Y[:, t] += 0.6 * X[:, first] + 0.5 * X[:, (3 * t + 1) % p]
    return np.asfortranarray(X), np.asfortranarray(Y), cond


def prepared(X, Y):
    """What the preparation leaves of complete inputs without constant or duplicate columns, in numpy: the columns of X centred
    and scaled to n - 1 standard deviation 1, those of Y centred.  For choices made without a device; the GPU tests take the
    handle's own matrices."""
    Xs = (X - X.mean(axis=0)) / X.std(axis=0, ddof=1)
    return np.asfortranarray(Xs), np.asfortranarray(Y - Y.mean(axis=0))


# ---- a planted cohort for cis_independent ----
COHORT = dict(n=300, p=600, q=40, window=30_000, spacing=1000, seed=0, permutations={"n": 200, "seed": 1}, fdr=0.05)
COHORT_KINDS = ("two",) * 8 + ("proxy",) * 8 + ("weak",) * 4 + ("null",) * 20


def cohort(seed=COHORT["seed"]):
    """dict(X, Y, snp_chrom, snp_pos, trait_chrom, trait_start, kinds, planted): n = 300, p = 600 variants 1000 bp apart on one
    chromosome, q = 40 genes 15 kb apart, each with the ~61 variants within 30 kb in its window.  X is independent noise but for
    what is planted around every gene's position j:
      two     y = 0.55 x_(j - 7) + 0.45 x_(j + 9) + noise: two independent signals;
      proxy   y = 0.6 x_j + noise, and x_(j - 2), x_(j + 3), x_(j + 11) are proxies of x_j at r^2 ~ 0.8: one signal;
      weak    y = 0.3 x_j + noise: eGenes with one modest signal, which keep the thresholds from being those of the
              strongest genes alone;
      null    noise.
    planted: per gene the variants with an effect."""
    c = COHORT
    n, p, q = c["n"], c["p"], c["q"]
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    Y = rng.standard_normal((n, q))
    centre = 15 + 15 * np.arange(q)
    planted = []
    for t, kind in enumerate(COHORT_KINDS):
        j = int(centre[t])
        if kind == "two":
            Y[:, t] += 0.55 * X[:, j - 7] + 0.45 * X[:, j + 9]
            planted.append([j - 7, j + 9])
        elif kind == "proxy":
            for d in (-2, 3, 11):
                X[:, j + d] = np.sqrt(0.8) * X[:, j] + np.sqrt(0.2) * X[:, j + d]
            Y[:, t] += 0.6 * X[:, j]
            planted.append([j])
        elif kind == "weak":
            Y[:, t] += 0.3 * X[:, j]
            planted.append([j])
        else:
            planted.append([])
    return dict(X=np.asfortranarray(X), Y=np.asfortranarray(Y), snp_chrom=np.array(["1"] * p, dtype=object),
                snp_pos=c["spacing"] * np.arange(p), trait_chrom=["1"] * q, trait_start=c["spacing"] * centre, kinds=COHORT_KINDS,
                planted=planted)


def decisions_are_clear(log, threshold, factor=10.0):
    """Every accept / reject decision of a logged run of independent_signals_ (numpy_scan's log) is clear of its threshold by
    `factor` in p: p <= threshold / factor or p >= threshold factor, for every active trait of every scan (a trait without a
    defined pair is rejected whatever the threshold)."""
    for cond, active, bs, pv in log:
        for t in np.nonzero(active)[0]:
            if bs[t] >= 0 and not (pv[t] <= threshold[t] / factor or pv[t] >= threshold[t] * factor):
                return False
    return True


# ---- the reference scan as the callable of independent_signals_ ----
def numpy_scan(Xs, Yc, lo, hi, n_cov=0, log=None):
    """scan(cond, active) on the reference: best_snp, best_pvalue, best_r, df per trait; the traits that are not active get an
    empty window.  log, a list, receives (cond, active, best_snp, best_pvalue) of every call."""
    from scipy.stats import t as student
    lo, hi = np.asarray(lo), np.asarray(hi)
    q = np.asarray(Yc).shape[1]

    def scan(cond, active):
        active = np.asarray(active, dtype=bool)
        ref = reference(Xs, Yc, np.where(active, lo, 0), np.where(active, hi, 0), cond, n_cov)
        assert thresholds_are_clear(ref)
        bs, _ = best(ref)
        br, pv = np.full(q, np.nan), np.full(q, np.nan)
        for t in np.nonzero(bs >= 0)[0]:
            br[t] = float(ref["r"][bs[t], t])
            tt = br[t] * np.sqrt(ref["df"][t] / (1.0 - br[t] * br[t]))
            pv[t] = 2.0 * student.sf(abs(tt), ref["df"][t])
        if log is not None:
            log.append(([list(c) for c in cond], active.copy(), bs.copy(), pv.copy()))
        return dict(best_snp=bs, best_pvalue=pv, best_r=br, df=ref["df"])
    return scan
