"""The interaction cis scan restated for the tests, independent of atlasqtl_amd: the statistic of aq_prep_cis_int in
np.longdouble on a handle's own matrices (prep.X_host() and prep.Y, so that the preparation is not tested again), the
elementwise error bound of an fp64 evaluation, and inputs to run it on.

Definition (include/atlasqtl_hip.h, aq_prep_cis_int).  Complete Y only.  Xs [n x p] and Yc [n x q] are the handle's prepared
matrices.  B is nb orthonormal n-vectors spanning [1, Z, e], nb = n_cov + 2; m is the per-sample multiplier, e centred.
  Per trait t:      y' = y_t - sum_k b_k (b_k'y_t);  S'yy_t = sum y'^2;  S0yy_t = sum y_t^2.
  Per predictor s,  g = Xs[:, s], w = g o m:  a_k = b_k'g, c_k = b_k'w, Sxx = g'g, Sww = w'w, Vg = Sxx - sum a_k^2,
                    Cgw = g'w - sum a_k c_k, Vw = Sww - sum c_k^2 - Cgw^2 / Vg.
  Per in-window pair:  Sgy = g'y', Swy = w'y';  num = Swy - (Cgw / Vg) Sgy;  S'' = S'yy - Sgy^2 / Vg;  r = num / sqrt(Vw S'');
                    df = n - nb - 2.
  Undefined pairs.  Vg <= 1e-10 Sxx, Vw <= 1e-10 Sww, S'' <= 1e-10 S0yy_t, or df < 1."""
import numpy as np

from tests import ciscond_util as CU
from tests import mscreen_util as MU

LD = MU.LD
U = MU.U
PATTERNS = CU.PATTERNS
windows = CU.windows
best = CU.best                   # reads r, bound and defined of the dict below
E_KINDS = ("binary", "continuous")
EQ, ZERO, PLANT = 1, 2, 3        # the planted predictors of case(): equal to e; zero wherever e = 0; a true interaction with trait 0


def basis(e, Z=None):
    """(B [nb x n], m [n]): m = e centred, B the orthonormal rows of a QR factorisation of [1, Z, m].  An orthonormal basis of
    the span the definition asks for, computed without atlasqtl_amd."""
    e = np.asarray(e, dtype=np.float64)
    n = e.shape[0]
    m = e - e.mean()
    cols = [np.ones(n)] + ([] if Z is None else [np.asarray(Z, dtype=np.float64)[:, l] for l in range(np.shape(Z)[1])]) + [m]
    Q, _ = np.linalg.qr(np.stack(cols, axis=1))
    return np.ascontiguousarray(Q.T), m


def reference(Xs, Yc, lo, hi, B, m):
    """dict(r [p x q long double; NaN where the pair is undefined or outside the window], bound [p x q], inside, defined [p x q
    bool], vg_ratio [p: Vg / Sxx], vw_ratio [p: Vw / Sww, NaN where Vg fails its rule], s2_ratio [p x q: S'' / S0yy of the
    in-window pairs of a defined predictor, NaN elsewhere], pred_ok [p], int_tol [p long double, NaN where not pred_ok],
    tol_bound [p], df).

    bound, to first order in u = 2^-53, for an evaluation that forms every length-n sum in fp64 in any order with one rounding
    per term -- each such sum is within e sum |terms| of the exact sum of ITS OWN terms, e = (n + 2) u, the form of
    mscreen_util.reference -- and forms w = g o m with one rounding per element, so that a sum with one or two factors w is
    within ew sum |terms|, ew = (n + 4) u.  B and m are inputs: no error is committed on them.
      the residual trait.  y'^ = y - sum_k b_k d^_k with nb dot products (each within e |y|, |b_k| = 1) and nb updates:
        |y'^ - y'| <= ey |y|,   ey = nb (n + 4) u.
      per predictor, with A_k = sum |b_k| |g|, C_k = sum |b_k| |w| and ch = (nb + 4) u for the roundings of a chain of nb + 1
      terms, each no larger than the sum of the magnitudes:
        dVg  <= e Sxx + sum_k 2 |a_k| e A_k + ch (Sxx + sum a_k^2)
        dCgw <= ew sum |g| |w| + sum_k (|a_k| ew C_k + |c_k| e A_k) + ch (|g'w| + sum |a_k c_k|)
        d(Cgw / Vg) <= dCgw / Vg + |Cgw / Vg| dVg / Vg + u |Cgw / Vg|
        dVw  <= ew Sww + sum_k 2 |c_k| ew C_k + 2 |Cgw| dCgw / Vg + Cgw^2 dVg / Vg^2 + ch (Sww + sum c_k^2 + Cgw^2 / Vg)
      the last line carrying the cancellation in Vw: every term is absolute, none is relative to Vw itself.
      per pair:
        dSgy <= e sum |g| |y'| + sqrt(Sxx) ey sqrt(S0yy)                   (Cauchy-Schwarz on g'(y'^ - y'))
        dSwy <= ew sum |w| |y'| + sqrt(Sww) ey sqrt(S0yy)
        dS'yy <= e S'yy + 2 sqrt(S'yy S0yy) ey
        dnum <= dSwy + |Cgw / Vg| dSgy + |Sgy| d(Cgw / Vg) + u (|Swy| + |Cgw / Vg| |Sgy|)
        dS'' <= dS'yy + 2 |Sgy| dSgy / Vg + Sgy^2 dVg / Vg^2 + 3 u (S'yy + Sgy^2 / Vg)
      the cancellations in num and S'' carried the same way: dSwy and |Cgw / Vg| dSgy are of the size of |Swy| and
      |Cgw / Vg| |Sgy|, not of num.
      r = num (Vw S'')^(-1/2):   dr <= dnum / sqrt(Vw S'') + |r| / 2 (dVw / Vw + dS'' / S''),   times mscreen_util.FACTOR (the
      epilogue's few roundings and second-order terms).
      int_tol = Vw / Sww:   tol_bound = FACTOR (dVw / Sww + int_tol (ew + u))."""
    Xl = np.asarray(Xs, dtype=LD)
    Yl = np.asarray(Yc, dtype=LD)
    Bl = np.asarray(B, dtype=LD)
    ml = np.asarray(m, dtype=LD)
    n, p = Xl.shape
    q = Yl.shape[1]
    nb = Bl.shape[0]
    assert Bl.shape == (nb, n) and ml.shape == (n,) and not np.isnan(np.asarray(Yc, dtype=np.float64)).any()
    df = n - nb - 2
    e, ew, u = LD((n + 2) * U), LD((n + 4) * U), LD(U)
    ey, ch = LD(nb * (n + 4) * U), LD((nb + 4) * U)
    W = Xl * ml[:, None]
    aX, aW, aB = np.abs(Xl), np.abs(W), np.abs(Bl)
    A, Cc = Bl @ Xl, Bl @ W                                    # nb x p
    AA, CC = aB @ aX, aB @ aW
    sxx, sww, sgw, agw = (Xl * Xl).sum(axis=0), (W * W).sum(axis=0), (Xl * W).sum(axis=0), (aX * aW).sum(axis=0)
    sa2, sac, sc2, aac = (A * A).sum(axis=0), (A * Cc).sum(axis=0), (Cc * Cc).sum(axis=0), np.abs(A * Cc).sum(axis=0)
    vg = sxx - sa2
    cgw = sgw - sac
    g_ok = vg > LD(1e-10) * sxx
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        cgv = cgw / vg
        vw = sww - sc2 - cgw * cgw / vg
        dvg = e * sxx + (2 * np.abs(A) * e * AA).sum(axis=0) + ch * (sxx + sa2)
        dcgw = ew * agw + (np.abs(A) * ew * CC + np.abs(Cc) * e * AA).sum(axis=0) + ch * (np.abs(sgw) + aac)
        dcgv = dcgw / vg + np.abs(cgv) * dvg / vg + u * np.abs(cgv)
        dvw = (ew * sww + (2 * np.abs(Cc) * ew * CC).sum(axis=0) + 2 * np.abs(cgw) * dcgw / vg + cgw * cgw * dvg / (vg * vg)
               + ch * (sww + sc2 + cgw * cgw / vg))
        pred_ok = g_ok & (vw > LD(1e-10) * sww)
        vg_ratio = (vg / sxx).astype(np.float64)
        vw_ratio = np.where(g_ok, (vw / sww).astype(np.float64), np.nan)
        int_tol = np.where(pred_ok, vw / sww, LD(np.nan))
        tol_bound = np.where(pred_ok, LD(MU.FACTOR) * (dvw / sww + (vw / sww) * (ew + u)), LD(np.nan))
    r = np.full((p, q), np.nan, dtype=LD)
    bound = np.full((p, q), np.nan, dtype=LD)
    s2_ratio = np.full((p, q), np.nan)
    inside = np.zeros((p, q), dtype=bool)
    defined = np.zeros((p, q), dtype=bool)
    for t in range(q):
        a, b = int(lo[t]), int(hi[t])
        if b <= a:
            continue
        inside[a:b, t] = True
        y = Yl[:, t]
        syy0 = (y * y).sum()
        y1 = y - Bl.T @ (Bl @ y)
        s1 = (y1 * y1).sum()
        w = slice(a, b)
        sgy, swy = y1 @ Xl[:, w], y1 @ W[:, w]
        asgy, aswy = np.abs(y1) @ aX[:, w], np.abs(y1) @ aW[:, w]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            dsgy = e * asgy + np.sqrt(sxx[w]) * ey * np.sqrt(syy0)
            dswy = ew * aswy + np.sqrt(sww[w]) * ey * np.sqrt(syy0)
            ds1 = e * s1 + 2 * np.sqrt(s1 * syy0) * ey
            num = swy - cgv[w] * sgy
            dnum = dswy + np.abs(cgv[w]) * dsgy + np.abs(sgy) * dcgv[w] + u * (np.abs(swy) + np.abs(cgv[w] * sgy))
            s2 = s1 - sgy * sgy / vg[w]
            ds2 = ds1 + 2 * np.abs(sgy) * dsgy / vg[w] + sgy * sgy * dvg[w] / (vg[w] * vg[w]) + 3 * u * (s1 + sgy * sgy / vg[w])
            ok = pred_ok[w] & (s2 > LD(1e-10) * syy0) & (df >= 1)
            den = np.sqrt(vw[w] * s2)
            rt = num / den
            bt = dnum / den + np.abs(rt) / 2 * (dvw[w] / vw[w] + ds2 / s2)
            s2_ratio[w, t] = np.where(pred_ok[w], (s2 / syy0).astype(np.float64) if syy0 > 0 else 0.0, np.nan)
        r[w, t][ok] = rt[ok]
        bound[w, t][ok] = LD(MU.FACTOR) * bt[ok]
        defined[w, t] = ok
    return dict(r=r, bound=bound, inside=inside, defined=defined, vg_ratio=vg_ratio, vw_ratio=vw_ratio, s2_ratio=s2_ratio,
                pred_ok=pred_ok, int_tol=int_tol, tol_bound=tol_bound, df=df)


def thresholds_are_clear(ref):
    """No ratio sits near a 1e-10 rule, by the factor ciscond_util.thresholds_are_clear uses: Vg / Sxx and Vw / Sww of every
    predictor and S'' / S0yy of every in-window pair are < 1e-13 or > 1e-6."""
    def clear(v):
        v = np.asarray(v, dtype=np.float64)
        v = v[~np.isnan(v)]
        return bool(np.all((v < 1e-13) | (v > 1e-6)))
    return clear(ref["vg_ratio"]) and clear(ref["vw_ratio"]) and clear(ref["s2_ratio"][ref["inside"]])


def t_of(r, df):
    r = np.asarray(r, dtype=np.float64)
    return r * np.sqrt(df / (1.0 - r * r))


# ---- inputs ----
def case(n, p, q, d, kind, seed=0):
    """(X, Y, Z, e): raw inputs (p >= 5) with d covariates (Z is None for d = 0) and the interaction variable e, `binary`
    (0 / 1, about half each) or `continuous`, with what the tests look for planted:
      - predictor EQ equals e: collinear with [1, Z, e], so Vg fails its rule and every pair of it is undefined;
      - predictor ZERO = e o h, zero wherever e = 0.  With binary e and d = 0 the interaction term g o m is a linear combination
        of 1, e and g (e^2 = e), Vw fails its rule and every pair of it is undefined.  With covariates the prepared predictor is
        the residual of g on [1, Z], which is no longer zero where e = 0, and with continuous e there is no identity e^2 = e:
        the reference then decides, and its ratios are clear of the rule;
      - trait 0 = 0.3 x_PLANT + 1.5 x_PLANT o (e centred and scaled) + noise: a true interaction effect, inside the window of
        trait 0 under both patterns of ciscond_util.windows, whose r is clear of every other pair of the trait.
    The other predictors are standard normal; trait t has a main effect of predictor t mod p and of e, and no interaction."""
    assert p >= 5 and kind in E_KINDS and d >= 0
    rng = np.random.default_rng(seed + 7919 * n + 31 * p + q + 1000003 * d + (500009 if kind == "binary" else 0))
    X = rng.standard_normal((n, p))
    if kind == "binary":
        e = np.zeros(n)
        e[rng.permutation(n)[: n // 2]] = 1.0
    else:
        e = rng.standard_normal(n) + 0.5
    Z = rng.standard_normal((n, d)) if d else None
    X[:, EQ] = e
    X[:, ZERO] = e * (1.5 + rng.standard_normal(n))
    Y = rng.standard_normal((n, q))
    es = (e - e.mean()) / e.std()
    for t in range(q):
        Y[:, t] += 0.3 * X[:, t % p] + 0.4 * es
        if d:
            Y[:, t] += 0.3 * Z[:, t % d]
    Y[:, 0] = 0.5 * rng.standard_normal(n) + 0.3 * X[:, PLANT] + 1.5 * X[:, PLANT] * es + 0.4 * es
    return (np.asfortranarray(X), np.asfortranarray(Y), None if Z is None else np.asfortranarray(Z), e)


def prepared(X, Y, Z=None):
    """What the preparation leaves of complete inputs without constant or duplicate columns, in numpy: every column of X and Y
    as its residual on [1, Z], those of X then scaled to n - 1 standard deviation 1.  For tests without a device; the GPU tests
    take the handle's own matrices."""
    n = X.shape[0]
    D = np.column_stack([np.ones(n)] + ([] if Z is None else [Z]))
    Q, _ = np.linalg.qr(D)
    Xr = X - Q @ (Q.T @ X)
    Yr = Y - Q @ (Q.T @ Y)
    return np.asfortranarray(Xr / Xr.std(axis=0, ddof=1)), np.asfortranarray(Yr)


def plants_hold(ref, kind, d, lo, hi):
    """What case() plants, read off the reference: EQ undefined through Vg, ZERO undefined through Vw where the algebra says
    so (binary e, no covariates) and clear of the rule elsewhere, and the planted pair the best of trait 0, clear of the
    runner-up by the bound."""
    inside, defined = ref["inside"], ref["defined"]
    ok = ref["vg_ratio"][EQ] < 1e-13 and not defined[EQ].any() and not ref["pred_ok"][EQ]
    if kind == "binary" and d == 0:
        ok = ok and ref["vg_ratio"][ZERO] > 1e-6 and ref["vw_ratio"][ZERO] < 1e-13 and not defined[ZERO].any()
    else:
        ok = ok and bool(ref["pred_ok"][ZERO]) and ref["vw_ratio"][ZERO] > 1e-6
    bs, clear = best(ref)
    return bool(ok and lo[0] <= PLANT < hi[0] and inside[PLANT, 0] and defined[PLANT, 0] and bs[0] == PLANT and clear[0])
