"""The cis fine-mapping restated for the tests, independent of atlasqtl_amd: the model of aq_prep_cis_finemap
(include/atlasqtl_hip.h) in np.longdouble on a handle's own matrices, with a float64 switch; the same model once more in
susieR's sufficient-statistics form; and inputs to run them on.

The model.  Xs [n x p] and Yc [n x q] are the prepared matrices, used as they are (susieR's susie(standardize = FALSE,
intercept = FALSE)).  Per trait with window [lo, hi) and L effects: d_s = x_s'x_s; a predictor with d_s <= 1e-10 n has prior
weight 0 and is counted in n_undef, the other P have pi = 1 / P.
  Start.         alpha = pi, mu = 0, fit_l = 0, sigma2 = y'y / (n - 1), V_l = scaled_prior_variance y'y / (n - 1), ELBO = -inf.
  An iteration.  Rf = y - sum_l fit_l in the order l = 0 ... L - 1; then per effect l = 0 ... L - 1:
                 r_l = Rf + fit_l; z = X_w'r_l;
                 lbf_s = 1/2 log(sigma2 / (sigma2 + V_l d_s)) + 1/2 z_s^2 V_l / (sigma2 (sigma2 + V_l d_s)) (0 if V_l = 0);
                 alpha_s = pi exp(lbf_s) / sum pi exp(lbf); lbf_model = log sum pi exp(lbf);
                 v_s = 1 / (d_s / sigma2 + 1 / V_l); mu_s = v_s z_s / sigma2; mu2_s = v_s + mu_s^2;
                 V_l <- sum alpha mu2 (used from the next iteration on), and V_l <- 0 if lbf_model at the new V_l is <= 0;
                 fit_l <- sum_s x_s alpha_s mu_s; Rf <- r_l - fit_l;
                 KL_l = -lbf_model + (2 sum z alpha mu - sum d alpha mu2) / (2 sigma2).
  After them.    ERSS = |Rf|^2 + sum_l (sum_s d_s alpha_ls mu2_ls - |fit_l|^2);
                 ELBO = -(n / 2) log(2 pi sigma2) - ERSS / (2 sigma2) - sum_l KL_l with the sigma2 the iteration used;
                 converged if tol > 0 and ELBO - ELBO_prev < tol, otherwise sigma2 <- ERSS / n.  tol = 0 never converges.
A converged trait's state is what it was in the iteration in which it stopped."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def _lbf(z, d, V, s2):
    """lbf_s for z [m x w], d [w], V and s2 [m x 1]; 0 where V = 0"""
    den = s2 + V * d
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 0.5 * np.log(s2 / den) + 0.5 * z * z * V / (s2 * den)
    return np.where(V == 0, 0 * out, out)


def _lse(lbf, ok, pi):
    """(the largest lbf, sum pi exp(lbf - largest)) over the predictors with weight, per row"""
    mx = np.max(np.where(ok, lbf, -np.inf), axis=1)
    w = np.where(ok, pi * np.exp(lbf - mx[:, None]), 0 * lbf)
    return mx, w, w.sum(axis=1)


def _fit_group(X, Y, L, iters, tol, spv, F, snapshots):
    """The model for the traits Y [n x m] that share the window X [n x w], in the number type F, all of them in one set of
    array operations (the long-double products are what a reference costs).  None if no predictor has weight."""
    n, w = X.shape
    m = Y.shape[1]
    d = (X * X).sum(axis=0)
    ok = d > F(1e-10) * F(n)
    P = int(ok.sum())
    if P == 0:
        return None
    pi = F(1) / F(P)
    two_pi = 8 * np.arctan(F(1))
    yy = (Y * Y).sum(axis=0)
    s2 = yy / F(n - 1)
    V = np.tile(F(spv) * yy / F(n - 1), (L, 1))
    alpha = np.zeros((L, m, w), dtype=F) + np.where(ok, pi, F(0))
    mu = np.zeros((L, m, w), dtype=F)
    fit = np.zeros((L, n, m), dtype=F)
    lbfm = np.zeros((L, m), dtype=F)
    act = np.ones(m, dtype=bool)
    prev = np.full(m, -np.inf, dtype=F)
    n_iter = np.zeros(m, dtype=np.int64)
    conv = np.zeros(m, dtype=bool)
    trace = np.full((iters, m), np.nan, dtype=F)
    margins, snaps = [], {}
    V_trace = np.full((iters, L, m), np.nan, dtype=F)
    for it in range(iters):
        a = np.nonzero(act)[0]
        if a.size == 0:
            break
        Rf = Y[:, a].copy()
        for l in range(L):
            Rf = Rf - fit[l][:, a]
        s2a = s2[a][:, None]
        kl = np.zeros(a.size, dtype=F)
        extra = np.zeros(a.size, dtype=F)                      # sum_l (sum d alpha mu2 - |fit_l|^2)
        for l in range(L):
            r = Rf + fit[l][:, a]
            z = r.T @ X
            Vl = V[l, a][:, None]
            mx, wgt, sm = _lse(_lbf(z, d, Vl, s2a), ok, pi)
            al = wgt / sm[:, None]
            lm = mx + np.log(sm)
            with np.errstate(divide="ignore"):
                v = 1 / (d / s2a + 1 / Vl)
            mm = np.where(ok, v * z / s2a, 0 * z)
            m2 = v + mm * mm
            Vn = (al * m2).sum(axis=1)
            mx2, _, sm2 = _lse(_lbf(z, d, Vn[:, None], s2a), ok, pi)
            lm2 = mx2 + np.log(sm2)
            margins += [float(abs(x)) for x in lm2[Vn > 0]]
            Vn = np.where(lm2 <= 0, 0 * Vn, Vn)
            f = X @ (al * mm).T
            Rf = r - f
            sz = (z * al * mm).sum(axis=1)
            sd = (d * al * m2).sum(axis=1)
            kl = kl + (-lm + (2 * sz - sd) / (2 * s2a[:, 0]))
            extra = extra + (sd - (f * f).sum(axis=0))
            alpha[l][a], mu[l][a], V[l, a], lbfm[l, a] = al, mm, Vn, lm
            fit[l][:, a] = f
        erss = (Rf * Rf).sum(axis=0) + extra
        elbo = -F(n) / 2 * np.log(two_pi * s2a[:, 0]) - erss / (2 * s2a[:, 0]) - kl
        trace[it, a] = elbo
        n_iter[a] = it + 1
        with np.errstate(invalid="ignore"):
            c = (elbo - prev[a] < F(tol)) if tol > 0 else np.zeros(a.size, dtype=bool)
        prev[a] = elbo
        s2[a[~c]] = erss[~c] / F(n)
        conv[a[c]] = True
        act[a[c]] = False
        V_trace[it] = V
        if it + 1 in snapshots:
            snaps[it + 1] = dict(alpha=alpha.copy(), mu=mu.copy(), V=V.copy(), sigma2=s2.copy(), lbf=lbfm.copy())
    return dict(alpha=alpha, mu=mu, V=V, sigma2=s2, lbf=lbfm, trace=trace, n_iter=n_iter, conv=conv, margins=margins, snaps=snaps,
                n_undef=w - P, V_trace=V_trace)


def reference(Xs, Yc, lo, hi, L, iters, tol=0.0, scaled_prior_variance=0.2, dtype=LD, snapshots=()):
    """The definition.  dict(alpha, mu [q x L x p, 0 outside the window], V, lbf [q x L], sigma2 [q], elbo [iters x q], V_trace
    [iters x q x L: V after every iteration], n_iter, converged, n_undef [q], margins [every |lbf_model(V_new)| of a null check
    with V_new > 0: where V_new = 0 the check decides nothing], snaps {k: the same state after k iterations, for k in snapshots}), in `dtype` (np.longdouble, or
    np.float64 for the float64 restatement).  A trait with an empty window, or without a predictor of weight, has n_iter = 0
    and NaN in sigma2, V, lbf."""
    F = dtype
    X, Y = np.asarray(Xs, dtype=F), np.asarray(Yc, dtype=F)
    n, p = X.shape
    q = Y.shape[1]

    def blank():
        return dict(alpha=np.zeros((q, L, p), dtype=F), mu=np.zeros((q, L, p), dtype=F), V=np.full((q, L), np.nan, dtype=F),
                    lbf=np.full((q, L), np.nan, dtype=F), sigma2=np.full(q, np.nan, dtype=F))
    out = blank()
    out.update(elbo=np.full((iters, q), np.nan, dtype=F), V_trace=np.full((iters, q, L), np.nan, dtype=F),
               n_iter=np.zeros(q, dtype=np.int64), converged=np.zeros(q, dtype=bool), n_undef=np.zeros(q, dtype=np.int64), margins=[],
               snaps={k: blank() for k in snapshots})
    groups = {}
    for t in range(q):
        if hi[t] > lo[t]:
            groups.setdefault((int(lo[t]), int(hi[t])), []).append(t)

    def put(dst, src, a, b, ts):
        dst["alpha"][ts, :, a:b] = np.transpose(src["alpha"], (1, 0, 2))
        dst["mu"][ts, :, a:b] = np.transpose(src["mu"], (1, 0, 2))
        dst["V"][ts], dst["lbf"][ts], dst["sigma2"][ts] = src["V"].T, src["lbf"].T, src["sigma2"]

    for (a, b), ts in groups.items():
        g = _fit_group(X[:, a:b], Y[:, ts], L, iters, tol, scaled_prior_variance, F, set(snapshots))
        if g is None:
            out["n_undef"][ts] = b - a
            continue
        put(out, g, a, b, ts)
        for k, s in g["snaps"].items():
            put(out["snaps"][k], s, a, b, ts)
        out["elbo"][:, ts], out["n_iter"][ts], out["converged"][ts], out["n_undef"][ts] = g["trace"], g["n_iter"], g["conv"], g["n_undef"]
        out["margins"] += g["margins"]
        out["V_trace"][:, ts, :] = np.transpose(g["V_trace"], (0, 2, 1))
    return out


def reference_ss(Xs, Yc, lo, hi, L, iters, scaled_prior_variance=0.2, dtype=LD):
    """The independent restatement, susieR's sufficient-statistics form, for a fixed number of iterations (tol = 0): per window
    X'X and X'y, b_l = alpha_l mu_l, z = X'y - X'X sum_(l' != l) b_l', |fit_l|^2 = b_l'X'X b_l, |y - X sum b|^2 = y'y -
    2 (sum b)'X'y + (sum b)'X'X (sum b).  No residual and no fit of length n is ever formed.  Returns dict(alpha, mu, V,
    sigma2, elbo) in the shapes of reference()."""
    F = dtype
    X, Y = np.asarray(Xs, dtype=F), np.asarray(Yc, dtype=F)
    n, p = X.shape
    q = Y.shape[1]
    out = dict(alpha=np.zeros((q, L, p), dtype=F), mu=np.zeros((q, L, p), dtype=F), V=np.full((q, L), np.nan, dtype=F),
               sigma2=np.full(q, np.nan, dtype=F), elbo=np.full((iters, q), np.nan, dtype=F))
    two_pi = 8 * np.arctan(F(1))
    for t in range(q):
        a, b = int(lo[t]), int(hi[t])
        if b <= a:
            continue
        Xw, y = X[:, a:b], Y[:, t]
        XtX, Xty, yty = Xw.T @ Xw, Xw.T @ y, y @ y
        d = np.diag(XtX).copy()
        ok = d > F(1e-10) * F(n)
        if not ok.any():
            continue
        pi = F(1) / F(int(ok.sum()))
        s2 = yty / F(n - 1)
        V = np.full(L, F(scaled_prior_variance) * yty / F(n - 1), dtype=F)
        al = np.zeros((L, b - a), dtype=F) + np.where(ok, pi, F(0))
        mu = np.zeros((L, b - a), dtype=F)
        for it in range(iters):
            kl, extra = F(0), F(0)
            for l in range(L):
                bb = al * mu
                z = Xty - XtX @ (bb.sum(axis=0) - bb[l])
                mx, wgt, sm = _lse(_lbf(z[None, :], d, V[l].reshape(1, 1), s2.reshape(1, 1)), ok, pi)
                lm = mx[0] + np.log(sm[0])
                with np.errstate(divide="ignore"):
                    v = 1 / (d / s2 + 1 / V[l])
                mm = np.where(ok, v * z / s2, 0 * z)
                m2 = v + mm * mm
                al[l], mu[l] = wgt[0] / sm[0], mm
                Vn = (al[l] * m2).sum()
                mx2, _, sm2 = _lse(_lbf(z[None, :], d, Vn.reshape(1, 1), s2.reshape(1, 1)), ok, pi)
                V[l] = 0 * Vn if mx2[0] + np.log(sm2[0]) <= 0 else Vn
                sd = (d * al[l] * m2).sum()
                kl = kl + (-lm + (2 * (z * al[l] * mu[l]).sum() - sd) / (2 * s2))
                bl = al[l] * mu[l]
                extra = extra + (sd - bl @ XtX @ bl)
            bs = (al * mu).sum(axis=0)
            erss = yty - 2 * (bs @ Xty) + bs @ XtX @ bs + extra
            out["elbo"][it, t] = -F(n) / 2 * np.log(two_pi * s2) - erss / (2 * s2) - kl
            s2 = erss / F(n)
        out["alpha"][t, :, a:b], out["mu"][t, :, a:b], out["V"][t], out["sigma2"][t] = al, mu, V, s2
    return out


# ---- comparisons ----
QUANTITIES = ("alpha", "mu", "V", "sigma2", "lbf")


def deviation(got, ref, key):
    """max |got - ref| of one quantity per trait (q values, long double), NaN = NaN, and the quantity's scale per trait: the
    largest |ref| of the trait, and at least 1 for alpha (a probability) and for lbf (lbf_model = the largest lbf_s + log of a
    sum near 1: the absolute error of a logarithm is the relative error of its argument, so an lbf_model of 0 -- an effect
    with V = 0, where it is log(sum pi) -- still carries the rounding of a number of size 1).  key: one of QUANTITIES, or elbo."""
    g, r = np.asarray(got[key], dtype=LD), np.asarray(ref[key], dtype=LD)
    if key == "elbo":                                          # [iterations x q]
        g, r = g.T, r.T
    q = r.shape[0]
    both_nan = np.isnan(g) & np.isnan(r)
    err = np.where(both_nan, LD(0), np.abs(g - r)).reshape(q, -1).max(axis=1)
    scale = np.nan_to_num(np.abs(r).reshape(q, -1), nan=0.0).max(axis=1)
    floor = LD(1) if key in ("alpha", "lbf") else LD(np.finfo(np.float64).tiny)
    return err, np.maximum(scale, floor)


# ---- inputs ----
PATTERNS = ("all", "band")
ZERO_COL = 2                # the column the tests make a column of zeros (planted() and the GPU tests' hook)


def windows(pattern, p, q, seed=0):
    """(s_lo, s_hi) int32.  all: every window is [0, p).  band: seeded random windows of up to 90 predictors; trait 0: [0, p),
    which holds its two causal variants and the zero column; trait 1: [0, min(p, 40)); trait 4, where there is one: empty."""
    lo, hi = np.zeros(q, dtype=np.int64), np.full(q, p, dtype=np.int64)
    if pattern == "band":
        rng = np.random.default_rng(1000 * seed + 7 * p + q)
        for t in range(q):
            a = int(rng.integers(0, p))
            lo[t], hi[t] = a, min(p, a + 1 + int(rng.integers(0, max(1, min(p, 90)))))
        lo[0], hi[0] = 0, p
        if q > 1:
            lo[1], hi[1] = 0, min(p, 40)
        if q > 4:
            lo[4], hi[4] = 5, 5
    else:
        assert pattern == "all"
    return lo.astype(np.int32), hi.astype(np.int32)


def causal(p):
    """the two causal variants of trait 0: each has non-causal neighbours in LD r ~ 0.9 next to it"""
    return (0, p - 2) if p < 12 else (5, p - 4)


def case(n, p, q, seed=0):
    """(X, Y): raw inputs, p >= 5.
      - trait 0 has two causal variants, causal(p), each with non-causal neighbours in LD r ~ 0.9 (the next column, and for
        p >= 12 the one before as well);
      - trait 1, where there is one, has no signal;
      - traits >= 2 carry one effect each, on predictor (3 t + 1) mod p, of a strength that varies with t, so that they stop
        at different iterations;
      - column ZERO_COL is meant to be replaced by zeros in the prepared matrix (the preparation would remove a constant
        column): it is in the window of trait 0 under both patterns;
      - trait 4 has an empty window under `band` (windows())."""
    assert p >= 5
    rng = np.random.default_rng(seed + 7919 * n + 31 * p + q)
    X = rng.standard_normal((n, p))
    c0, c1 = causal(p)
    for c in (c0, c1):
        for nb in ((c + 1,) if p < 12 else (c - 1, c + 1)):
            X[:, nb] = 0.9 * X[:, c] + np.sqrt(1 - 0.81) * X[:, nb]
    Y = rng.standard_normal((n, q))
    Y[:, 0] += 1.0 * X[:, c0] - 0.8 * X[:, c1]
    for t in range(2, q):
        Y[:, t] += (0.25 + 0.15 * (t % 5)) * X[:, (3 * t + 1) % p]
    return np.asfortranarray(X), np.asfortranarray(Y)


def prepared(X, Y, zero_col=ZERO_COL):
    """What the preparation leaves of complete inputs without constant or duplicate columns, in numpy, with column zero_col
    (None: none) replaced by zeros: for the tests that run without a device."""
    Xs = (X - X.mean(axis=0)) / X.std(axis=0, ddof=1)
    if zero_col is not None:
        Xs[:, zero_col] = 0.0
    return np.asfortranarray(Xs), np.asfortranarray(Y - Y.mean(axis=0))
