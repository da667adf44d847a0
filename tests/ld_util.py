"""LD pruning restated for the tests, independent of atlasqtl_amd: the band of correlations of a standardised matrix in
np.longdouble, the greedy first-one-wins rule in plain Python, and genotypes with linkage disequilibrium to run them on.

Semantics (include/atlasqtl_hip.h, aq_prep_ld_prune).  Xs is n x p1, every column with mean 0 and sum of squares n - 1.
r(i, j) = Xs_i . Xs_j / (n - 1).  A pair i < j is eligible when j - i <= window, group[i] == group[j] and, with window_bp,
|pos_j - pos_i| <= window_bp.  Going through j in increasing order, column j is removed iff some KEPT i < j forms an eligible
pair with it and r(i, j)^2 > r2; its tag is the smallest such i."""
import numpy as np

LD = np.longdouble


def gram_ld(Xs):
    """Xs' Xs / (n - 1) in long double, p1 x p1."""
    Xl = np.asarray(Xs, dtype=LD)
    return (Xl.T @ Xl) / LD(Xl.shape[0] - 1)


def band_ld(Xs, window, gram=None):
    """band[j, b] = r(j - 1 - b, j) in long double, NaN where j - 1 - b < 0: p1 x window."""
    G = gram_ld(Xs) if gram is None else gram
    p1 = G.shape[0]
    band = np.full((p1, window), np.nan, dtype=LD)
    for j in range(p1):
        m = min(window, j)
        if m:
            band[j, :m] = G[j - 1 - np.arange(m), j]
    return band


def eligible(i, j, window, group=None, pos=None, window_bp=None):
    if not (i < j and j - i <= window):
        return False
    if group is not None and group[i] != group[j]:
        return False
    if window_bp is not None and abs(int(pos[j]) - int(pos[i])) > window_bp:
        return False
    return True


def greedy(band, r2, window, group=None, pos=None, window_bp=None):
    """The greedy rule on a band (p1 x >= window).  Returns (removed bool[p1], ld_of int[p1] (-1: kept), ld_r2 longdouble[p1]
    (NaN: kept), margin): margin is the smallest |r^2 - r2| over all eligible pairs, what the threshold decisions rest on."""
    p1 = band.shape[0]
    removed = np.zeros(p1, dtype=bool)
    ld_of = np.full(p1, -1, dtype=np.int64)
    ld_r2 = np.full(p1, np.nan, dtype=LD)
    margin = np.inf
    for j in range(p1):
        for i in range(max(0, j - window), j):            # increasing i: the first hit is the smallest
            if not eligible(i, j, window, group, pos, window_bp):
                continue
            rr = band[j, j - 1 - i] ** 2
            margin = min(margin, abs(float(rr - LD(r2))))
            if rr > r2 and not removed[i] and ld_of[j] < 0:
                removed[j], ld_of[j], ld_r2[j] = True, i, rr
    return removed, ld_of, ld_r2, margin


def haplotype_copy_genotypes(n, p, rng, rho, maf=0.3):
    """n x p int8 dosages 0 / 1 / 2, the sum of two haplotypes.  On each haplotype SNP j copies SNP j - 1 with every sample
    flipped with probability rho[j] (a scalar serves all SNPs); SNP 0 is Bernoulli(maf).  r^2 between neighbours is about
    (1 - 2 rho)^2 and decays along the chain, so with rho drawn per SNP it spreads over (0, 1)."""
    rho = np.broadcast_to(np.asarray(rho, dtype=float), (p,))
    H = np.empty((2, n, p), dtype=np.int8)
    H[:, :, 0] = rng.random((2, n)) < maf
    for j in range(1, p):
        flip = rng.random((2, n)) < rho[j]
        H[:, :, j] = H[:, :, j - 1] ^ flip
    return (H[0] + H[1]).astype(np.int8)


def ld_case(n, p, q, seed, na=0.0):
    """Genotypes in LD (per-SNP flip probabilities from 0.002 to 0.45, log-uniform) with the constant and duplicate columns
    of tests.test_gpu_prepare._case laid over them -- columns 3 and p - 2 constant, 7 and 11 copies of 1, p - 1 a copy of 4 --
    and a Gaussian Y."""
    rng = np.random.default_rng(seed)
    rho = np.exp(rng.uniform(np.log(0.002), np.log(0.45), size=p))
    G = haplotype_copy_genotypes(n, p, rng, rho)
    G[:, 3] = 1
    G[:, p - 2] = 2
    G[:, 7] = G[:, 1]
    G[:, p - 1] = G[:, 4]
    G[:, 11] = G[:, 1]
    Y = rng.normal(size=(n, q))
    if na > 0:
        Y[rng.random(Y.shape) < na] = np.nan
    return G, Y


def standardise(G):
    """scale() of the non-constant, first-of-its-kind columns of G on the host: (Xs, original index of each column)."""
    X = np.asarray(G, dtype=np.float64)
    keep, seen = [], set()
    for j in range(X.shape[1]):
        col = X[:, j]
        if np.all(col == col[0]):
            continue
        Xc = (col - col.mean()) / col.std(ddof=1)
        key = Xc.tobytes()
        if key in seen:
            continue
        seen.add(key)
        keep.append(j)
    Xk = X[:, keep]
    return (Xk - Xk.mean(0)) / Xk.std(0, ddof=1), np.array(keep)


def three_groups(p):
    """Three groups over p columns whose borders (at p // 3 + 1 and 2 p // 3 + 3, clipped) are not multiples of 16 for the
    sizes the tests use."""
    g = np.zeros(p, dtype=np.int64)
    a, b = min(p - 2, p // 3 + 1), min(p - 1, 2 * p // 3 + 3)
    g[a:] = 1
    g[b:] = 2
    return g


def chain_abc(n=400, seed=7):
    """Three columns A, B, C with r^2(A, B) > 0.5, r^2(B, C) > 0.5 and r^2(A, C) < 0.5: B = A + e1, C = B + e2 - lam A chosen so
    that C leans on B's own part.  Returns the n x 3 float64 matrix and its long-double correlation matrix."""
    rng = np.random.default_rng(seed)
    a, e = rng.normal(size=n), rng.normal(size=n)
    X = np.column_stack([a, a + 0.75 * e, 0.25 * a + e])
    Xs = (X - X.mean(0)) / X.std(0, ddof=1)
    return X, gram_ld(Xs)
