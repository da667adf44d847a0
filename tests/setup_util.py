"""The once-per-handle set-up of aq_vb_create restated for the tests, independent of atlasqtl_amd: where every entry of X, Y and the
initial matrices lies in the device buffers (index maps), what the Gram blocks hold (np.longdouble), how far an fp64 evaluation may
be from that (derived bounds), fp64 restatements of the device algorithms (to show on the CPU that the bounds hold for a correct
implementation and fail for a subtly wrong one), and the inputs the two test files run (tests/test_setup_host.py asserts what they
hold, tests/test_gpu_setup.py reads the buffers of a handle through aq_vb_debug_get_setup).

Layouts, from atlasqtl_amd/csrc/aq_core_sweep.h, aq_vb.h and aq_plan_const.h.  nb = ceil(p / 16) SNP blocks, ntile = q_pad / 16 trait
tiles, NTT = n_pad / 16 sample tiles; a padding position holds 0.0 (doubles) or the index n_pad (list slots).
  XA   [nb][NTT][2][64] double2   lane l: SNP 16 b + (l & 15), sample slot g = l >> 4; the pair (h, c) is k-step s = 2 h + c of the
                                  16-sample tile, whose slot g is sample 16 T + 4 s + g (accumulator map row = 4 reg + lane / 16;
                                  dmode 1: 16 T + 4 g + s)
  XU   [nb][NTT][2][64] double2   lane l: sample 16 T + (l & 15), SNP 16 b + 4 s + (l >> 4); the pair (h, c) is s = 2 h + c
  XR   [nb][NR][16]               row i, SNP 16 b + jj; rows n ... NR - 1 are zero (row n_pad is the one the list padding names)
  G    [nb][16][16]               x_{16 b + i}' x_{16 b + j}
  Gx   [nb][16][16]               x_{16 b + i}' x_{16 (b - 1) + j}; block 0 is zero
  GK   [ntile][nb][AQ_GK_STRIDE]  per trait k of the tile, over the trait's observed samples: the lower triangle of the diagonal block
                                  at [(i (i + 1) / 2 + j) 16 + k], i >= j; the cross block at AQ_GK_DIAG + [(16 i + j) 16 + k]
  midx [q_pad][Mmax] int32        trait k's list: its missing samples ascending -- wide split with 2 m > n: its observed samples
                                  (mobs[k] = 1) -- then n_pad; mcnt4[k] = 4 ceil(len / 16), the padded length in MFMA k-steps
  R, mis [ntile][n_pad][16], gam, mu [ntile][p_pad][16]    row r, trait 16 t + k

Bounds, in the convention of tests/mscreen_util.py: an m-term fp64 sum in any order, one rounding per product, is within
(m + 2) u sum |terms| of the exact sum, u = 2^-53; the first-order bound below is multiplied by that file's FACTOR = 2 for the
second-order terms.  With A = sum over all samples of |x_i x_j|, A_mis / A_obs the same over the trait's missing / observed
samples, mp the padded list length:
  G, Gx                  compensated (Kahan) sum: each product rounds once (u A), the compensated sum of the rounded products is
                         within 2 u |S| + O(n u^2) A of their sum                                     u (A + 2 |S|)
  GK = G - correction    the error of G (above), the mp-term correction in any order ((mp + 2) u A_mis), the subtraction's
                         rounding (u |value|)                                       u (A + 2 |G_ij| + (mp + 2) A_mis + |value|)
  GK, direct (mobs = 1)  an mp-term sum over the listed observed samples                              (mp + 2) u A_obs
  GK diagonal, redone    see redone_bound                                                              4 u |value|
"""
import numpy as np

from tests.mscreen_util import FACTOR, LD, U

GK_DIAG = 136 * 16                      # AQ_GK_DIAG
GK_STRIDE = 136 * 16 + 256 * 16         # AQ_GK_STRIDE
MIS_MMAX = 1024                         # AQ_MIS_MMAX
REDO_FRACTION = 0.125                   # aq_k_gk_diag_exact redoes a diagonal entry below this fraction of G_jj
REDO_CLEAR = 0.01                       # no input may put a diagonal entry this close (relative) to the threshold

# which = ... of aq_vb_debug_get_setup (include/atlasqtl_hip.h), and the geometry record's fields
WHICH = {name: i for i, name in enumerate(("geometry", "XA", "XU", "XR", "G", "Gx", "GK", "midx", "mcnt4", "mobs", "mis", "R", "gam",
                                           "mu"))}
GEOMETRY_FIELDS = ("nb", "ntile", "n_pad", "p_pad", "q_pad", "NR", "Mmax", "dmode", "use_la", "la_mask", "la_wide", "use_mis", "use_tw")
DTYPES = {"XA": np.float64, "XU": np.float64, "midx": np.int32, "mcnt4": np.int32, "mobs": np.int32}


# ------------------------------------------------------------------------------------------------------------------------------
# index maps: for every position of a buffer the flat column-major index (row + rows * column) of the source entry, or -1 = padding

def _src(row, col, rows, cols):
    return np.where((row < rows) & (col < cols), row + rows * col, -1).astype(np.int64)


def map_xa(nb, n_pad, n, p, dmode=0):
    b, T, h, l, c = np.indices((nb, n_pad // 16, 2, 64, 2))
    s, g = 2 * h + c, l >> 4
    return _src(16 * T + (4 * g + s if dmode else 4 * s + g), 16 * b + (l & 15), n, p)


def map_xu(nb, n_pad, n, p):
    b, T, h, l, c = np.indices((nb, n_pad // 16, 2, 64, 2))
    return _src(16 * T + (l & 15), 16 * b + 4 * (2 * h + c) + (l >> 4), n, p)


def map_xr(nb, NR, n, p):
    b, i, jj = np.indices((nb, NR, 16))
    return _src(i, 16 * b + jj, n, p)


def map_tiled(ntile, rows_pad, rows, q):
    t, r, k = np.indices((ntile, rows_pad, 16))
    return _src(r, 16 * t + k, rows, q)


def gather(idx, mat, fill=0.0):
    """The buffer an index map describes: mat (column-major source) at idx, `fill` at the padding."""
    flat = np.asarray(mat).reshape(-1, order="F")
    return np.where(idx >= 0, flat[np.maximum(idx, 0)], fill)


def gk_offsets():
    """(diag [16][16][16] with -1 above the diagonal, cross [16][16][16]): the offset of entry (i, j) of trait slot k inside one
    (tile, SNP block) of GK."""
    i, j, k = np.indices((16, 16, 16))
    diag = np.where(i >= j, (i * (i + 1) // 2 + j) * 16 + k, -1)
    cross = GK_DIAG + (16 * i + j) * 16 + k
    return diag, cross


def pack_gk(diag, cross):
    """[..., nb, 16 (i), 16 (j), 16 (k)] blocks -> [..., nb, GK_STRIDE] in the layout of GK (the upper triangle of diag is not stored)."""
    od, oc = gk_offsets()
    out = np.zeros(diag.shape[:-3] + (GK_STRIDE,), dtype=diag.dtype)
    low = od >= 0
    out[..., od[low]] = diag[..., low]
    out[..., oc.reshape(-1)] = cross.reshape(cross.shape[:-3] + (-1,))
    return out


def index_lists(miss, n_pad, Mmax, q_pad, wide):
    """(midx [q_pad][Mmax], mcnt4 [q_pad], mobs [q_pad]) from the n x q pattern `miss` (True = missing)."""
    n, q = miss.shape
    midx = np.full((q_pad, Mmax), n_pad, dtype=np.int32)
    mcnt4, mobs = np.zeros(q_pad, dtype=np.int32), np.zeros(q_pad, dtype=np.int32)
    for k in range(q):
        m = int(miss[:, k].sum())
        mobs[k] = 1 if (wide and 2 * m > n) else 0
        rows = np.nonzero(~miss[:, k] if mobs[k] else miss[:, k])[0]
        midx[k, :rows.size] = rows
        mcnt4[k] = 4 * -(-rows.size // 16)
    return midx, mcnt4, mobs


def expected_mmax(miss, wide):
    m = miss.sum(axis=0)
    longest = int(np.max(np.minimum(m, miss.shape[0] - m) if wide else m))
    return max(16, -(-longest // 16) * 16)


# ------------------------------------------------------------------------------------------------------------------------------
# reference values and bounds (long double)

def _blocks(M, nb, shift=0):
    """[nb][16][16] blocks (b, b - shift) of the p_pad x p_pad matrix M; the blocks b < shift are zero."""
    out = np.zeros((nb, 16, 16), dtype=M.dtype)
    for b in range(shift, nb):
        out[b] = M[16 * b:16 * b + 16, 16 * (b - shift):16 * (b - shift) + 16]
    return out


def _padded(X):
    n, p = X.shape
    Xp = np.zeros((n, -(-p // 16) * 16), dtype=LD)
    Xp[:, :p] = X
    return Xp


def gram_reference(X):
    """dict of [nb][16][16] long-double arrays: G, Gx (block 0 zero), A, Ax = the same sums over |x_i x_j|, and the bounds bG, bGx."""
    Xp = _padded(X)
    nb = Xp.shape[1] // 16
    S, A = Xp.T @ Xp, np.abs(Xp).T @ np.abs(Xp)
    out = dict(G=_blocks(S, nb), Gx=_blocks(S, nb, 1), A=_blocks(A, nb), Ax=_blocks(A, nb, 1))
    out["bG"] = LD(FACTOR * U) * (out["A"] + 2 * np.abs(out["G"]))
    out["bGx"] = LD(FACTOR * U) * (out["Ax"] + 2 * np.abs(out["Gx"]))
    return out


def redone_bound(value):
    """A diagonal entry that aq_k_gk_diag_exact redoes: 4 u |value| (times FACTOR).

    Both sums -- x_j' x_j over all n samples and over the mp listed ones -- are carried as unevaluated pairs hi + lo: every product is
    split exactly (x^2 = pr + pe), every addition into hi is a two-sum whose error goes to lo, so hi + lo misses the exact sum only
    by the roundings of the additions into lo.  |lo| stays below n u S (S the sum), so those roundings add up to at most n^2 u^2 S:
    second order.  The redo applies where value < S_all / 8, i.e. S_mis > 7/8 S_all, so hi_all and hi_mis lie within a factor of two
    and hi_all - hi_mis is exact (Sterbenz); lo_all - lo_mis rounds once, u |lo_all - lo_mis| <= 2 n u^2 S: second order; the final
    addition rounds once: u |value|.  First order that is u |value|.  The second-order terms are (n^2 + 2 n) u^2 S_all, which is
    below u |value| while value / S_all > (n^2 + 2 n) u = 1.8e-9 at n = 4000 (asserted for every redone entry of the cases in
    tests/test_setup_host.py); a standardised column keeps x_ij^2 > 0 at every observed sample, so the ratio never gets near it.
    With both at most u |value| the error is below 2 u |value|; the bar is twice that."""
    return LD(FACTOR * 4 * U) * np.abs(value)


def gk_reference(X, miss, mcnt4, mobs, gram=None):
    """Per trait the blocks X_b' diag(obs_k) X_b and X_b' diag(obs_k) X_{b-1} and their bounds.  Returns a dict of
    [q][nb][16][16] arrays: D, C (values), bD, bC (bounds; 0 = the entry must be exact), redone [q][nb][16] (diagonal entries below
    G_jj / 8 of a trait listed by its missing samples), margin [q][nb][16] (|D_jj / G_jj - 1/8| * 8, the relative distance from the
    threshold; inf where it does not apply), and kind [q] (0 = no missing sample: a copy of G / Gx; 1 = G - correction; 2 = direct)."""
    n, q = miss.shape
    gram = gram or gram_reference(X)
    Xp = _padded(X)
    nb = Xp.shape[1] // 16
    Xa = np.abs(Xp)
    out = {key: np.zeros((q, nb, 16, 16), dtype=LD) for key in ("D", "C", "bD", "bC")}
    out["redone"] = np.zeros((q, nb, 16), dtype=bool)
    out["margin"] = np.full((q, nb, 16), np.inf)
    out["kind"] = np.zeros(q, dtype=np.int64)
    fu = LD(FACTOR * U)
    dg = np.arange(16)
    for k in range(q):
        mk, mp = miss[:, k], 4 * int(mcnt4[k])
        if not mk.any():
            out["D"][k], out["C"][k] = gram["G"], gram["Gx"]        # kind 0: the test compares with the handle's own G and Gx
            continue
        So = Xp[~mk].T @ Xp[~mk]
        out["D"][k], out["C"][k] = _blocks(So, nb), _blocks(So, nb, 1)
        if mobs[k]:
            out["kind"][k] = 2
            Ao = Xa[~mk].T @ Xa[~mk]
            out["bD"][k] = fu * (mp + 2) * _blocks(Ao, nb)
            out["bC"][k] = fu * (mp + 2) * _blocks(Ao, nb, 1)
            continue
        out["kind"][k] = 1
        Am = Xa[mk].T @ Xa[mk]
        out["bD"][k] = fu * (gram["A"] + 2 * np.abs(gram["G"]) + (mp + 2) * _blocks(Am, nb) + np.abs(out["D"][k]))
        out["bC"][k] = fu * (gram["Ax"] + 2 * np.abs(gram["Gx"]) + (mp + 2) * _blocks(Am, nb, 1) + np.abs(out["C"][k]))
        out["bC"][k][0] = 0                                           # there is no block -1: exactly zero
        gjj, djj = gram["G"][:, dg, dg], out["D"][k][:, dg, dg]
        live = gjj > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            out["margin"][k] = np.where(live, np.abs(djj / gjj - LD(REDO_FRACTION)) / LD(REDO_FRACTION), np.inf).astype(np.float64)
        red = live & (djj < LD(REDO_FRACTION) * gjj)
        out["redone"][k] = red
        for b, j in zip(*np.nonzero(red)):
            out["bD"][k][b, j, j] = redone_bound(djj[b, j])
    return out


def tile_traits(a, q_pad, fill=None):
    """[q][nb][16][16] -> [ntile][nb][16][16][16 (k)]; the padded trait slots hold `fill` ([nb][16][16]) or zero."""
    q, nb = a.shape[:2]
    full = np.zeros((q_pad,) + a.shape[1:], dtype=a.dtype)
    full[:q] = a
    if fill is not None:
        full[q:] = fill
    return np.ascontiguousarray(full.reshape(q_pad // 16, 16, nb, 16, 16).transpose(0, 2, 3, 4, 1))


def worst_ratio(got, ref, bound):
    """Largest |got - ref| / bound over the entries with bound > 0; the entries with bound == 0 must be exact (AssertionError)."""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    zero = bound == 0
    assert np.all(err[zero] == 0), f"{int((err[zero] != 0).sum())} entries that must be exact are not"
    if zero.all():
        return 0.0
    return float(np.max(err[~zero] / bound[~zero]))


def check_gram(X, G, Gx, gram=None):
    """G, Gx [nb][16][16] fp64 against the reference.  Exact: G bitwise symmetric, zero rows and columns for SNP >= p (the bound is
    zero there), Gx block 0 zero.  Bounded: every entry.  Returns {"G": worst ratio, "Gx": worst ratio}."""
    gram = gram or gram_reference(X)
    assert np.array_equal(G, G.transpose(0, 2, 1)), "G is not bitwise symmetric"
    assert not Gx[0].any(), "Gx block 0 is not zero"
    return {"G": worst_ratio(G, gram["G"], gram["bG"]), "Gx": worst_ratio(Gx, gram["Gx"], gram["bGx"])}


GK_ROWS = ("copy", "indirect", "direct", "redone")


def check_gk(X, miss, mcnt4, mobs, q_pad, G, Gx, GK, gram=None, ref=None):
    """GK [ntile][nb][GK_STRIDE] fp64 against the reference, every stored entry under the row of the table it belongs to.  Exact: a
    trait without a missing sample, and every padded trait slot, holds the packed lower triangle of the given G and the given Gx;
    the cross block of SNP block 0 is zero.  Returns ({row: worst ratio}, {row: entries})."""
    q = miss.shape[1]
    ntile, nb = q_pad // 16, G.shape[0]
    ref = ref or gk_reference(X, miss, mcnt4, mobs, gram)
    kind = np.zeros(q_pad, dtype=np.int64)
    kind[:q] = ref["kind"]
    lab = np.broadcast_to(kind.reshape(ntile, 1, 1, 1, 16), (ntile, nb, 16, 16, 16))
    lab_d = lab.copy()
    for k, b, j in zip(*np.nonzero(ref["redone"])):
        lab_d[k // 16, b, j, j, k % 16] = 3
    labels = pack_gk(lab_d, lab)
    ref_p = pack_gk(tile_traits(ref["D"], q_pad), tile_traits(ref["C"], q_pad))
    bound_p = pack_gk(tile_traits(ref["bD"], q_pad), tile_traits(ref["bC"], q_pad))
    shape = (ntile, nb, 16, 16, 16)
    copy_p = pack_gk(np.broadcast_to(G[None, :, :, :, None], shape), np.broadcast_to(Gx[None, :, :, :, None], shape))
    got = np.asarray(GK).reshape(ntile, nb, GK_STRIDE)
    sel = labels == 0
    assert np.array_equal(got[sel].view(np.int64), copy_p[sel].view(np.int64)), "a trait without missing samples does not hold G / Gx"
    ratios, counts = {"copy": 0.0}, {"copy": int(sel.sum())}
    for l, row in enumerate(GK_ROWS):
        sel = labels == l
        counts[row] = int(sel.sum())
        if l > 0 and sel.any():
            ratios[row] = worst_ratio(got[sel], ref_p[sel], bound_p[sel])
    return ratios, counts


# ------------------------------------------------------------------------------------------------------------------------------
# fp64 restatements of the device algorithms (what a correct implementation computes, and two subtly wrong ones)

def _gram_f64(X, compensated):
    """G and Gx [nb][16][16] by one pass over the samples in order: compensated (aq_dot_kahan) or a plain running sum."""
    n, p = X.shape
    Xp = np.zeros((n, -(-p // 16) * 16))
    Xp[:, :p] = X
    nb = Xp.shape[1] // 16
    Xb = Xp.reshape(n, nb, 16)
    Xprev = np.zeros_like(Xb)
    Xprev[:, 1:] = Xb[:, :-1]
    res = []
    for other in (Xb, Xprev):
        s, c = np.zeros((nb, 16, 16)), np.zeros((nb, 16, 16))
        for r in range(n):
            prod = Xb[r][:, :, None] * other[r][:, None, :]
            if compensated:
                t = prod - c
                u = s + t
                c = (u - s) - t
                s = u
            else:
                s = s + prod
        res.append(s)
    return res


def kahan_gram_f64(X):
    return _gram_f64(X, True)


def plain_gram_f64(X):
    return _gram_f64(X, False)


def list_sum_f64(X, rows):
    """(diag, cross) [nb][16][16]: running fp64 sums of x_i x_j over `rows` in order (the padded slots add zeros)."""
    n, p = X.shape
    Xp = np.zeros((n, -(-p // 16) * 16))
    Xp[:, :p] = X
    nb = Xp.shape[1] // 16
    Xb = Xp.reshape(n, nb, 16)
    d, c = np.zeros((nb, 16, 16)), np.zeros((nb, 16, 16))
    for r in rows:
        d = d + Xb[r][:, :, None] * Xb[r][:, None, :]
        c[1:] = c[1:] + Xb[r][1:, :, None] * Xb[r][:-1, None, :]
    return d, c


def _two_prod(a, b):
    """a b = p + e exactly (Dekker / Veltkamp; numpy has no fused multiply-add)."""
    p = a * b
    sp = 134217729.0
    ah = a * sp; ah = ah - (ah - a); al = a - ah
    bh = b * sp; bh = bh - (bh - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd_redo_f64(x, rows):
    """The redo of aq_k_gk_diag_exact for the columns x (n x c) and one list: both sums of squares as hi + lo pairs, then
    (hi_all - hi_mis) + (lo_all - lo_mis).  The list's padding slots name an all-zero row: they add nothing."""
    hi, lo = np.zeros((2, x.shape[1])), np.zeros((2, x.shape[1]))
    for which, rr in enumerate((range(x.shape[0]), rows)):
        for r in rr:
            v = x[r]
            pr, pe = _two_prod(v, v)
            sm = hi[which] + pr
            bb = sm - hi[which]
            lo[which] += ((hi[which] - (sm - bb)) + (pr - bb)) + pe
            hi[which] = sm
    return (hi[0] - hi[1]) + (lo[0] - lo[1])


def gk_restated_f64(X, midx, mcnt4, mobs, n_pad, G, Gx, redo=True):
    """GK [ntile][nb][GK_STRIDE] as the device algorithms form it, in fp64 and list order: G - correction (trait listed by its
    missing samples), the direct sum (listed by its observed samples), and with `redo` the double-double redo of the diagonal
    entries that come out below G_jj / 8."""
    n, p = X.shape
    q_pad, nb = midx.shape[0], G.shape[0]
    Xp = np.zeros((n, 16 * nb))
    Xp[:, :p] = X
    D, C = np.zeros((q_pad, nb, 16, 16)), np.zeros((q_pad, nb, 16, 16))
    dg = np.arange(16)
    for k in range(q_pad):
        rows = midx[k, :4 * mcnt4[k]]
        rows = rows[rows != n_pad]
        d, c = list_sum_f64(X, rows)
        if mobs[k]:
            D[k], C[k] = d, c
            continue
        D[k], C[k] = G - d, Gx - c
        C[k][0] = 0.0
        if redo:
            for b in range(nb):
                js = np.nonzero(D[k][b, dg, dg] < REDO_FRACTION * G[b, dg, dg])[0]
                if js.size:
                    D[k][b, js, js] = dd_redo_f64(Xp[:, 16 * b + js], rows)
    return pack_gk(tile_traits(D, q_pad), tile_traits(C, q_pad))


# ------------------------------------------------------------------------------------------------------------------------------
# inputs

def _genotypes(n, p, regime, rng):
    from tests.util import _regime_genotypes
    return _regime_genotypes(n, p, frozenset(regime), rng)


def make_setup_problem(n, p, q, regime=(), missing=None, seed=5):
    """A problem in the form of tests.util.make_problem for a handle that is created and read, never run: genotypes from
    make_regime_problem's generator (tests.util._regime_genotypes: Binomial(2, 0.2), "ld" = haplotype copying with r^2 about 0.99
    across every block border, "rare" = every 5th column with 1 - 3 carriers), standardised by the oracle's scale_columns; Y normal
    with the NaN pattern `missing` (a function (n, q, carriers, rng) -> n x q bool), centred over its observed rows; explicit
    hyper-parameters and initial values through set_hyper / set_init (the automatic ones solve for p0, which has no solution at
    p = 1; tests.util.make_problem and make_regime_problem accept neither p = 1 nor p <= 80).  Every entry of gam_vb and mu_beta_vb is
    distinct.  Extra keys: miss (n x q bool), carriers."""
    from atlasqtl_amd import hyper_init as H
    from oracle import prepare_oracle
    rng = np.random.default_rng(seed + 7919 * n + 31 * p + q)
    G, carriers = _genotypes(n, p, regime, rng)
    X = np.asfortranarray(prepare_oracle.scale_columns(G))
    assert X.shape == (n, p) and np.all(np.isfinite(X))
    Y = rng.normal(size=(n, q))
    miss = np.zeros((n, q), dtype=bool) if missing is None else missing(n, q, carriers, rng)
    Y[miss] = np.nan
    Y = np.asfortranarray(Y - np.nanmean(Y, axis=0)[None, :])
    lh = H.set_hyper(q, p, eta=rng.uniform(0.5, 2.0, size=q), kappa=rng.uniform(0.5, 2.0, size=q), n0=rng.uniform(-2.0, -1.0, size=q),
                     nu=0.5, rho=3.0, t02=0.5)
    li = H.set_init(q, p, gam_vb=np.asfortranarray(rng.uniform(0.01, 0.99, size=(p, q))),
                    mu_beta_vb=np.asfortranarray(rng.normal(size=(p, q))), sig02_inv_vb=1.5, sig2_beta_vb=rng.uniform(0.5, 2.0, size=q),
                    sig2_theta_vb=rng.uniform(0.5, 2.0, size=p), tau_vb=rng.uniform(0.5, 2.0, size=q), theta_vb=rng.normal(size=p),
                    zeta_vb=rng.normal(size=q) - 1.5)
    return dict(X=X, Y=Y, list_hyper=lh, list_init=li, n=n, p=p, q=q, miss=miss, carriers=carriers, truth=dict(X=G))


def _drop(miss, k, rows):
    miss[np.asarray(rows, dtype=np.int64), k] = True


def _random_rows(rng, n, m, keep=()):
    """m rows drawn without replacement, `keep` among them."""
    keep = np.asarray(keep, dtype=np.int64)
    rest = np.setdiff1d(np.arange(n), keep)
    return np.concatenate([keep, rng.choice(rest, size=m - keep.size, replace=False)])


def short_longest(n):
    """The longest list of the short-list cases: AQ_MIS_MMAX where n allows it, else the largest multiple of 16 that leaves eight
    observed samples (a whole number of groups: a list with no padding slot at all, of length Mmax)."""
    return min(MIS_MMAX, 16 * ((n - 8) // 16))


def short_pattern(n, q, carriers, rng):
    """q = 20: a full trait tile and a ragged one.  Missing counts 0, 1, 15, 16, 17, 5 % and short_longest(n); where the case has rare
    variants, all carriers of one of them missing in traits 7, 8, 9 (a 3-carrier column, the last column, another 3-carrier column)
    and 16 (second tile, nothing else missing)."""
    assert q == 20
    miss = np.zeros((n, q), dtype=bool)
    for k, m in ((1, 1), (2, 15), (3, 16), (4, 17), (6, short_longest(n)), (18, 17)):
        _drop(miss, k, _random_rows(rng, n, m))
    for k in (5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 19):
        miss[:, k] = rng.random(n) < 0.05
    if carriers:
        cols = sorted(carriers)
        three = [j for j in cols if len(carriers[j]) == 3]
        for k, j in ((7, three[0]), (8, cols[-1]), (9, three[-1]), (16, cols[len(cols) // 2])):
            _drop(miss, k, carriers[j])
    return miss


def wide_pattern(n, q, carriers, rng):
    """q = 20 under the wide split, where a trait is listed by the shorter of its missing and its observed samples: missing counts
    0, 1, 16, 17, 5 %; n // 2 and n // 2 + 1 (2 m = n and 2 m = n + 2 for even n, 2 m = n - 1 and 2 m = n + 1 for odd n); well
    beyond n / 2 with observed lists of 1, 15, 16, 17 samples; all carriers of a rare variant missing in an indirect trait (8, 18)
    and in a direct one (7, 16)."""
    assert q == 20 and carriers
    cols = sorted(carriers)
    three = [j for j in cols if len(carriers[j]) == 3]
    miss = np.zeros((n, q), dtype=bool)
    plan = {1: (1, ()), 2: (16, ()), 3: (17, ()), 4: (int(0.05 * n), ()), 5: (n // 2, ()), 6: (n // 2 + 1, ()),
            7: (int(0.8 * n), carriers[three[0]]), 8: (int(0.05 * n), carriers[three[-1]]), 9: (int(0.45 * n), ()),
            10: (int(0.55 * n), ()), 11: (n - 16, ()), 12: (n - 17, ()), 13: (n - 1, ()), 14: (n - 15, ()), 15: (15, ()),
            16: (int(0.6 * n), carriers[cols[-1]]), 18: (int(0.05 * n), carriers[cols[len(cols) // 2]]), 19: (int(0.6 * n), ())}
    for k, (m, keep) in plan.items():
        _drop(miss, k, _random_rows(rng, n, m, keep))
    return miss


def fallback_pattern(n, q, carriers, rng):
    miss = rng.random((n, q)) < 0.1
    miss[:, 0] = False
    miss[:3] = False
    return miss


# The cases of tests/test_gpu_setup.py: name -> (family, n, p, q, regime, pattern, environment).
COMPLETE_P, COMPLETE_N, COMPLETE_Q = (1, 15, 16, 17, 33, 48), (17, 50, 333), (1, 17)
CASES = {}
for _n in COMPLETE_N:
    for _p in COMPLETE_P:
        for _q in COMPLETE_Q:
            CASES[f"complete-n{_n}-p{_p}-q{_q}"] = ("complete", _n, _p, _q, (), None, {})
CASES["complete-n4000-p48-q17"] = ("complete", 4000, 48, 17, (), None, {})
for _name, _n, _regime in (("rare", 300, ("rare",)), ("ld", 300, ("ld",)), ("ld-rare", 300, ("ld", "rare")), ("rare", 1000, ("rare",)),
                           ("rare", 1040, ("rare",))):       # n = 1040: the only one whose longest list reaches AQ_MIS_MMAX
    CASES[f"short-{_name}-n{_n}"] = ("short", _n, 40, 20, _regime, short_pattern, {})
# the wide split forced at small n with AQ_LA_C = 9, in nine parts of six sample tiles (n_pad = 864): n = 857 as
# tests/test_gpu_split_instances.py, and the even n = 856 next to it, because 2 m = n exists for even n only and 2 m = n + 1 for odd n only
for _n in (857, 856):
    CASES[f"wide-n{_n}"] = ("wide", _n, 40, 20, ("ld", "rare"), wide_pattern, {"AQ_LA_C": "9"})
CASES["fallback-n50"] = ("fallback", 50, 17, 5, (), fallback_pattern, {"AQ_KERNEL": "3"})

_problems = {}


def case_problem(name):
    """The problem of a case, built once per process and never modified."""
    if name not in _problems:
        family, n, p, q, regime, pattern, env = CASES[name]
        _problems[name] = make_setup_problem(n, p, q, regime, pattern)
    return _problems[name]
