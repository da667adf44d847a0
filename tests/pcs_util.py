"""The relationship operator applied to a block of vectors, and the criteria a set of genotype PCs is held to, restated for
the tests, independent of atlasqtl_amd.

Semantics (include/atlasqtl_hip.h, aq_prep_grm_apply).  Xs is n x p1, every column with mean 0 and sum of squares n - 1; Q is
n x L.  Z = Xs (Xs' Q) / p1 = K Q with K = Xs Xs' / p1; trace K = (sum of Xs^2) / p1."""
import numpy as np

from tests import grm_util as GU

LD, U = GU.LD, GU.U


def standardise(G):
    """The standardised matrix of genotypes G as the preparation forms it, in NumPy: constant columns dropped, every column
    centred and divided by its n - 1 standard deviation."""
    X = np.asarray(G, dtype=np.float64)
    X = X[:, X.std(axis=0) > 0]
    return (X - X.mean(axis=0)) / X.std(axis=0, ddof=1)


def operator(Xs):
    """Q -> Xs (Xs' Q) / p1 in fp64 NumPy: the operator the subspace iteration runs on when no device is there."""
    Xs = np.asarray(Xs, dtype=np.float64)
    return lambda Q: Xs @ (Xs.T @ Q) / Xs.shape[1]


def apply_ld(Xs, Q):
    """Xs (Xs' Q) / p1 in long double, n x L.  (Contiguous operands and einsum: a long-double array has no BLAS behind it.)"""
    Xl = np.ascontiguousarray(Xs, dtype=LD)
    Xt = np.ascontiguousarray(Xl.T)
    Ql = np.ascontiguousarray(Q, dtype=LD)
    T = np.einsum("ji,ic->jc", Xt, Ql)
    return np.einsum("ij,jc->ic", Xl, T) / LD(Xl.shape[1])


def apply_bound(Xs, Q):
    """B = (n + p1 + 4) 2^-53 |Xs| (|Xs'| |Q|) / p1 in long double: the same first-order argument as grm_util.grm_bound.  An
    entry of T = Xs' Q is an n-term fp64 dot product in any order, within n 2^-53 of sum |x q|; an entry of Xs T is a p1-term
    one over those, (p1 + n) 2^-53 of |Xs| (|Xs'| |Q|) to first order; the padding adds exact zeros; and the division, the
    rounding of T when it is stored and of the result are one rounding each.  It holds for any tiling and any split."""
    Al = np.abs(np.ascontiguousarray(Xs, dtype=LD))
    At = np.ascontiguousarray(Al.T)
    Ql = np.abs(np.ascontiguousarray(Q, dtype=LD))
    n, p1 = Al.shape
    T = np.einsum("ji,ic->jc", At, Ql)
    return LD((n + p1 + 4) * U) * np.einsum("ij,jc->ic", Al, T) / LD(p1)


def trace_ld(Xs):
    Xl = np.asarray(Xs, dtype=LD)
    return (Xl * Xl).sum() / LD(Xl.shape[1])


def pcs_by_columns(Xs, k):
    """The k leading eigenpairs of K = Xs Xs' / p1 by the p1 x p1 route, for n >> p1: eigh(Xs' Xs / p1), the matrix formed in
    long double and rounded to fp64, mapped back by Xs and normalised.  (eigenvalues descending [k], eigenvectors n x k signed
    by pc_sign, gap [k], lambda_1); the gap is taken among all p1 eigenvalues and 0, which K has n - p1 times."""
    Xs = np.asarray(Xs, dtype=np.float64)
    p1 = Xs.shape[1]
    Xt = np.ascontiguousarray(Xs.T, dtype=LD)
    w, W = np.linalg.eigh((np.einsum("ai,bi->ab", Xt, Xt) / LD(p1)).astype(np.float64))
    w, W = w[::-1], W[:, ::-1]
    V = Xs @ W[:, :k]
    V /= np.linalg.norm(V, axis=0)
    spec = np.concatenate([w, [0.0]])
    gap = np.array([np.min(np.abs(np.delete(spec, i) - spec[i])) for i in range(k)])
    return w[:k], GU.pc_sign(V), gap, float(w[0])


def check_pcs(out, lam_ref, V_ref, gap, lam1, k, eig_rtol, label=""):
    """The criteria of a result of subspace_pcs_ / genotype_pcs(solver="subspace") against reference eigenpairs:
      eigenvalues within eig_rtol relative;
      every PC within the Davis-Kahan bound of its reference vector, ||v - v_e (v_e' v)||_2 <= 2 residual lambda_1 / gap (the
      residual as returned is relative to lambda_1; the distance is to the span of v_e, so no 1 - cos^2 is formed);
      |V'V - I| <= 64 2^-53 k; the sign rule.
    Prints every figure before it asserts; returns (worst eigenvalue error, worst distance / bound)."""
    V, lam, res = out["pcs"], out["eigenvalues"], out["residuals"]
    assert V.shape == (V_ref.shape[0], k) and lam.shape == (k,) and res.shape == (k,)
    eig_err = np.abs(lam - lam_ref) / lam_ref
    ortho = float(np.max(np.abs(V.T @ V - np.eye(k))))
    dist = np.array([np.linalg.norm(V[:, i] - V_ref[:, i] * (V_ref[:, i] @ V[:, i])) for i in range(k)])
    bound = 2 * res * lam1 / gap
    print(f"{label}: iterations {out['iterations']}, residuals {res}, eigenvalue rel. error {eig_err}, "
          f"distance {dist} (bound {bound}), |V'V - I| {ortho:.3e} (bound {64 * U * k:.3e})")
    assert (eig_err <= eig_rtol).all()
    assert (dist <= bound).all()
    assert ortho <= 64 * U * k
    np.testing.assert_array_equal(V, GU.pc_sign(V))
    return float(eig_err.max()), float(np.max(dist / bound))


def apply_case(n, p, L):
    """(X n x p float64 with no constant and no duplicated column, Q n x L) for a test of the operator at (n, p1 = p, L):
    standard normal, the same bits on every call."""
    rng = np.random.default_rng(100000 * L + 1000 * n + p)
    X = np.asfortranarray(rng.standard_normal((n, p)))
    Q = np.asfortranarray(rng.standard_normal((n, L)))
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q
