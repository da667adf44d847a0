"""The genetic relationship matrix and its principal components restated for the tests, independent of atlasqtl_amd: the
GRM of a standardised matrix in np.longdouble, the elementwise error bound of an fp64 evaluation in any order, the sign rule
of the PCs, and genotypes with population structure to run them on.

Semantics (include/atlasqtl_hip.h, aq_prep_grm).  Xs is n x p1, every column with mean 0 and sum of squares n - 1.
K[a, b] = (sum_j Xs[a, j] Xs[b, j]) / p1."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def pop_case(n, p, seed):
    """Balding-Nichols genotypes with F_ST = 0.1, n x p int8: ancestral frequencies U(0.1, 0.9); three populations with
    frequencies Beta(f (1 - F) / F, (1 - f) (1 - F) / F); sample i belongs to population 0 if i mod 6 < 3, to population 1
    if i mod 6 < 5, else to population 2; genotypes Binomial(2, frequency)."""
    rng = np.random.default_rng(seed)
    F = 0.1
    f = rng.uniform(0.1, 0.9, size=p)
    freq = rng.beta(f * (1 - F) / F, (1 - f) * (1 - F) / F, size=(3, p))
    m = np.arange(n) % 6
    pop = np.where(m < 3, 0, np.where(m < 5, 1, 2))
    return rng.binomial(2, freq[pop]).astype(np.int8)


def grm_ld(Xs):
    """Xs Xs' / p1 in long double, n x n.  (Rows contiguous and einsum: several times faster than @ on a Fortran-ordered
    long-double array, which has no BLAS behind it.)"""
    Xl = np.ascontiguousarray(Xs, dtype=LD)
    return np.einsum("aj,bj->ab", Xl, Xl) / LD(Xl.shape[1])


def grm_bound(Xs):
    """B[a, b] = (p1 + 2) 2^-53 (sum_j |Xs[a, j] Xs[b, j]|) / p1, in long double: the worst case of a p1-term fp64 dot product
    summed in any order ((p1 - 1) additions and one rounding per product: p1 2^-53 relative to sum |x y|, to first order),
    plus the division and the rounding of the result.  It holds for any tiling and any number of splits."""
    Al = np.abs(np.ascontiguousarray(Xs, dtype=LD))
    p1 = Al.shape[1]
    return LD((p1 + 2) * U) * np.einsum("aj,bj->ab", Al, Al) / LD(p1)


def pc_sign(V):
    """Columns of V signed so that the entry of largest magnitude is positive; the first such entry decides a tie."""
    V = np.array(V, dtype=np.float64, ndmin=2)
    for c in range(V.shape[1]):
        first = 0
        for i in range(V.shape[0]):
            if abs(V[i, c]) > abs(V[first, c]):
                first = i
        if V[first, c] < 0:
            V[:, c] = -V[:, c]
    return V


def top_eig(K_ld, k):
    """(eigenvalues descending [k], eigenvectors n x k signed by pc_sign, gap [k], lambda_1) of the long-double GRM rounded
    to fp64: gap_i is the distance of lambda_i to its nearest other eigenvalue."""
    w, V = np.linalg.eigh(np.asarray(K_ld, dtype=np.float64))
    w, V = w[::-1], V[:, ::-1]
    gap = np.array([np.min(np.abs(np.delete(w, i) - w[i])) for i in range(k)])
    return w[:k], pc_sign(V[:, :k]), gap, float(w[0])
