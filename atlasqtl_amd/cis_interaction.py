"""The interaction= argument of cis_screen(), on the host: the interaction variable checked (_interaction_vector), the
orthonormal basis of [1, Z, e] that the genotype x environment scan takes, by a long-double Gram-Schmidt under the rule of
aq_cov_basis (interaction_basis), and what that scan refuses to be combined with (refuse_with_interaction).  cis.cis_screen and
cis.cis_handle call them; nothing here touches a device.
"""
from __future__ import annotations

import numpy as np

from .checks import AtlasqtlError, refuse_

COV_TOL = 1e-10                                        # AQ_COV_TOL of csrc/aq_cov_kernels.h: the rule of aq_cov_basis


def _interaction_vector(e, n=None):
    """The interaction variable as one finite, non-constant float64 vector (of n values, where n is given)."""
    try:
        ev = np.asarray(e, dtype=np.float64)
    except (TypeError, ValueError):
        ev = None
    if ev is None or ev.ndim != 1 or ev.size < 1 or (n is not None and ev.shape[0] != int(n)):
        want = "one value per sample" if n is None else f"one value per sample ({int(n)})"
        raise AtlasqtlError(f"cis_screen: interaction must be one numeric vector with {want}, not "
                            f"{'that' if ev is None else ev.shape}. One interaction term per call.")
    if not np.all(np.isfinite(ev)):
        raise AtlasqtlError("cis_screen: interaction must be finite without missing value.")
    if ev.max() == ev.min():
        raise AtlasqtlError("cis_screen: interaction is constant: it cannot be told from the intercept.")
    return ev


def interaction_basis(e, covariates, n, n_cov):
    """(B, m) for the interaction scan, on the host: m = e centred (n values) and B, nb x n with nb = n_cov + 2, the orthonormal
    rows spanning [1, Z, e] in this order, by Gram-Schmidt with one re-orthogonalisation and long-double dot products.  A
    column is dropped when what is left of it after the columns before it has a squared norm <= 1e-10 times its own (the
    rule of aq_cov_basis).  Refused with AtlasqtlError, before anything is computed on a device: an e of the wrong length, a
    non-finite e, a constant e, an e inside span[1, Z], and covariates whose rank (the columns not dropped) is not n_cov, the
    number the handle was prepared with."""
    n, n_cov = int(n), int(n_cov)
    ev = _interaction_vector(e, n)
    if covariates is None:
        Z = np.zeros((n, 0))
    else:
        try:
            Z = np.asarray(covariates, dtype=np.float64)
        except (TypeError, ValueError):
            Z = None
        if Z is None or Z.ndim != 2 or Z.shape[0] != n or not np.all(np.isfinite(Z)):
            raise AtlasqtlError(f"cis_screen: covariates must be a finite numeric matrix with one row per sample ({n}).")
    LD = np.longdouble
    rows = [np.full(n, 1.0 / np.sqrt(n))]

    def remainder(col):
        v = np.array(col, dtype=np.float64)
        own = float(np.dot(v.astype(LD), v.astype(LD)))
        for _ in range(2):
            for b in rows:
                v = v - b * float(np.dot(b.astype(LD), v.astype(LD)))
        rem = float(np.dot(v.astype(LD), v.astype(LD)))
        return v, rem, own

    for l in range(Z.shape[1]):
        v, rem, own = remainder(Z[:, l])
        if rem > COV_TOL * own:
            rows.append(v / np.sqrt(rem))
    rank = len(rows) - 1
    if rank != n_cov:
        raise AtlasqtlError(f"cis_screen: the covariates given with interaction= have rank {rank}, but the data were prepared with "
                            f"{n_cov} covariates. Pass the covariates the data were prepared with.")
    m = ev - ev.mean()
    v, rem, own = remainder(m)
    if not rem > COV_TOL * own:
        raise AtlasqtlError("cis_screen: interaction lies in the span of the intercept and the covariates: its effect cannot be "
                            "told from theirs.")
    rows.append(v / np.sqrt(rem))
    return np.ascontiguousarray(np.stack(rows, axis=0)), m


def refuse_with_interaction(permutations, condition_on, Y):
    refuse_("cis_screen", [(permutations, "interaction= together with permutations= is not supported: permutation nulls are "
                                          "computed for the plain scan only. best_pvalue_bonferroni corrects each trait's best interaction."),
                           (condition_on, "interaction= together with condition_on= is not supported. Run the two separately.")],
            (Y, "interaction= needs complete Y; Y has missing values."))
