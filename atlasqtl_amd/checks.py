"""The argument checks of the reference, R/prepare_atlasqtl.R:90-124 (``check_verbose_``, ``check_annealing_``) and
R/utils.R:10-100 (``check_*_``), with the reference's wording so that tests read like its own; ``AtlasqtlError``, raised
wherever the reference calls ``stop()``; the two predicates the option parsers of the package share, ``_is_whole`` and
``_is_real``; and the two checks the cis entries share, ``name_or_index_`` (a trait or a variant by its name or its index) and
``refuse_`` (arguments that do not go together, a path that needs complete Y).  This module imports nothing from the package.
"""
from __future__ import annotations

import numpy as np

_EPS75 = np.finfo(np.float64).eps ** 0.75


class AtlasqtlError(ValueError):
    """Raised where the reference calls ``stop()``."""


def check_natural_(x, name, eps=_EPS75):                      # R/utils.R:10-15
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    if np.any((x < eps) | (np.abs(x - np.round(x)) > eps)):
        raise AtlasqtlError(f"{name} must be natural.")


def check_positive_(x, name, eps=_EPS75):                     # R/utils.R:17-24
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    if np.any(x < eps):
        msg = f"{name} must be positive, greater than {eps:.3g}."
        if x.size > 1:
            msg = "All entries of " + msg
        raise AtlasqtlError(msg)


def check_zero_one_(x, name):                                 # R/utils.R:26-32
    x = np.asarray(x)
    if np.any(x < 0) or np.any(x > 1):
        msg = f"{name} must lie between 0 and 1."
        if x.size > 1:
            msg = "All entries of " + msg
        raise AtlasqtlError(msg)


def check_vector_(x, name, size=None, null_ok=False, na_ok=False):
    """check_structure_(x, "vector", ...) of R/utils.R:34-100 for numeric vectors."""
    if x is None:
        if null_ok:
            return None
        raise AtlasqtlError(f"{name} must be a non-empty a numeric vector.")
    a = np.atleast_1d(np.asarray(x, dtype=np.float64))
    ok = a.ndim == 1 and a.size > 0
    if size is not None:
        sizes = size if isinstance(size, (tuple, list)) else (size,)
        ok = ok and a.size in sizes
    if not na_ok:
        ok = ok and not np.any(np.isnan(a))
    ok = ok and bool(np.all(np.isfinite(a[~np.isnan(a)])))
    if not ok:
        raise AtlasqtlError(f"{name} must be a non-empty a numeric vector"
                            + (f" of length {size}" if size is not None else "")
                            + ", finite" + ("" if na_ok else " without missing value")
                            + (" or must be NULL" if null_ok else "") + ".")
    return a


def check_matrix_(x, name, shape=None, na_ok=False):
    """check_structure_(x, "matrix", ...) of R/utils.R:34-100."""
    a = np.asarray(x, dtype=np.float64)
    ok = a.ndim == 2 and a.size > 0
    if shape is not None:
        ok = ok and tuple(a.shape) == tuple(shape)
    if not na_ok:
        ok = ok and not np.any(np.isnan(a))
    ok = ok and bool(np.all(np.isfinite(a[~np.isnan(a)])))
    if not ok:
        raise AtlasqtlError(f"{name} must be a non-empty a numeric matrix"
                            + (f" of dimension {shape[0]} x {shape[1]}" if shape is not None else "")
                            + ", finite" + ("" if na_ok else " without missing value") + ".")
    return a


def check_verbose_(verbose):                                  # R/prepare_atlasqtl.R:90-95
    if verbose not in (0, 1, 2):
        raise AtlasqtlError("The verbose argument must be set to 0, 1 or 2.")


def check_annealing_(anneal):                                 # R/prepare_atlasqtl.R:100-124
    if anneal is None:
        return
    a = check_vector_(anneal, "anneal", size=3)
    check_natural_(a[[0, 2]], "anneal[c(1, 3)]")
    check_positive_(a[1], "anneal[2]")
    if a[0] not in (1, 2, 3):
        raise AtlasqtlError("The annealing spacing scheme must be set to 1 for geometric 2 for harmonic or 3 "
                            "for linear spacing.")
    if a[1] < 1.5:
        raise AtlasqtlError("Initial annealing temperature very small. May not be large enough for a "
                            "successful exploration. Please increase it or select no annealing.")
    if a[2] > 1000:
        raise AtlasqtlError("Temperature grid size very large. This may be unnecessarily computationally "
                            "demanding. Please decrease it.")


def _is_whole(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def _is_real(x, lo, hi, lo_open=False, hi_open=False):
    """x is a real number, no bool, between lo and hi: an end belongs to the interval unless it is named open."""
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
        return False
    x = float(x)
    return (lo < x if lo_open else lo <= x) and (x < hi if hi_open else x <= hi)


def name_or_index_(names, unknown, unusable, outside):
    """lookup(v) -> the index that v names among `names`: a name in it (the first index of a repeated name) or a whole number
    in [0, len(names)), no bool.  The three refusals are the caller's texts, formatted with v (as given), i (int(v)) and n
    (len(names)): `unknown` for a name that is not there, `unusable` for what is neither a name nor a whole number, `outside`
    for an index out of range.  The names are indexed when the first name is looked up."""
    first = {}

    def lookup(v):
        if isinstance(v, (str, np.str_)):
            if not first:
                first.update({str(nm): i for i, nm in reversed(list(enumerate(names)))})
            if str(v) not in first:
                raise AtlasqtlError(unknown.format(v=v))
            return first[str(v)]
        if not _is_whole(v):
            raise AtlasqtlError(unusable.format(v=v, n=len(names)))
        if not 0 <= int(v) < len(names):
            raise AtlasqtlError(outside.format(v=v, i=int(v), n=len(names)))
        return int(v)
    return lookup


def refuse_(who, together=(), complete_y=None):
    """What an entry refuses of its arguments' combination, as AtlasqtlError under its name `who`.  together: (value, message)
    pairs, arguments that do not go with the one asked for: the message of the first whose value is not None.  complete_y:
    (Y, message), for a path that takes complete Y only: the message where Y has a missing value; a Y of None is not at
    hand (a file yet to be read) and passes."""
    for value, message in together:
        if value is not None:
            raise AtlasqtlError(f"{who}: {message}")
    if complete_y is not None and complete_y[0] is not None and np.isnan(np.asarray(complete_y[0], dtype=np.float64)).any():
        raise AtlasqtlError(f"{who}: {complete_y[1]}")
