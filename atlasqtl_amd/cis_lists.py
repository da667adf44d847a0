"""The condition_on= argument of cis_screen(), on the host: the argument as q lists of column indices (condition_lists) and
what the conditional scan refuses to be combined with (refuse_with_condition).  cis.cis_handle checks its argument with them
and cis_condition.py builds the forward-backward pass on that scan, so this module imports nothing of either.
"""
from __future__ import annotations

import numpy as np

from .checks import AtlasqtlError, name_or_index_, refuse_


def refuse_with_condition(permutations, Y):
    refuse_("cis_screen", [(permutations, "condition_on= together with permutations= is not supported: permutation nulls are "
                                          "computed for the unconditional scan only. Run the two separately, or cis_independent().")],
            (Y, "condition_on= needs complete Y; Y has missing values."))


def condition_lists(condition_on, names_x, names_y):
    """The condition_on argument of cis_screen() checked on the host: q lists of indices into names_x.  condition_on: a dict
    trait -> variants (a trait is an index into names_y or a name in it; traits not named get an empty list), or a list of q
    lists.  A variant is an index into names_x or a name in it; a single variant may stand without a list.  At most 4
    distinct variants per trait."""
    names_x, names_y = list(names_x), list(names_y)
    q = len(names_y)
    trait, variant = (name_or_index_(names, f"cis_screen: condition_on names the {what} {{v!r}}, which is not among the {what}s kept.",
                                     f"cis_screen: condition_on must name a {what} by its name or its index, not {{v!r}}.",
                                     f"cis_screen: condition_on has the {what} index {{i}} outside [0, {{n}}).")
                      for names, what in ((names_y, "trait"), (names_x, "variant")))
    if isinstance(condition_on, dict):
        items = [[] for _ in range(q)]
        for key, vs in condition_on.items():
            t = trait(key)
            if items[t]:
                raise AtlasqtlError(f"cis_screen: condition_on names trait {t} twice.")
            items[t] = vs
    else:
        try:
            items = list(condition_on)
        except TypeError:
            items = None
        if items is None or len(items) != q or isinstance(condition_on, str):
            raise AtlasqtlError(f"cis_screen: condition_on must be a dict trait -> variants or a list of one list per trait ({q}).")
    out = []
    for t, vs in enumerate(items):
        if isinstance(vs, (str, np.str_)) or np.ndim(vs) == 0:
            vs = [vs]
        lst = [variant(v) for v in vs]
        if len(lst) > 4:
            raise AtlasqtlError(f"cis_screen: trait {t} conditions on {len(lst)} variants; at most 4 are supported.")
        if len(set(lst)) != len(lst):
            raise AtlasqtlError(f"cis_screen: condition_on names a variant of trait {t} more than once.")
        out.append(lst)
    return out
