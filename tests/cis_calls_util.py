"""What the three cis entries (cis_screen, cis_independent, cis_finemap) and the handle-level functions under them hand to the
library, what they return and what they refuse, recorded on the stub library of tests/screen_calls_util.py with the two
fine-mapping entries added: tools/record_screen_calls.py wrote tests/golden/cis_calls_parent.json with this module from the
commit before cis.py was split by concern; tests/test_cis_calls_host.py replays it.

The code is reached through names both that commit and this one have: the public names of atlasqtl_amd, and for the
handle-level functions a lookup over the atlasqtl_amd modules loaded (function_).  The public entries run on a stubbed
preparation: prepare_data_ is replaced in every atlasqtl_amd module that has the name by a function that counts its calls and
returns the stub problem as prepared from 11 columns given, of which column 2 was removed -- so that the cut of snp_chrom and
snp_pos to the kept columns decides trait 1's window.  INITIAL_CAP is patched the same way, wherever it is named.

Every case records (library calls with arguments, how often the preparation ran, the result or the exception's type and
text)."""
import sys

import numpy as np

import atlasqtl_amd as A
from atlasqtl_amd import _lib
from tests import screen_calls_util as U
from tests.screen_calls_util import HANDLE, HI, LO, N, P, Q, _values, _view

# snp, trait, effect, alpha: trait 0's effects 0 and 1 give the same set {0, 1}; its effect 2 has V = 0; trait 2's effect 0 is
# one variant, its effect 1 the set {5, 6, 7}, which the purity below makes impure.  10 rows: more than a cap of 3 or 4.
ROWS = [(0, 0, 0, 0.6), (1, 0, 0, 0.37), (3, 0, 0, 0.02), (1, 0, 1, 0.55), (0, 0, 1, 0.42), (2, 0, 2, 0.99),
        (9, 2, 0, 0.97), (5, 2, 1, 0.5), (6, 2, 1, 0.3), (7, 2, 1, 0.18)]
PRIOR_V = {0: [0.5, 0.4, 0.0], 2: [0.3, 0.2]}         # trait -> V of its first effects; 0 for the others
P_GIVEN, REMOVED = 11, 2
SNP_CHROM = ["1"] * 6 + ["2"] * 5                      # per column given; the kept ones: 5 on "1", 5 on "2"
SNP_POS = [100, 200, 250, 300, 400, 500, 100, 200, 300, 400, 500]
TRAITS = dict(trait_chrom=["1", "1", "2"], trait_start=[105, 250, 110], trait_end=[395, 250, 490], window=10)   # LO, HI above


class CisStubLib(U.StubLib):
    """StubLib with the fine-mapping of the cis windows and the purity of its sets."""

    def aq_prep_cis_finemap(self, h, lo, hi, act, params, cap, snp, trait, effect, alpha, mu, mu2, n_rows, sigma2, V, lbf, elbo, n_iter,
                            conv, n_undef, a_dense, m_dense, plan):
        pm = params._obj
        L, iters = int(pm.L), int(pm.max_iter)
        k = max(int(cap), 0)
        rc = self._rec("aq_prep_cis_finemap", h, _values(lo, Q), _values(hi, Q), _values(act, Q),
                       dict(L=L, max_iter=iters, tol=pm.tol, scaled_prior_variance=pm.scaled_prior_variance, coverage=pm.coverage,
                            alpha_min=pm.alpha_min), cap, *[{"out": k}] * 6, type(n_rows._obj).__name__, _values(sigma2, Q),
                       _values(V, Q * L), _values(lbf, Q * L), _values(elbo, iters * Q), _values(n_iter, Q), _values(conv, Q),
                       _values(n_undef, Q), None if a_dense is None else {"out": Q * L * P},
                       None if m_dense is None else {"out": Q * L * P}, type(plan._obj).__name__)
        lo, hi = _view(lo, Q), _view(hi, Q)
        fitted = [t for t in range(Q) if lo[t] < hi[t] and (act is None or _view(act, Q)[t])]
        rows = [r for r in ROWS if r[1] in fitted and r[2] < L and lo[r[1]] <= r[0] < hi[r[1]]]
        w = min(len(rows), k)
        for dst, col in ((snp, 0), (trait, 1), (effect, 2), (alpha, 3)):
            _view(dst, w)[:] = [r[col] for r in rows[:w]]
        _view(mu, w)[:] = [0.1 * (r[0] + 1) * (-1) ** r[2] for r in rows[:w]]
        _view(mu2, w)[:] = [(0.1 * (r[0] + 1)) ** 2 + 0.01 for r in rows[:w]]
        n_rows._obj.value = len(rows)
        run = min(3, iters)
        for t in fitted:
            _view(sigma2, Q)[t] = 0.8 + 0.1 * t
            _view(V, Q * L)[t * L:(t + 1) * L] = (PRIOR_V[t] + [0.0] * L)[:L]
            _view(lbf, Q * L)[t * L:(t + 1) * L] = [1.5 + t + 0.25 * l for l in range(L)]
            _view(elbo, iters * Q)[t:run * Q:Q] = [-10.0 + it + t for it in range(run)]
            _view(n_iter, Q)[t], _view(conv, Q)[t] = run, 1
        _view(n_undef, Q)[0] = 1
        if a_dense is not None:
            _view(a_dense, Q * L * P)[:] = np.linspace(0.0, 1.0, Q * L * P)
            _view(m_dense, Q * L * P)[:] = np.linspace(-1.0, 1.0, Q * L * P)
        self._plan(plan._obj, L=L, batch_tiles=2, n_batches=1, forced=0, state_budget=1 << 30, state_bytes=4096, band_bytes=2048,
                   fit_bytes=1024)
        return rc

    def aq_prep_set_purity(self, h, ptr, idx, n_sets, mn, mean):
        offs = _values(ptr, n_sets + 1)
        members = _values(idx, offs[n_sets] + 1)
        rc = self._rec("aq_prep_set_purity", h, offs, members, n_sets, {"out": n_sets}, {"out": n_sets})
        for b in range(n_sets):
            s = members[offs[b]:offs[b + 1]]
            _view(mn, n_sets)[b], _view(mean, n_sets)[b] = (1.0, 1.0) if len(s) == 1 else (0.3, 0.45) if 5 in s else (0.8, 0.9)
        return rc


def _modules():
    return [m for name, m in sorted(sys.modules.items()) if name.startswith("atlasqtl_amd.") and m is not None]


def function_(name):
    """The function `name` of the one atlasqtl_amd module that defines it."""
    found = [getattr(m, name) for m in _modules() if getattr(getattr(m, name, None), "__module__", None) == m.__name__]
    assert len(found) == 1, (name, found)
    return found[0]


class patched:
    """`name` set to `value` in every atlasqtl_amd module that has it, and put back."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = [(m, getattr(m, self.name)) for m in _modules() if hasattr(m, self.name)]
        assert self.old, self.name
        for m, _ in self.old:
            setattr(m, self.name, self.value)

    def __exit__(self, *exc):
        for m, v in self.old:
            setattr(m, self.name, v)


def cases():
    """name -> a function of no arguments that returns (the stub it ran on, how often the preparation ran, what came back or
    dict(raises, text))."""
    Y, names_x, names_y, e, perms = U.problem()
    Ynan = Y.copy()
    Ynan[3, 1] = np.nan
    X = np.zeros((N, P_GIVEN))
    Z = np.random.default_rng(5).standard_normal((N, 2))
    coords = dict(snp_chrom=SNP_CHROM, snp_pos=SNP_POS)
    out = {}

    def case(name, call, prep_Y=Y, cap=None, n_cov=0, **stub_kw):
        """call(prep): on a PreparedData of the stub, for the handle-level functions; the public entries ignore it and get
        theirs from the stubbed preparation, which hands them the Y they passed."""
        def run():
            from atlasqtl_amd.prepare import PreparedData
            stub = CisStubLib(**stub_kw)
            _lib._lib = stub
            made = []

            def prepare(Yg, Xg, *args, **kw):
                cov = kw.get("covariates")
                prep = PreparedData(HANDLE, N, P, Q, Y if isinstance(Yg, str) else np.asfortranarray(Yg, dtype=np.float64),
                                    kw.get("device", 0), n_cov=np.shape(cov)[1] if np.ndim(cov) == 2 else 0)
                made.append(prep)
                removed = np.arange(P_GIVEN) == REMOVED
                return dict(X=prep, names_x=names_x, names_y=names_y, bool_rmvd_x=removed, rmvd_cst_x=np.array([REMOVED]),
                            rmvd_coll_x=np.zeros(0, dtype=np.int64), rmvd_cov_x=np.zeros(0, dtype=np.int64),
                            rmvd_ld_x=np.zeros(0, dtype=np.int64), n_covariates=prep.n_cov)
            prep = PreparedData(HANDLE, N, P, Q, prep_Y, 0, n_cov=n_cov)
            try:
                with patched("prepare_data_", prepare), patched("INITIAL_CAP", (1 << 16) if cap is None else cap):
                    try:
                        res = call(prep)
                    except Exception as err:                      # the exception is what is recorded
                        res = dict(raises=type(err).__name__, text=str(err))
                return stub, len(made), res
            finally:
                for pr in made + [prep]:
                    pr.handle = None                              # nothing to destroy: keep __del__ out of the record
        assert name not in out, name
        out[name] = run

    # ---- cis_finemap_handle ----
    fm = function_("cis_finemap_handle")
    for label, kw in (("defaults", {}), ("traits/bool", dict(traits=[True, False, True])), ("traits/index", dict(traits=[2])),
                      ("traits/names", dict(traits=["gene2", "gene0"])), ("traits/one_name", dict(traits="gene0")),
                      ("dense", dict(dense=True, L=3)), ("L2", dict(L=2, coverage=0.5, min_abs_corr=0.0, max_iter=2)),
                      ("max_rows", dict(max_rows=10)), ("max_rows/too_small", dict(max_rows=4))):
        case(f"cis_finemap_handle/{label}", lambda prep, kw=kw: fm(prep, names_x, names_y, LO, HI, **kw))
    case("cis_finemap_handle/second_call", lambda prep: fm(prep, names_x, names_y, LO, HI), cap=3)
    case("cis_finemap_handle/library_refuses", lambda prep: fm(prep, names_x, names_y, LO, HI, traits=[0]), prep_Y=Ynan,
         codes={"aq_prep_cis_finemap": 1})
    bad_fm = dict(L=[0, 17, 2.5, True], coverage=[0.0, 1.0, "0.9"], min_abs_corr=[-0.1, 1.5], tol=[-1e-3, np.inf, None],
                  max_iter=[0, 2.0], scaled_prior_variance=[0.0, np.inf], alpha_min=[-0.1, 2.0], max_rows=[0, 2.5])
    for arg, values in bad_fm.items():
        for i, v in enumerate(values):
            case(f"refused/cis_finemap_handle/{arg}/{i}", lambda prep, kw={arg: v}: fm(prep, names_x, names_y, LO, HI, **kw))
            case(f"refused/cis_finemap/{arg}/{i}", lambda prep, kw={arg: v}: A.cis_finemap(Y, X, **TRAITS, **coords, **kw))
    bad_traits = dict(bool_length=[True, False], unknown_name=["gene0", "nope"], index_high=[0, 3], index_negative=[-1],
                      real=[1.5], none_inside=[0, None], bool_inside=np.array([True, 1], dtype=object), matrix=np.ones((3, 1), dtype=bool))
    for label, v in bad_traits.items():
        case(f"refused/cis_finemap_handle/traits/{label}", lambda prep, v=v: fm(prep, names_x, names_y, LO, HI, traits=v))
    case("_traits_arg/first_of_a_repeated_name", lambda prep: function_("_traits_arg")(["b", np.str_("a"), np.int64(3)], ["a", "b", "a", "c"]))

    # ---- the three public entries on the stubbed preparation ----
    case("cis_screen/plain", lambda prep: A.cis_screen(Y, X, **TRAITS, **coords, p_value=0.05))
    case("cis_screen/bonferroni/max_pairs", lambda prep: A.cis_screen(Y, X, **TRAITS, **coords, max_pairs=2, device=1))
    case("cis_screen/second_call", lambda prep: A.cis_screen(Y, X, **TRAITS, **coords, fdr=0.9), cap=3)
    case("cis_screen/condition_on/names", lambda prep: A.cis_screen(Y, X, **TRAITS, **coords, p_value=0.05,
                                                                    condition_on={"gene0": ["snp3", "snp1"], "gene2": "snp9"}))
    case("cis_screen/condition_on/indices", lambda prep: A.cis_screen(Y, X, **TRAITS, **coords, p_value=0.05,
                                                                      condition_on=[[3, 1], [], 9]))
    case("cis_screen/condition_on/k_eff_below", lambda prep: A.cis_screen(Y, X, **TRAITS, **coords, fdr=0.3, condition_on={0: [3, 1], 2: [9, 7]}),
         cap=3, k_eff_cap=1)
    case("cis_screen/interaction", lambda prep: A.cis_screen(Y, X, **TRAITS, **coords, p_value=0.05, interaction=e))
    case("cis_screen/interaction/covariates", lambda prep: A.cis_screen(Y, X, **TRAITS, **coords, p_value=0.05, interaction=e, covariates=Z))
    case("cis_screen/interaction/second_call", lambda prep: A.cis_screen(Y, X, **TRAITS, **coords, p_value=0.5, interaction=list(e)), cap=3)
    case("cis_screen/permutations", lambda prep: A.cis_screen(Y, X, **TRAITS, **coords, p_value=0.05, permutations=perms))
    case("cis_screen/permutations/seed", lambda prep: A.cis_screen(Y, X, **TRAITS, **coords, permutations={"n": 2, "seed": 4}))
    case("cis_screen/missing_y", lambda prep: A.cis_screen(Ynan, X, **TRAITS, **coords, p_value=0.05))
    case("cis_screen/trait_end_defaults", lambda prep: A.cis_screen(Y, X, ["1", "3", "2"], [250, 1, 300], **coords, window=150, p_value=0.05))
    case("cis_independent", lambda prep: A.cis_independent(Y, X, **TRAITS, **coords, fdr=1.0, permutations=perms, max_signals=2))
    case("cis_independent/no_egene", lambda prep: A.cis_independent(Y, X, **TRAITS, **coords, fdr=1e-6, permutations=perms))
    case("cis_finemap", lambda prep: A.cis_finemap(Y, X, **TRAITS, **coords))
    case("cis_finemap/arguments", lambda prep: A.cis_finemap(Y, X, **TRAITS, **coords, L=3, coverage=0.9, min_abs_corr=0.2, tol=0.0, max_iter=5,
                                                             scaled_prior_variance=0.1, traits=["gene2"], alpha_min=1e-3, max_rows=8,
                                                             covariates=Z, dense=True, device=1))
    case("cis_finemap/second_call", lambda prep: A.cis_finemap(Y, X, **TRAITS, **coords), cap=3)
    case("cis_finemap/max_rows_too_small", lambda prep: A.cis_finemap(Y, X, **TRAITS, **coords, max_rows=4))

    # ---- the refusals of the entries: the window, the coordinates, the traits ----
    entries = dict(cis_screen=A.cis_screen, cis_independent=lambda *a, **kw: A.cis_independent(*a, permutations=perms, **kw),
                   cis_finemap=A.cis_finemap)
    no_window = {k: v for k, v in TRAITS.items() if k != "window"}
    for who, f in entries.items():
        for i, w in enumerate((-1, 2.5, True, None)):
            case(f"refused/{who}/window/{i}", lambda prep, f=f, w=w: f(Y, X, **no_window, **coords, window=w))
        case(f"refused/{who}/no_coordinates", lambda prep, f=f: f(Y, X, **TRAITS))
        case(f"refused/{who}/no_snp_pos", lambda prep, f=f: f(Y, X, **TRAITS, snp_chrom=SNP_CHROM))
        case(f"refused/{who}/snp_chrom_length", lambda prep, f=f: f(Y, X, **TRAITS, snp_chrom=SNP_CHROM[:-1], snp_pos=SNP_POS))
        case(f"refused/{who}/snp_pos_length", lambda prep, f=f: f(Y, X, **TRAITS, snp_chrom=SNP_CHROM, snp_pos=SNP_POS + [600]))
        case(f"refused/{who}/snp_pos_matrix", lambda prep, f=f: f(Y, X, **TRAITS, snp_chrom=SNP_CHROM, snp_pos=np.zeros((P_GIVEN, 1))))
        case(f"refused/{who}/trait_count", lambda prep, f=f: f(Y, X, ["1", "1"], [105, 250], **coords))
        case(f"refused/{who}/trait_end_length", lambda prep, f=f: f(Y, X, ["1", "1", "2"], [105, 250, 110], [395, 250], **coords))
        case(f"refused/{who}/trait_end_before_start", lambda prep, f=f: f(Y, X, ["1", "1", "2"], [105, 250, 110], [395, 240, 490], **coords))
        case(f"refused/{who}/positions_decrease", lambda prep, f=f: f(Y, X, **TRAITS, snp_chrom=SNP_CHROM, snp_pos=SNP_POS[:-1] + [50]))
        case(f"refused/{who}/chromosome_split", lambda prep, f=f: f(Y, X, **TRAITS, snp_chrom=SNP_CHROM[:-1] + ["1"], snp_pos=SNP_POS))
    hw = dict(cis_handle=function_("cis_handle"), cis_independent_handle=lambda *a: function_("cis_independent_handle")(*a, permutations=perms),
              cis_finemap_handle=fm)
    for who, f in hw.items():
        case(f"refused/{who}/windows/outside", lambda prep, f=f: f(prep, names_x, names_y, [0, 2, 5], [4, 2, 11]))
        case(f"refused/{who}/windows/count", lambda prep, f=f: f(prep, names_x, names_y, [0, 2], [4, 2]))
        case(f"refused/{who}/windows/real", lambda prep, f=f: f(prep, names_x, names_y, [0.0, 2.0, 5.0], HI))

    # ---- the thresholds, the permutations, max_signals ----
    sc = lambda **kw: (lambda prep: A.cis_screen(Y, X, **TRAITS, **coords, **kw))                      # noqa: E731
    ch = lambda **kw: (lambda prep: hw["cis_handle"](prep, names_x, names_y, LO, HI, **kw))             # noqa: E731
    ind = lambda **kw: (lambda prep: A.cis_independent(Y, X, **TRAITS, **coords, **{"permutations": perms, **kw}))     # noqa: E731
    indh = lambda **kw: (lambda prep: function_("cis_independent_handle")(prep, names_x, names_y, LO, HI,            # noqa: E731
                                                                          **{"permutations": perms, **kw}))
    bad_options = dict(both=dict(p_value=0.1, fdr=0.1), p_value_zero=dict(p_value=0.0), p_value_bool=dict(p_value=True), fdr_high=dict(fdr=1.5),
                       max_pairs_zero=dict(max_pairs=0), max_pairs_real=dict(max_pairs=2.0), permutations_zero=dict(permutations=0),
                       permutations_real=dict(permutations=2.5), permutations_dict=dict(permutations={"seed": 1}),
                       permutations_seed=dict(permutations={"n": 2, "seed": -1}), permutations_rows=dict(permutations=np.zeros((2, N), dtype=np.int64)),
                       permutations_width=dict(permutations=perms[:, :-1]), permutations_float=dict(permutations=perms.astype(float)))
    for label, kw in bad_options.items():
        case(f"refused/cis_screen/{label}", sc(**kw))
        case(f"refused/cis_handle/{label}", ch(**kw))
    for label, kw in dict(max_signals_zero=dict(max_signals=0), max_signals_six=dict(max_signals=6), max_signals_real=dict(max_signals=2.0),
                          max_signals_bool=dict(max_signals=True), permutations_none=dict(permutations=None), permutations_zero=dict(permutations=0),
                          permutations_width=dict(permutations=perms[:, :-1]), fdr_zero=dict(fdr=0.0), fdr_high=dict(fdr=1.5),
                          fdr_text=dict(fdr="0.05")).items():
        case(f"refused/cis_independent/{label}", ind(**kw))
        case(f"refused/cis_independent_handle/{label}", indh(**kw))
    case("refused/independent_signals_/max_signals", lambda prep: A.independent_signals_(None, [0], [0.1], [0.5], 6))

    # ---- not together with; complete Y only ----
    together = dict(condition_on_permutations=dict(condition_on=[[3], [], []], permutations=2),
                    interaction_permutations=dict(interaction=e, permutations=2),
                    interaction_condition_on=dict(interaction=e, condition_on=[[3], [], []]),
                    interaction_condition_on_permutations=dict(interaction=e, condition_on=[[3], [], []], permutations=2))
    for label, kw in together.items():
        case(f"refused/cis_screen/{label}", sc(**kw))
        case(f"refused/cis_handle/{label}", ch(**kw))
    case("refused/cis_screen/missing_y/condition_on", lambda prep: A.cis_screen(Ynan, X, **TRAITS, **coords, condition_on=[[3], [], []]))
    case("refused/cis_screen/missing_y/interaction", lambda prep: A.cis_screen(Ynan, X, **TRAITS, **coords, interaction=e))
    case("refused/cis_independent/missing_y", lambda prep: A.cis_independent(Ynan, X, **TRAITS, **coords, permutations=perms))
    case("refused/cis_handle/missing_y/condition_on", ch(condition_on=[[3], [], []]), prep_Y=Ynan)
    case("refused/cis_handle/missing_y/interaction", ch(interaction=e), prep_Y=Ynan)
    case("refused/cis_independent_handle/missing_y", indh(), prep_Y=Ynan)
    case("cis_screen/condition_on/y_from_a_file", lambda prep: A.cis_screen("y.txt", X, **TRAITS, **coords, condition_on=[[3], [], []]))

    # ---- condition_lists ----
    bad_lists = dict(unknown_variant={"gene0": ["nope"]}, unknown_trait={"nope": [1]}, variant_index_high=[[10], [], []],
                     variant_index_negative=[[-1], [], []], trait_index_high={3: [1]}, bool_variant=[[True], [], []], bool_trait={True: [1]},
                     real_variant=[[1.0], [], []], none_variant=[[None], [], []], duplicate=[[3, "snp3"], [], []], five=[[0, 1, 2, 3, 4], [], []],
                     trait_twice={"gene0": [1], 0: [2]}, wrong_length=[[1], []], text="snp1", number=3, nested=[[[1]], [], []])
    for label, v in bad_lists.items():
        case(f"refused/cis_screen/condition_on/{label}", sc(condition_on=v))
        case(f"refused/cis_handle/condition_on/{label}", ch(condition_on=v))
    case("condition_lists/first_of_a_repeated_name", lambda prep: function_("condition_lists")(
        {"b": ["y", np.int64(0)], np.str_("a"): np.str_("x"), 3: ()}, ["x", "y", "x"], ["a", "b", "a", "c"]))
    case("condition_lists/empty_entry_named_twice", lambda prep: function_("condition_lists")({"a": [], 0: [1]}, ["x", "y"], ["a", "b"]))

    # ---- interaction_basis ----
    inside = 3.0 + 2.0 * Z[:, 0] - Z[:, 1]
    dup = np.column_stack([Z, Z[:, 0]])
    bad_e = dict(length=e[:-1], matrix=np.stack([e, e], axis=1), text=["a"] * N, empty=[], scalar=1.0, nan=np.where(np.arange(N) == 2, np.nan, e),
                 inf=np.where(np.arange(N) == 2, np.inf, e), constant=np.full(N, 2.5))
    for label, v in bad_e.items():
        case(f"refused/cis_screen/interaction/{label}", sc(interaction=v))
        case(f"refused/cis_handle/interaction/{label}", ch(interaction=v))
        case(f"refused/cis_screen/interaction/{label}/y_from_a_file", lambda prep, v=v: A.cis_screen("y.txt", X, **TRAITS, **coords, interaction=v))
    case("refused/cis_screen/interaction/inside_the_span", sc(interaction=inside, covariates=Z))
    case("refused/cis_screen/interaction/covariates_rank", sc(interaction=e, covariates=dup))
    case("refused/cis_screen/interaction/covariates_rows", sc(interaction=e, covariates=Z[:-1]))
    case("refused/cis_screen/interaction/covariates_text", sc(interaction=e, covariates=[["a", "b"]] * N))
    case("refused/cis_screen/interaction/covariates_nan", sc(interaction=e, covariates=np.where(np.arange(2 * N).reshape(N, 2) == 5, np.nan, Z)))
    case("refused/cis_screen/interaction/covariates_vector", sc(interaction=e, covariates=Z[:, 0]))
    case("refused/cis_handle/interaction/inside_the_span", ch(interaction=inside, covariates=Z), n_cov=2)
    case("refused/cis_handle/interaction/rank_below_n_cov", ch(interaction=e, covariates=dup), n_cov=3)
    case("refused/cis_handle/interaction/covariates_not_given", ch(interaction=e), n_cov=2)
    case("refused/cis_handle/interaction/covariates_not_prepared", ch(interaction=e, covariates=Z))
    case("refused/cis_handle/interaction/covariates_rows", ch(interaction=e, covariates=Z[:-1]), n_cov=2)
    case("cis_handle/interaction/duplicated_covariate", ch(interaction=e, covariates=dup, p_value=0.05), n_cov=2)
    case("interaction_basis", lambda prep: function_("interaction_basis")(e, Z, N, 2))
    return out


def record():
    """name -> dict(calls, prepared, result) of every case, with the loaded library put back afterwards."""
    saved = _lib._lib
    try:
        table = {}
        for name, run in cases().items():
            stub, prepared, res = run()
            table[name] = dict(calls=U.encode(stub.calls), prepared=prepared, result=U.encode(res))
        return table
    finally:
        _lib._lib = saved
