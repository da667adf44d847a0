"""What the screen family's Python hands to the library and what it makes of the answer, recorded on a stub in the place of
the loaded library (no GPU, no shared object): tools/record_screen_calls.py wrote tests/golden/screen_calls_parent.json with
this module from the commit before prepare.py was split and the screen entries' marshalling got one owner;
tests/test_screen_calls_host.py replays it.  Only names that both that commit and this one have are used.

The stub stands for one prepared problem, n = 12, p = 10, q = 3, with the windows [0, 4) [2, 2) [5, 10).  Every method records
its arguments -- scalars as they are, the values behind the input pointers at the lengths the entry defines, the incoming
values of the outputs the callers zero, the length of the other outputs, the type behind a byref -- and answers with one small
fixed table that honours `cap` and the windows."""
import ctypes as C
import math

import numpy as np

from atlasqtl_amd import _lib

N, P, Q = 12, 10, 3
LO, HI = [0, 2, 5], [4, 2, 10]
PAIRS = [(0, 0, 0.9), (1, 0, -0.8), (3, 0, 0.5), (5, 2, 0.7), (6, 2, -0.6), (9, 2, 0.95), (2, 0, 0.3)]     # snp, trait, r
BEST = {0: (0, 0.9), 2: (9, 0.95)}                     # trait -> best_snp, best_r of the plain scans
COND_BEST = {0: (1, 0.99), 2: (8, -0.98)}              # ... of the conditional and the interaction scan
HANDLE = 7


def _view(ptr, k):
    return np.ctypeslib.as_array(ptr, shape=(int(k),)) if int(k) > 0 else np.zeros(0)


def _values(ptr, k):
    return None if ptr is None else _view(ptr, k).tolist()


class StubLib:
    """The entries of the screen family and of the three return-code sites as plain methods; `calls` is the record."""

    def __init__(self, k_eff_cap=None, codes=None):
        self.calls = []
        self.k_eff_cap = k_eff_cap                     # the conditional scan reports min(list length, this)
        self.codes = codes or {}                       # entry -> return code

    def _rec(self, name, *args):
        self.calls.append([name] + list(args))
        return self.codes.get(name, 0)

    def aq_last_error(self):
        self._rec("aq_last_error")
        return b"stub: the library's message"

    def aq_prep_destroy(self, h):
        self._rec("aq_prep_destroy", h)

    def aq_rank_int(self, Y, n, q, c, out, n_obs, n_tied, device):
        return self._rec("aq_rank_int", _values(Y, n * q), n, q, c, {"out": n * q}, _values(n_obs, q), _values(n_tied, q), device)

    def aq_prep_ld_prune(self, h, ld):
        return self._rec("aq_prep_ld_prune", h, type(ld._obj).__name__)

    # ---- the table behind every scan ----
    def _fill(self, lo, hi, cap, snp, trait, r, n_pairs, best_snp, best_r, best):
        lo, hi = _view(lo, Q), _view(hi, Q)
        rows = [pr for pr in PAIRS if lo[pr[1]] <= pr[0] < hi[pr[1]]]
        k = min(len(rows), max(int(cap), 0))
        for dst, col in ((snp, 0), (trait, 1), (r, 2)):
            _view(dst, k)[:] = [pr[col] for pr in rows[:k]]
        n_pairs._obj.value = len(rows)
        bs, br = _view(best_snp, Q), _view(best_r, Q)
        for t in range(Q):
            bs[t], br[t] = best[t] if t in best and lo[t] < hi[t] else (-1, np.nan)

    @staticmethod
    def _plan(plan, **own):
        cis = plan.cis if hasattr(plan, "cis") else plan
        cis.tile, cis.sample_chunk, cis.lds_bytes, cis.n_items, cis.window_pairs, cis.staged_pairs = 64, 128, 100, 5, 9, 8192
        for name, v in own.items():
            setattr(plan, name, v)

    def aq_prep_marginal(self, h, cut, cap, snp, trait, r, n_pairs, rs, best_snp, best_r, n_undef, r_dense):
        rc = self._rec("aq_prep_marginal", h, _values(cut, Q), cap, {"out": max(cap, 0)}, {"out": max(cap, 0)}, {"out": max(cap, 0)},
                       type(n_pairs._obj).__name__, _values(rs, P), {"out": Q}, {"out": Q}, type(n_undef._obj).__name__,
                       None if r_dense is None else {"out": P * Q})
        everything = (C.c_int32 * Q)(0, 0, 0), (C.c_int32 * Q)(P, P, P)
        self._fill(everything[0], everything[1], cap, snp, trait, r, n_pairs, best_snp, best_r, BEST)
        counts = _view(rs, P)
        for s, _, _ in PAIRS:
            counts[s] += 1
        n_undef._obj.value = 2
        if r_dense is not None:
            _view(r_dense, P * Q)[:] = np.linspace(-0.9, 0.9, P * Q)
        return rc

    def aq_prep_marginal_perm(self, h, cut, B, perms, max_r2, hs, nsel, nundef):
        rc = self._rec("aq_prep_marginal_perm", h, _values(cut, Q), B, _values(perms, B * N), {"out": B * Q}, _values(hs, B),
                       _values(nsel, B), _values(nundef, B))
        _view(max_r2, B * Q)[:] = [0.1 + 0.15 * b + 0.05 * t for b in range(B) for t in range(Q)]
        _view(hs, B)[:] = [b % 3 for b in range(B)]
        _view(nsel, B)[:] = [2 * b for b in range(B)]
        _view(nundef, B)[:] = 2
        return rc

    def aq_prep_cis(self, h, lo, hi, cut, cap, snp, trait, r, n_pairs, best_snp, best_r, n_undef, plan):
        rc = self._rec("aq_prep_cis", h, _values(lo, Q), _values(hi, Q), _values(cut, Q), cap, {"out": max(cap, 0)},
                       {"out": max(cap, 0)}, {"out": max(cap, 0)}, type(n_pairs._obj).__name__, {"out": Q}, {"out": Q},
                       _values(n_undef, Q), type(plan._obj).__name__)
        self._fill(lo, hi, cap, snp, trait, r, n_pairs, best_snp, best_r, BEST)
        _view(n_undef, Q)[0] = 1
        self._plan(plan._obj)
        return rc

    def aq_prep_cis_perm(self, h, lo, hi, B, perms, max_r2):
        rc = self._rec("aq_prep_cis_perm", h, _values(lo, Q), _values(hi, Q), B, _values(perms, B * N), {"out": B * Q})
        lo, hi = _view(lo, Q), _view(hi, Q)
        _view(max_r2, B * Q)[:] = [0.1 + 0.15 * b + 0.05 * t if lo[t] < hi[t] else -1.0 for b in range(B) for t in range(Q)]
        return rc

    def aq_prep_cis_cond(self, h, lo, hi, ptr, idx, cut, cap, snp, trait, r, n_pairs, best_snp, best_r, n_undef, k_eff, plan):
        offs = _values(ptr, Q + 1)
        rc = self._rec("aq_prep_cis_cond", h, _values(lo, Q), _values(hi, Q), offs, _values(idx, offs[Q] + 1), _values(cut, Q), cap,
                       {"out": max(cap, 0)}, {"out": max(cap, 0)}, {"out": max(cap, 0)}, type(n_pairs._obj).__name__, {"out": Q},
                       {"out": Q}, _values(n_undef, Q), _values(k_eff, Q), type(plan._obj).__name__)
        self._fill(lo, hi, cap, snp, trait, r, n_pairs, best_snp, best_r, COND_BEST)
        lo, hi, ke = _view(lo, Q), _view(hi, Q), _view(k_eff, Q)
        for t in range(Q):
            k = offs[t + 1] - offs[t]
            ke[t] = 0 if lo[t] >= hi[t] else (k if self.k_eff_cap is None else min(k, self.k_eff_cap))
        self._plan(plan._obj, kc=2, max_k=4, lds_bytes=200, streams=3, qo_bytes=1 << 33)
        return rc

    def aq_prep_cis_int(self, h, lo, hi, basis, nb, mult, cut, cap, snp, trait, r, n_pairs, best_snp, best_r, n_undef, int_tol, plan):
        rc = self._rec("aq_prep_cis_int", h, _values(lo, Q), _values(hi, Q), _values(basis, nb * N), nb, _values(mult, N),
                       _values(cut, Q), cap, {"out": max(cap, 0)}, {"out": max(cap, 0)}, {"out": max(cap, 0)},
                       type(n_pairs._obj).__name__, {"out": Q}, {"out": Q}, _values(n_undef, Q), {"out": P}, type(plan._obj).__name__)
        self._fill(lo, hi, cap, snp, trait, r, n_pairs, best_snp, best_r, COND_BEST)
        _view(int_tol, P)[:] = np.linspace(0.05, 0.95, P)
        self._plan(plan._obj, streams=2, n_basis=nb, lds_bytes=300, mult_pad=16, basis_bytes=nb * N * 8)
        return rc


def problem():
    """(Y 12 x 3 complete and centred, names_x, names_y, e: the interaction variable, perms 3 x 12)."""
    rng = np.random.default_rng(11)
    Y = rng.standard_normal((N, Q))
    Y -= Y.mean(axis=0)
    perms = np.stack([rng.permutation(N) for _ in range(3)])
    return np.asfortranarray(Y), [f"snp{j}" for j in range(P)], [f"gene{t}" for t in range(Q)], rng.standard_normal(N), perms


def encode(x):
    """x as JSON can carry it: arrays with their dtype and shape, whole numbers as int, everything real as float."""
    if isinstance(x, dict):
        return {"dict": {str(k): encode(v) for k, v in x.items()}}
    if isinstance(x, (list, tuple)):
        return [encode(v) for v in x]
    if isinstance(x, np.ndarray):
        vals = [str(v) for v in x.ravel()] if x.dtype == object else x.ravel().tolist()
        return {"dtype": str(x.dtype), "shape": list(x.shape), "values": vals}
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x)
    if x is None or isinstance(x, str):
        return x
    raise TypeError(f"cannot record {type(x)}")


def _prep(stub, Y):
    from atlasqtl_amd.prepare import PreparedData
    _lib._lib = stub
    return PreparedData(HANDLE, N, P, Q, Y, 0)


def cases():
    """name -> a function of no arguments that returns (the stub it ran on, what came back)."""
    from atlasqtl_amd import cis as CIS
    from atlasqtl_amd import cis_condition as CC
    from atlasqtl_amd import marginal as M
    from atlasqtl_amd import prepare as PR
    Y, names_x, names_y, e, perms = problem()
    cut = np.array([0.25, np.inf, 0.5])
    basis = np.stack([np.full(N, 1.0 / np.sqrt(N)), (e - e.mean()) / np.linalg.norm(e - e.mean())])      # 2 x n
    out = {}

    def method(name, call, **stub_kw):
        def run():
            stub = StubLib(**stub_kw)
            prep = _prep(stub, Y)
            try:
                return stub, call(prep)
            finally:
                prep.handle = None                                # nothing to destroy: keep __del__ out of the record
        out[name] = run

    # ---- group 1: the six PreparedData screen methods ----
    for cap in (0, 3, 20):
        method(f"marginal/cap{cap}", lambda prep, cap=cap: prep.marginal(cut, cap))
        method(f"marginal/dense/cap{cap}", lambda prep, cap=cap: prep.marginal(cut, cap, dense=True))
        method(f"cis/cap{cap}", lambda prep, cap=cap: prep.cis(LO, HI, cut, cap))
        for label, cond in (("0", [[], [], []]), ("1", [[3], [], []]), ("4", [[3], [0, 1], [9, 2, 4, 6]])):
            method(f"cis_conditional/{label}/cap{cap}", lambda prep, cap=cap, cond=cond: prep.cis_conditional(LO, HI, cond, cut, cap))
        method(f"cis_interaction/cap{cap}", lambda prep, cap=cap: prep.cis_interaction(LO, HI, basis, e - e.mean(), cut, cap))
    method("marginal_permute", lambda prep: prep.marginal_permute(cut, perms))
    method("cis_permute", lambda prep: prep.cis_permute(LO, HI, perms.astype(np.int64)))

    # ---- group 2: the handle-level functions ----
    modes = {"p_value": dict(p_value=0.01), "fdr": dict(fdr=0.2), "bonferroni": {}, "max_pairs": dict(p_value=0.5, max_pairs=2)}
    for label, kw in modes.items():
        method(f"screen_handle/{label}", lambda prep, kw=kw: M.screen_handle(prep, names_x, names_y, **kw))
        method(f"cis_handle/{label}", lambda prep, kw=kw: CIS.cis_handle(prep, names_x, names_y, LO, HI, **kw))
    method("screen_handle/dense", lambda prep: M.screen_handle(prep, names_x, names_y, p_value=0.05, dense=True))
    method("screen_handle/permutations", lambda prep: M.screen_handle(prep, names_x, names_y, p_value=0.05, permutations=perms))
    method("screen_handle/fdr/permutations", lambda prep: M.screen_handle(prep, names_x, names_y, fdr=0.5, permutations=perms))
    method("cis_handle/permutations", lambda prep: CIS.cis_handle(prep, names_x, names_y, LO, HI, p_value=0.05, permutations=perms))
    method("cis_handle/condition_on", lambda prep: CIS.cis_handle(prep, names_x, names_y, LO, HI, p_value=0.05,
                                                                  condition_on={"gene0": ["snp3", 1], 2: 9}))
    method("cis_handle/condition_on/k_eff_below", lambda prep: CIS.cis_handle(prep, names_x, names_y, LO, HI, fdr=0.3,
                                                                              condition_on=[[3, 1], [], [9, 7]]), k_eff_cap=1)
    method("cis_handle/interaction", lambda prep: CIS.cis_handle(prep, names_x, names_y, LO, HI, p_value=0.05, interaction=e))

    def small_cap(call):
        def run(prep):
            old = M.INITIAL_CAP
            M.INITIAL_CAP = 3
            try:
                return call(prep)
            finally:
                M.INITIAL_CAP = old
        return run
    method("screen_handle/second_call", small_cap(lambda prep: M.screen_handle(prep, names_x, names_y, p_value=0.5)))
    method("cis_handle/second_call", small_cap(lambda prep: CIS.cis_handle(prep, names_x, names_y, LO, HI, p_value=0.5)))
    method("cis_handle/condition_on/second_call",
           small_cap(lambda prep: CIS.cis_handle(prep, names_x, names_y, LO, HI, p_value=0.5, condition_on=[[3], [], [9]])), k_eff_cap=0)
    method("cis_independent_handle", lambda prep: CC.cis_independent_handle(prep, names_x, names_y, LO, HI, fdr=1.0, permutations=perms,
                                                                             max_signals=2))

    # ---- group 3: the three return-code sites ----
    def failing(name, call, entry):
        for code in (1, 2):
            def run(code=code):
                stub = StubLib(codes={entry: code})
                prep = _prep(stub, Y)
                try:
                    return stub, call(prep, code)
                except Exception as err:                          # the exception is what is recorded
                    return stub, dict(raises=type(err).__name__, text=str(err))
                finally:
                    prep.handle = None
            out[f"{name}/code{code}"] = run
    failing("rank_normalize", lambda prep, code: PR.rank_normalize(Y), "aq_rank_int")
    failing("_ld_prune_handle", lambda prep, code: PR._ld_prune_handle((prep, np.zeros(P, dtype=bool)), _lib.AqPrepLd()), "aq_prep_ld_prune")
    failing("_prepared_from_handle", lambda prep, code: PR._prepared_from_handle(code, HANDLE, "aq_prepare_data_cov", N, P, Q, 0), None)
    return out


def record():
    """name -> dict(calls, result) of every case, with the loaded library put back afterwards."""
    saved = _lib._lib
    try:
        table = {}
        for name, run in cases().items():
            stub, res = run()
            table[name] = dict(calls=encode(stub.calls), result=encode(res))
        return table
    finally:
        _lib._lib = saved


def differences(want, got, where="", rtol=1e-12):
    """Where two recorded values differ: everything must be equal, but a real number may differ by rtol relative (the
    p-values, q-values, cutoffs and beta shapes pass through scipy, whose libm may differ between machines)."""
    if isinstance(want, float) and isinstance(got, float):
        same = (math.isnan(want) and math.isnan(got)) or want == got or abs(want - got) <= rtol * max(abs(want), abs(got))
        return [] if same else [f"{where}: {want!r} != {got!r}"]
    if type(want) is not type(got):
        return [f"{where}: {type(want).__name__} {want!r} != {type(got).__name__} {got!r}"]
    if isinstance(want, dict):
        if sorted(want) != sorted(got):
            return [f"{where}: keys {sorted(want)} != {sorted(got)}"]
        return [d for k in want for d in differences(want[k], got[k], f"{where}/{k}", rtol)]
    if isinstance(want, list):
        if len(want) != len(got):
            return [f"{where}: length {len(want)} != {len(got)}"]
        return [d for i, (a, b) in enumerate(zip(want, got)) for d in differences(a, b, f"{where}[{i}]", rtol)]
    return [] if want == got else [f"{where}: {want!r} != {got!r}"]
