"""What tests/golden/prepare_errors_parent.json and tests/golden/prepare_routes_parent.json hold, computed through the C ABI
alone (ctypes, no prepare.py): tools/record_prepare_errors.py and tools/record_prepare_routes.py wrote the two tables from the
library of the commit before the prepare side was split into units, tests/test_prepare_errors_host.py and
tests/test_gpu_prepare_routes.py compute them again from the library at hand and compare.

  error_rows(L)     (entry, case, rc, message) of every argument error the five aq_prepare_data* entries raise before
                    aq_need_device, through every entry and combination of optional arguments that can reach it.  Every case
                    names device -1, so a case that passes all checks ends in aq_need_device on any machine.
  route_digests(L)  SHA-256 of the raw bytes of everything a prepare handle returns, per route, and of the entries on a finished
                    handle that the split moved (GRM, GRM operator, LD band, LD pruning, rank transform).  Needs the GPU."""
import ctypes as C
import hashlib
import itertools
import os

import numpy as np

from atlasqtl_amd import _lib

N_MAX = 82944                 # AQ_N_MAX of csrc/aq_plan_const.h
NO_DEVICE = (2, "no HIP device visible: libatlasqtl_hip has no CPU fallback (MI355X / gfx950 required)")
BAD_DEVICE = (1, "device ordinal out of range")     # what aq_need_device says of device -1 where a device is visible
u8p = C.POINTER(C.c_uint8)


def clear_env():
    for k in list(os.environ):
        if k.startswith("AQ_") and k != "AQ_LIB":
            del os.environ[k]


def pack_bed(G):
    """n_file x p codes (0 hom A1, 1 missing, 2 het, 3 hom A2) -> the variant-major blocks of a .bed, p x ceil(n_file / 4)."""
    n, p = G.shape
    pad = np.zeros((4 * ((n + 3) // 4), p), dtype=np.uint8)
    pad[:n] = G
    q4 = pad.reshape(-1, 4, p)
    return np.ascontiguousarray((q4[:, 0] | (q4[:, 1] << 2) | (q4[:, 2] << 4) | (q4[:, 3] << 6)).T)


def _cov(d, Z):
    if d is None:
        return None, None
    c = _lib.AqPrepCov()
    c.d, c.Z = d, (None if Z is None else _lib.as_dp(Z))
    return c, Z


def _yt(method, offset=0.375):
    if method is None:
        return None
    y = _lib.AqPrepYtrans()
    y.method, y.offset = method, offset
    return y


def _ref(x):
    return None if x is None else C.byref(x)


def call_entry(L, entry, pin, cov, yt, out):
    """One of the five entries; `pin` is an AqPrepInput, an AqPrepBedInput or None, `out` a c_void_p or None."""
    bed = isinstance(pin, _lib.AqPrepBedInput)
    o = _ref(out)
    if entry == "aq_prepare_data":
        return L.aq_prepare_data(_ref(pin), o)
    if entry == "aq_prepare_data_cov":
        return L.aq_prepare_data_cov(_ref(pin), _ref(cov), o)
    if entry == "aq_prepare_data_bed":
        return L.aq_prepare_data_bed(_ref(pin), o)
    if entry == "aq_prepare_data_bed_cov":
        return L.aq_prepare_data_bed_cov(_ref(pin), _ref(cov), o)
    assert entry == "aq_prepare_data_opt"
    return L.aq_prepare_data_opt(None if bed else _ref(pin), _ref(pin) if bed else None, _ref(cov), _ref(yt), o)


# ------------------------------------------------------------------------------------------------------------------------------
# argument errors

def _dense_input(keep, n=6, p=3, q=2, X="f64", Y=True):
    rng = np.random.default_rng(11)
    Xa = np.asfortranarray(rng.normal(size=(6, 3)))
    Xi = np.asfortranarray(rng.integers(0, 3, size=(6, 3)).astype(np.int8))
    Ya = np.asfortranarray(rng.normal(size=(6, 2)))
    keep += [Xa, Xi, Ya]
    pin = _lib.AqPrepInput()
    pin.n, pin.p, pin.q, pin.device = n, p, q, -1
    pin.X = _lib.as_dp(Xa) if X == "f64" else None
    pin.X_i8 = Xi.ctypes.data_as(C.POINTER(C.c_int8)) if X == "i8" else None
    pin.Y = _lib.as_dp(Ya) if Y else None
    return pin


def _bed_input(keep, n=6, n_file=6, p=3, q=2, bed=True, Y=True, idx=None, count_a2=1, missing=0):
    rng = np.random.default_rng(12)
    blocks = pack_bed(rng.choice(np.array([0, 2, 3], dtype=np.uint8), size=(8, 3)))
    Ya = np.asfortranarray(rng.normal(size=(6, 2)))
    ia = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    keep += [blocks, Ya, ia]
    pin = _lib.AqPrepBedInput()
    pin.n_file, pin.n, pin.p, pin.q, pin.device = n_file, n, p, q, -1
    pin.bed = C.cast(blocks.ctypes.data, u8p) if bed else None
    pin.sample_idx = None if ia is None else _lib.as_ip(ia)
    pin.Y = _lib.as_dp(Ya) if Y else None
    pin.count_a2, pin.missing = count_a2, missing
    return pin


def _good_z(n=6, d=2):
    return np.asfortranarray(np.random.default_rng(13).normal(size=(n, d)))


INPUT_CASES = {
    "dense": [("valid", {}), ("valid_int8", dict(X="i8")), ("null_in", None), ("null_out", {}), ("null_X", dict(X=None)),
              ("null_Y", dict(Y=False)), ("n_1", dict(n=1)), ("p_0", dict(p=0)), ("q_0", dict(q=0))],
    "bed": [("valid", {}), ("valid_subset", dict(n=3, idx=[5, 0, 2])), ("null_in", None), ("null_out", {}), ("null_bed", dict(bed=False)),
            ("null_Y", dict(Y=False)), ("n_1", dict(n=1, idx=[0])), ("p_0", dict(p=0)), ("q_0", dict(q=0)),
            ("n_gt_n_file", dict(n=6, n_file=5)), ("null_idx_n_ne_n_file", dict(n=5, n_file=6)),
            ("idx_negative", dict(n=3, idx=[0, -1, 2])), ("idx_n_file", dict(n=3, idx=[0, 1, 6])), ("count_a2_2", dict(count_a2=2)),
            ("missing_minus_1", dict(missing=-1)), ("missing_2", dict(missing=2))],
}
# the covariate argument: None = the entry is given NULL; else (d, Z or a callable of n)
COV_CASES = [("null", None), ("d_0", (0, None)), ("good", (2, _good_z)), ("null_Z", (2, None)), ("d_97", (97, lambda n: _good_z(n, 97))),
             ("d_minus_1", (-1, _good_z)), ("d_plus_1_eq_n", (5, lambda n: _good_z(n, 5))),
             ("nan_in_Z", (2, lambda n: np.asfortranarray(np.where(np.arange(2 * n).reshape(n, 2, order="F") == n + 1, np.nan, _good_z(n))))),
             ("inf_in_Z", (2, lambda n: np.asfortranarray(np.where(np.arange(2 * n).reshape(n, 2, order="F") == 0, np.inf, _good_z(n))))),
             ("constant_column", (2, lambda n: np.asfortranarray(np.column_stack([_good_z(n)[:, 0], np.full(n, 3.0)])))),
             ("repeated_column", (2, lambda n: np.asfortranarray(np.column_stack([_good_z(n)[:, 0], _good_z(n)[:, 0]]))))]
# the transform argument: None = NULL; else (method, offset)
YT_CASES = [("null", None), ("method_0", (0, 0.375)), ("method_0_bad_offset", (0, 7.0)), ("int", (1, 0.375)), ("offset_0", (1, 0.0)),
            ("offset_half", (1, 0.5)), ("method_2", (2, 0.375)), ("method_minus_1", (-1, 0.375)), ("offset_negative", (1, -0.1)),
            ("offset_0.6", (1, 0.6)), ("offset_nan", (1, float("nan")))]
ENTRIES = {"dense": ("aq_prepare_data", "aq_prepare_data_cov", "aq_prepare_data_opt"),
           "bed": ("aq_prepare_data_bed", "aq_prepare_data_bed_cov", "aq_prepare_data_opt")}


def _error_cases():
    """(entry, case name, kind, input modifiers or None, covariate case, transform case): every combination an entry can express,
    with the input cases crossed with the plain optional arguments only and the optional-argument cases with the valid input."""
    plain_cov, plain_yt = ("null", "d_0", "good"), ("null", "method_0", "int")
    for kind in ("dense", "bed"):
        plain, with_cov, opt = ENTRIES[kind]
        for (iname, mods), (cname, cv), (yname, yv) in itertools.product(INPUT_CASES[kind], COV_CASES, YT_CASES):
            odd_in, odd_cov, odd_yt = not iname.startswith("valid"), cname not in plain_cov, yname not in plain_yt
            if odd_in + odd_cov + odd_yt > 1 and not (odd_cov and odd_yt and not odd_in and cname == "d_97" and yname == "method_2"):
                continue
            case = f"{kind}:{iname}/cov:{cname}/yt:{yname}"
            if cname == "null" and yname == "null":
                yield plain, case, kind, mods, cv, yv
            if yname == "null":
                yield with_cov, case, kind, mods, cv, yv
            yield opt, case, kind, mods, cv, yv
        for cname, yname in (("null", "int"), ("good", "int"), ("null", "method_0")):   # n = AQ_N_MAX + 1; no basis is ever formed
            mods = dict(n=N_MAX + 1) if kind == "dense" else dict(n=N_MAX + 1, n_file=N_MAX + 1)
            yield opt, f"{kind}:n_max_plus_1/cov:{cname}/yt:{yname}", kind, mods, dict(COV_CASES)[cname], dict(YT_CASES)[yname]


def error_rows(L):
    """[entry, case, rc, message] per case, and for aq_prepare_data_opt the cases of its own: both, neither, NULL out."""
    clear_env()
    rows = []
    for entry, case, kind, mods, cv, yv in _error_cases():
        keep = []
        pin = None if mods is None else (_dense_input if kind == "dense" else _bed_input)(keep, **mods)
        if entry == "aq_prepare_data_opt" and pin is None:
            continue                                   # aq_prepare_data_opt without an input: the cases of its own below
        n = 6 if pin is None else pin.n
        if cv is None:
            cov = None
        else:
            # a basis is formed only for n that passed the shape checks: Z has n rows then (6 otherwise, never read)
            Z = cv[1](n if 2 <= n <= 6 else 6) if callable(cv[1]) else None
            cov = _cov(cv[0], Z)[0]
            keep.append(Z)
        out = None if "null_out" in case else C.c_void_p()
        rc = call_entry(L, entry, pin, cov, _yt(*yv) if yv else None, out)
        assert rc != 0 and (out is None or not out.value), (entry, case)      # device -1: nothing can succeed
        rows.append([entry, case, rc, L.aq_last_error().decode()])
    keep = []
    d, b, h = _dense_input(keep), _bed_input(keep), C.c_void_p()
    for case, args in (("opt:both", (C.byref(d), C.byref(b), None, None, C.byref(h))), ("opt:neither", (None, None, None, None, C.byref(h))),
                       ("opt:both/yt:int", (C.byref(d), C.byref(b), None, C.byref(_yt(1)), C.byref(h))),
                       ("opt:neither/null_out", (None, None, None, None, None)), ("opt:dense/null_out", (C.byref(d), None, None, None, None))):
        rc = L.aq_prepare_data_opt(*args)
        rows.append(["aq_prepare_data_opt", case, rc, L.aq_last_error().decode()])
    return rows


# ------------------------------------------------------------------------------------------------------------------------------
# routes on the GPU

N, P, Q = 203, 37, 3
ABSORBED = 7                  # the column that the first covariate equals


def _sha(a):
    return hashlib.sha256(np.asarray(a).tobytes(order="A")).hexdigest()


def route_data(n):
    """Genotype codes n x P with two constant columns (5, 20), two exact duplicates (9 of 3, 30 of 12), columns in LD (15 with 14;
    23, 24 with 22), Y n x Q with 10 % NaN, covariates n x 2 whose first column is genotype column ABSORBED."""
    rng = np.random.default_rng(2037 + n)
    maf = rng.uniform(0.1, 0.5, size=P)
    G = rng.binomial(2, maf, size=(n, P)).astype(np.int8)
    G[:, 5], G[:, 20] = 0, 2
    G[:, 9], G[:, 30] = G[:, 3], G[:, 12]
    for src, dst, flips in ((14, 15, 6), (22, 23, 4), (22, 24, 12)):
        G[:, dst] = G[:, src]
        rows = rng.choice(n, size=flips, replace=False)
        G[rows, dst] = (G[rows, dst] + 1) % 3
    Y = np.asfortranarray(rng.normal(size=(n, Q)) + 0.4 * G[:, [1, 14, 22]])
    Y[rng.random((n, Q)) < 0.10] = np.nan
    Y[:4, :] = [[0.5] * Q, [0.5] * Q, [-1.25] * Q, [2.0] * Q]                 # observed everywhere, with a tie
    Z = np.asfortranarray(np.column_stack([G[:, ABSORBED].astype(np.float64), rng.normal(size=n)]))
    return np.asfortranarray(G), Y, Z


def _codes(G, count_a2):
    """dosages 0 / 1 / 2 -> .bed codes (0 hom A1, 2 het, 3 hom A2) under the counted allele."""
    a2 = G if count_a2 else 2 - G
    return np.array([0, 2, 3], dtype=np.uint8)[a2]


def _sources(n):
    """name -> (ctypes input with device 0, the arrays it points into) for the five sources of the matrix."""
    G, Y, Z = route_data(n)
    rng = np.random.default_rng(77 + n)
    X64 = np.asfortranarray(G.astype(np.float64))
    X64[:, [2, 17, 33]] += 0.25 * rng.normal(size=(n, 3))                     # not every fp64 column is a dosage

    def dense(X):
        pin = _lib.AqPrepInput()
        pin.n, pin.p, pin.q, pin.device, pin.Y = n, P, Q, 0, _lib.as_dp(Y)
        pin.X = _lib.as_dp(X) if X.dtype == np.float64 else None
        pin.X_i8 = X.ctypes.data_as(C.POINTER(C.c_int8)) if X.dtype == np.int8 else None
        return pin, [X, Y]

    def bed(codes, idx, count_a2, missing):
        blocks = pack_bed(codes)
        ia = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
        pin = _lib.AqPrepBedInput()
        pin.n_file, pin.n, pin.p, pin.q, pin.device, pin.Y = codes.shape[0], n, P, Q, 0, _lib.as_dp(Y)
        pin.bed, pin.sample_idx = C.cast(blocks.ctypes.data, u8p), (None if ia is None else _lib.as_ip(ia))
        pin.count_a2, pin.missing = count_a2, missing
        return pin, [blocks, ia, Y]

    mis = _codes(G, 1)
    holes = rng.random((n, P)) < 0.03
    holes[:, [3, 9, ABSORBED]] = False                                         # the duplicates stay duplicates
    mis[holes] = 1
    idx = rng.permutation(n + 57)[:n]                                          # a subset of a larger file, in no order
    full = rng.choice(np.array([0, 2, 3], dtype=np.uint8), size=(n + 57, P))
    full[idx] = _codes(G, 0)
    return dict(f64=dense(X64), i8=dense(G), bed=bed(_codes(G, 1), None, 1, 0), bed_missing=bed(mis, None, 1, 1),
                bed_subset=bed(full, idx, 0, 0)), Y, Z


def _handle_digests(L, h, n):
    """Everything the handle returns through aq_prep_get and the four info entries."""
    out = {}
    pk = C.c_int32(-1)
    cst, coll, dup = np.zeros(P, np.uint8), np.zeros(P, np.uint8), np.zeros(P, np.int32)
    mean, sd = np.zeros(P), np.zeros(P)
    _lib.check(L.aq_prep_info(h, C.byref(pk), cst.ctypes.data_as(u8p), coll.ctypes.data_as(u8p), _lib.as_ip(dup), _lib.as_dp(mean),
                              _lib.as_dp(sd)), "aq_prep_info")
    out["p_kept"] = int(pk.value)
    out.update(bool_cst=_sha(cst), bool_coll=_sha(coll), dup_of=_sha(dup), x_mean=_sha(mean), x_sd=_sha(sd))
    X, Y = np.zeros((n, pk.value), order="F"), np.zeros((n, Q), order="F")
    _lib.check(L.aq_prep_get(h, _lib.as_dp(X), _lib.as_dp(Y)), "aq_prep_get")
    out.update(X=_sha(X), Y=_sha(Y))
    d, ab, r2 = C.c_int32(-1), np.zeros(P, np.uint8), np.zeros(P)
    _lib.check(L.aq_prep_cov_info(h, C.byref(d), ab.ctypes.data_as(u8p), _lib.as_dp(r2)), "aq_prep_cov_info")
    out.update(n_cov=int(d.value), n_absorbed=int(ab.sum()), cov_absorbed=_sha(ab), cov_r2=_sha(r2))
    m, off, nobs, ntied = C.c_int32(-1), C.c_double(-1.0), np.zeros(Q, np.int32), np.zeros(Q, np.int32)
    _lib.check(L.aq_prep_ytrans_info(h, C.byref(m), C.byref(off), _lib.as_ip(nobs), _lib.as_ip(ntied)), "aq_prep_ytrans_info")
    out.update(yt_method=int(m.value), yt_offset=float(off.value), yt_n_obs=_sha(nobs), yt_n_tied=_sha(ntied))
    counts = np.zeros((4, P), dtype=np.int32, order="F")
    out["genotype_counts_rc"] = int(L.aq_prep_genotype_counts(h, _lib.as_ip(counts)))
    out["genotype_counts"] = _sha(counts)
    return out


def _finished_handle_digests(L, h, n):
    """The entries on a finished handle, in this order: GRM, GRM operator at two padded widths, LD band, LD pruning."""
    out = {}
    rng = np.random.default_rng(5 + n)
    K, tr = np.zeros((n, n), order="F"), C.c_double(0.0)
    _lib.check(L.aq_prep_grm(h, _lib.as_dp(K), C.byref(tr)), "aq_prep_grm")
    out.update(grm=_sha(K), grm_trace=_sha(np.float64(tr.value)))
    for width in (5, 17):
        Qm, Zm, tr = np.asfortranarray(rng.normal(size=(n, width))), np.zeros((n, width), order="F"), C.c_double(0.0)
        _lib.check(L.aq_prep_grm_apply(h, _lib.as_dp(Qm), width, _lib.as_dp(Zm), C.byref(tr)), "aq_prep_grm_apply")
        out[f"grm_apply_{width}"], out[f"grm_apply_{width}_trace"] = _sha(Zm), _sha(np.float64(tr.value))
    pk = C.c_int32(-1)
    _lib.check(L.aq_prep_info(h, C.byref(pk), None, None, None, None, None), "aq_prep_info")
    band = np.zeros((pk.value, 8), order="F")
    _lib.check(L.aq_prep_ld_band(h, 8, _lib.as_dp(band)), "aq_prep_ld_band")
    out["ld_band"] = _sha(band)
    ld = _lib.AqPrepLd()
    ld.window, ld.r2, ld.group, ld.pos, ld.window_bp = 8, 0.5, None, None, 0
    _lib.check(L.aq_prep_ld_prune(h, C.byref(ld)), "aq_prep_ld_prune")
    rm, of, r2 = np.zeros(P, np.uint8), np.zeros(P, np.int32), np.zeros(P)
    _lib.check(L.aq_prep_ld_info(h, C.byref(pk), rm.ctypes.data_as(u8p), _lib.as_ip(of), _lib.as_dp(r2)), "aq_prep_ld_info")
    X = np.zeros((n, pk.value), order="F")
    _lib.check(L.aq_prep_get(h, _lib.as_dp(X), None), "aq_prep_get")
    out.update(ld_p_kept=int(pk.value), ld_removed=_sha(rm), ld_of=_sha(of), ld_r2=_sha(r2), ld_X=_sha(X))
    return out


def route_digests(L):
    """route name -> {field: digest or small integer}, each route through the entry that is named for it (aq_prepare_data_opt
    where Y is transformed).  Stops at the first entry that fails (_lib.check raises)."""
    clear_env()
    table = {}
    for n, wanted in ((N, None), (N + 1, ("i8", "bed"))):
        sources, Y, Z = _sources(n)
        for (src, (pin, keep)), d, method in itertools.product(sources.items(), (0, 2), (0, 1)):
            if wanted is not None and (src not in wanted or d or method):
                continue
            name = f"n{n}/{src}/cov{d}/yt{method}"
            cov, yt, h = (_cov(2, Z)[0] if d else None), (_yt(1) if method else None), C.c_void_p()
            entry = "aq_prepare_data_opt" if method else ENTRIES["dense" if src in ("f64", "i8") else "bed"][1 if d else 0]
            _lib.check(call_entry(L, entry, pin, cov, yt, h), name)
            try:
                table[name] = _handle_digests(L, h, n)
                if src in ("i8", "bed") and not d and not method:
                    table[name].update(_finished_handle_digests(L, h, n))
            finally:
                L.aq_prep_destroy(h)
        out, nobs, ntied = np.zeros((n, Q), order="F"), np.zeros(Q, np.int32), np.zeros(Q, np.int32)
        _lib.check(L.aq_rank_int(_lib.as_dp(Y), n, Q, 0.375, _lib.as_dp(out), _lib.as_ip(nobs), _lib.as_ip(ntied), 0), "aq_rank_int")
        table[f"n{n}/aq_rank_int"] = dict(Y=_sha(out), n_obs=_sha(nobs), n_tied=_sha(ntied))
    return table
