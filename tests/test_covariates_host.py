"""Host: the covariate argument of the device-side preparation (aq_cov_basis, aq_prepare_data_cov, aq_prepare_data_bed_cov,
prepare_on_device(covariates=)) -- the basis against the long-double restatement of tests/cov_util.py, and every argument
error, which must come before the first device call: all of this runs on a machine without a GPU."""
import ctypes as C

import numpy as np
import pytest

from atlasqtl_amd import _lib
from tests import cov_util as CU


def _basis(hiplib, Z):
    Z = np.asfortranarray(Z, dtype=np.float64)
    n, d = Z.shape
    Q = np.full((n, d + 1), np.nan, order="F")
    bad = C.c_int32(-7)
    rc = hiplib.aq_cov_basis(_lib.as_dp(Z), n, d, _lib.as_dp(Q), C.byref(bad))
    return rc, Q, bad.value, hiplib.aq_last_error().decode()


@pytest.mark.parametrize("n,d", [(50, 1), (333, 5), (200, 96), (5000, 32)])
def test_basis_matches_the_long_double_restatement(hiplib, n, d):
    Z = CU.covariates(n, d, np.random.default_rng(n + d))
    rc, Q, bad, _ = _basis(hiplib, Z)
    assert rc == 0 and bad == -1
    W = CU.with_intercept(Z)
    Q_ref, bad_ref = CU.basis_ld(W)
    assert bad_ref is None
    assert np.all(Q[:, 0] == 1.0 / np.sqrt(float(n)))
    assert np.abs(Q.T @ Q - np.eye(d + 1)).max() <= 1e-13
    Ql, Wl = Q.astype(CU.LD), W.astype(CU.LD)
    back = Ql @ (Ql.T @ Wl) - Wl
    assert np.sqrt((back ** 2).sum()) <= 1e-12 * np.sqrt((Wl ** 2).sum())
    assert (np.sqrt((back ** 2).sum(0)) <= 1e-12 * np.sqrt((Wl ** 2).sum(0))).all()      # column by column: the scales differ
    assert np.abs(Q - Q_ref.astype(np.float64)).max() <= 1e-12


@pytest.mark.parametrize("kind", ["constant", "duplicate", "sum"])
def test_collinear_covariate_is_named(hiplib, kind):
    n, d = 120, 6
    Z = CU.covariates(n, d, np.random.default_rng(3))
    if kind == "constant":
        col = 2
        Z[:, col] = 37.5
    elif kind == "duplicate":
        col = 4
        Z[:, col] = Z[:, 1]
    else:
        col = 5
        Z[:, col] = Z[:, 0] + Z[:, 3]
    rc, _, bad, msg = _basis(hiplib, Z)
    assert rc == 1 and bad == col
    assert f"column {col + 1} of the covariates is collinear" in msg
    assert CU.basis_ld(CU.with_intercept(Z))[1] == col + 1            # the restatement's rule names the same column of W
    # from both preparation entries and from Python, before any device call
    for call in (_call_cov, _call_bed_cov):
        rc, msg = call(hiplib, n, Z)
        assert rc == 1 and f"column {col + 1} of the covariates is collinear" in msg
    from atlasqtl_amd.prepare import AtlasqtlError, prepare_on_device
    rng = np.random.default_rng(0)
    with pytest.raises(AtlasqtlError, match=f"column {col + 1} of the covariates is collinear"):
        prepare_on_device(rng.normal(size=(n, 3)), rng.normal(size=(n, 8)), covariates=Z)


def _call_cov(hiplib, n, Z, p=5, q=2):
    rng = np.random.default_rng(1)
    X = np.asfortranarray(rng.normal(size=(n, p)))
    Y = np.asfortranarray(rng.normal(size=(n, q)))
    Z = np.asfortranarray(Z, dtype=np.float64)
    pin = _lib.AqPrepInput()
    pin.n, pin.p, pin.q, pin.X, pin.X_i8, pin.Y, pin.device = n, p, q, _lib.as_dp(X), None, _lib.as_dp(Y), 0
    cov = _lib.AqPrepCov()
    cov.d, cov.Z = Z.shape[1], _lib.as_dp(Z)
    h = C.c_void_p()
    rc = hiplib.aq_prepare_data_cov(C.byref(pin), C.byref(cov), C.byref(h))
    assert rc != 0 and not h.value
    return rc, hiplib.aq_last_error().decode()


def _call_bed_cov(hiplib, n, Z, p=5, q=2):
    rng = np.random.default_rng(1)
    blocks = np.zeros((p, (n + 3) // 4), dtype=np.uint8)
    Y = np.asfortranarray(rng.normal(size=(n, q)))
    Z = np.asfortranarray(Z, dtype=np.float64)
    pin = _lib.AqPrepBedInput()
    pin.n_file, pin.n, pin.p, pin.q = n, n, p, q
    pin.bed, pin.sample_idx, pin.Y = C.cast(blocks.ctypes.data, C.POINTER(C.c_uint8)), None, _lib.as_dp(Y)
    pin.count_a2, pin.missing, pin.device = 0, 0, 0
    cov = _lib.AqPrepCov()
    cov.d, cov.Z = Z.shape[1], _lib.as_dp(Z)
    h = C.c_void_p()
    rc = hiplib.aq_prepare_data_bed_cov(C.byref(pin), C.byref(cov), C.byref(h))
    assert rc != 0 and not h.value
    return rc, hiplib.aq_last_error().decode()


@pytest.mark.parametrize("call", [_call_cov, _call_bed_cov])
def test_argument_errors_come_before_the_device(hiplib, call):
    """AQ_ERR_ARG (1) with a message about the covariates, not AQ_ERR_DEVICE "no HIP device": with or without a GPU."""
    rng = np.random.default_rng(2)
    n = 150
    Z = rng.normal(size=(n, 4))
    for bad_value in (np.nan, np.inf):
        Zb = Z.copy()
        Zb[17, 2] = bad_value
        rc, msg = call(hiplib, n, Zb)
        assert rc == 1 and "covariates must be" in msg and "finite" in msg
    rc, msg = call(hiplib, n, rng.normal(size=(n, 97)))                 # d = 97
    assert rc == 1 and "between 1 and 96" in msg and "97 given" in msg
    rc, msg = call(hiplib, 20, rng.normal(size=(20, 19)))               # D = d + 1 = n
    assert rc == 1 and "need more than 20 samples, n = 20" in msg
    rc, msg = call(hiplib, 20, rng.normal(size=(20, 30)))               # D > n
    assert rc == 1 and "need more than 31 samples, n = 20" in msg
    # a NULL covariate pointer with d > 0
    pin = _lib.AqPrepInput()
    X = np.asfortranarray(rng.normal(size=(n, 3)))
    pin.n, pin.p, pin.q, pin.X, pin.X_i8, pin.Y, pin.device = n, 3, 1, _lib.as_dp(X), None, _lib.as_dp(X), 0
    cov = _lib.AqPrepCov()
    cov.d, cov.Z = 2, None
    h = C.c_void_p()
    assert hiplib.aq_prepare_data_cov(C.byref(pin), C.byref(cov), C.byref(h)) == 1
    assert "NULL covariate pointer" in hiplib.aq_last_error().decode()
    assert hiplib.aq_cov_basis(None, 10, 2, None, None) == 1
    assert hiplib.aq_prep_cov_info(None, None, None, None) == 1


def test_python_validates_before_the_device():
    from atlasqtl_amd.prepare import AtlasqtlError, prepare_on_device
    rng = np.random.default_rng(4)
    n = 60
    Y, X = rng.normal(size=(n, 3)), rng.normal(size=(n, 7))
    with pytest.raises(AtlasqtlError, match="same number of samples"):
        prepare_on_device(Y, X, covariates=rng.normal(size=(n - 1, 2)))
    with pytest.raises(AtlasqtlError, match="covariates must be"):
        prepare_on_device(Y, X, covariates=rng.normal(size=n))          # not 2-D
    Z = rng.normal(size=(n, 2))
    Z[3, 1] = np.nan
    with pytest.raises(AtlasqtlError, match="covariates must be"):
        prepare_on_device(Y, X, covariates=Z)
    with pytest.raises(AtlasqtlError, match="between 1 and 96"):
        prepare_on_device(rng.normal(size=(300, 2)), rng.normal(size=(300, 4)), covariates=rng.normal(size=(300, 97)))
    with pytest.raises(AtlasqtlError, match="need more than"):
        prepare_on_device(Y, X.astype(np.int8), covariates=rng.normal(size=(n, n - 1)))
    import atlasqtl_amd as A
    with pytest.raises(AtlasqtlError, match="same number of samples"):
        A.atlasqtl(Y, X, p0=(2, 4), verbose=0, covariates=rng.normal(size=(n + 2, 2)))
