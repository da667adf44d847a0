"""The reference's two in-place operators, with the arithmetic done by libatlasqtl_hip.so on the GPU:

  coreDualLoop(...) / coreDualMisLoop(...)     R/RcppExports.R:4-10  (in place, as the reference)
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import as_dp, as_ip, check, lib


def _f64F(a, name, shape=None):
    a = np.asarray(a)
    if a.dtype != np.float64 or not a.flags.f_contiguous:
        raise TypeError(f"{name} must be a float64 Fortran-ordered (R layout) array; it is updated in place")
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
    return a


def _vec(a, name, n):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (n,):
        raise ValueError(f"{name} must have length {n}")
    return a


def coreDualLoop(cp_X, cp_Y_X, gam_vb, log_Phi_theta_plus_zeta, log_1_min_Phi_theta_plus_zeta, log_sig2_inv_vb,
                 log_tau_vb, m1_beta, cp_betaX_X, mu_beta_vb, sig2_beta_vb, tau_vb, shuffled_ind, sample_q, c=1.0):
    """R/RcppExports.R:4-6 -> src/coreLoop.cpp:38-86.  gam_vb, m1_beta, cp_betaX_X, mu_beta_vb are
    modified in place (they must be float64 Fortran-ordered p x q arrays); returns None."""
    gam_vb = _f64F(gam_vb, "gam_vb")
    p, q = gam_vb.shape
    cp_X = _f64F(np.asfortranarray(cp_X, dtype=np.float64), "cp_X", (p, p))
    cp_Y_X = _f64F(np.asfortranarray(cp_Y_X, dtype=np.float64), "cp_Y_X", (q, p))
    lP = _f64F(np.asfortranarray(log_Phi_theta_plus_zeta, dtype=np.float64), "log_Phi_theta_plus_zeta", (p, q))
    l1 = _f64F(np.asfortranarray(log_1_min_Phi_theta_plus_zeta, dtype=np.float64), "log_1_min_Phi_theta_plus_zeta",
               (p, q))
    m1_beta = _f64F(m1_beta, "m1_beta", (p, q))
    cp_betaX_X = _f64F(cp_betaX_X, "cp_betaX_X", (p, q))
    mu_beta_vb = _f64F(mu_beta_vb, "mu_beta_vb", (p, q))
    lt = _vec(log_tau_vb, "log_tau_vb", q)
    s2 = _vec(sig2_beta_vb, "sig2_beta_vb", q)
    tv = _vec(tau_vb, "tau_vb", q)
    si = np.ascontiguousarray(shuffled_ind, dtype=np.int32)
    sq = np.ascontiguousarray(sample_q, dtype=np.int32)
    rc = lib().aq_core_dual_loop(as_dp(cp_X), as_dp(cp_Y_X), as_dp(gam_vb), as_dp(lP), as_dp(l1),
                                 float(log_sig2_inv_vb), as_dp(lt), as_dp(m1_beta), as_dp(cp_betaX_X),
                                 as_dp(mu_beta_vb), as_dp(s2), as_dp(tv), as_ip(si), len(si), as_ip(sq), len(sq),
                                 float(c), p, q)
    check(rc, "coreDualLoop")


def coreDualMisLoop(cp_X, cp_X_rm, cp_Y_X, gam_vb, log_Phi_theta_plus_zeta, log_1_min_Phi_theta_plus_zeta,
                    log_sig2_inv_vb, log_tau_vb, m1_beta, cp_betaX_X, mu_beta_vb, sig2_beta_vb, tau_vb, shuffled_ind,
                    sample_q, c=1.0):
    """R/RcppExports.R:8-10 -> src/coreLoop.cpp:91-138.  cp_X_rm: list of q (p x p) matrices;
    sig2_beta_vb: p x q.  In place like coreDualLoop."""
    gam_vb = _f64F(gam_vb, "gam_vb")
    p, q = gam_vb.shape
    if len(cp_X_rm) != q:
        raise ValueError("cp_X_rm must be a list of q matrices")
    cp_X = np.asfortranarray(cp_X, dtype=np.float64)
    rms = [_f64F(np.asfortranarray(m, dtype=np.float64), "cp_X_rm[[k]]", (p, p)) for m in cp_X_rm]
    arr = (_lib.dp * q)(*[as_dp(m) for m in rms])
    cp_Y_X = np.asfortranarray(cp_Y_X, dtype=np.float64)
    lP = np.asfortranarray(log_Phi_theta_plus_zeta, dtype=np.float64)
    l1 = np.asfortranarray(log_1_min_Phi_theta_plus_zeta, dtype=np.float64)
    m1_beta = _f64F(m1_beta, "m1_beta", (p, q))
    cp_betaX_X = _f64F(cp_betaX_X, "cp_betaX_X", (p, q))
    mu_beta_vb = _f64F(mu_beta_vb, "mu_beta_vb", (p, q))
    s2 = _f64F(np.asfortranarray(sig2_beta_vb, dtype=np.float64), "sig2_beta_vb", (p, q))
    lt = _vec(log_tau_vb, "log_tau_vb", q)
    tv = _vec(tau_vb, "tau_vb", q)
    si = np.ascontiguousarray(shuffled_ind, dtype=np.int32)
    sq = np.ascontiguousarray(sample_q, dtype=np.int32)
    rc = lib().aq_core_dual_mis_loop(as_dp(cp_X), arr, as_dp(cp_Y_X), as_dp(gam_vb), as_dp(lP), as_dp(l1),
                                     float(log_sig2_inv_vb), as_dp(lt), as_dp(m1_beta), as_dp(cp_betaX_X),
                                     as_dp(mu_beta_vb), as_dp(s2), as_dp(tv), as_ip(si), len(si), as_ip(sq), len(sq),
                                     float(c), p, q)
    check(rc, "coreDualMisLoop")
