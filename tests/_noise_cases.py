# -*- coding: utf-8 -*-
"""Inputs of the linear noise model's tests (test_batch_noise_cpu.py, test_gpu_batch_noise.py): bases with mixed signs and
magnitudes spread over three decades, weights that keep every variance positive, the NumPy statement of the model and of
its gradient."""
import math

import numpy as np

from oracle import ref
from _cases import NO_GENERAL, coeffs_of

KEEP = 0.9          # sum_k |s_k Psi_k| <= KEEP * diag: diag_eff >= 0.1 diag > 0


def noise_basis(diag, K, per, seed=0):
    """``Psi`` for the diagonal ``diag`` (B, N): ``(B, K, N)`` (``per``) or ``(K, N)``.  ``Psi_k[n] = +-10^(-3 u) d[n]``
    with ``u`` uniform in [0, 1], random signs, and ``d`` the problem's diagonal (shared basis: the smallest diagonal over
    the problems), so that ``|Psi_k| <= diag`` for every problem."""
    rng = np.random.RandomState(1000 + seed)
    d = np.asarray(diag, dtype=np.float64)
    d = d if per else (d.min(axis=0) if d.ndim == 2 else d)
    shape = d.shape[:-1] + (K, d.shape[-1])
    q = np.where(rng.rand(*shape) < 0.5, -1.0, 1.0) * 10.0 ** (-3.0 * rng.rand(*shape))
    return np.ascontiguousarray(q * d[..., None, :])


def noise_weights(B, K, seed=0):
    """``s`` (B, K), uniform in ``[-KEEP / K, KEEP / K]``: with :func:`noise_basis` every variance stays positive."""
    return np.random.RandomState(2000 + seed).uniform(-1.0, 1.0, (B, K)) * (KEEP / K)


def host_diag(diag, s, Psi):
    """The expression the device's variances are the bits of: ``diag + (s_0 * Psi_0 + s_1 * Psi_1 + ...)``, (B, N)."""
    B, K = s.shape
    P = np.broadcast_to(Psi, (B, K, Psi.shape[-1]))
    m = s[:, 0, None] * P[:, 0]
    for k in range(1, K):
        m = m + s[:, k, None] * P[:, k]
    return diag + m


def noise_gradient(Psi_b, alpha, c):
    """``(g[K], S[K])`` of one problem: ``g_k = 1/2 sum_n Psi_k[n] (alpha_n^2 - c_n)`` and the scale its deviations are
    measured against, ``S_k = 1/2 sum_n |Psi_k[n]| (alpha_n^2 + c_n)``, both summed with ``math.fsum``."""
    g = [0.5 * math.fsum(Psi_b[k] * (alpha * alpha - c)) for k in range(Psi_b.shape[0])]
    S = [0.5 * math.fsum(np.abs(Psi_b[k]) * (alpha * alpha + c)) for k in range(Psi_b.shape[0])]
    return np.array(g), np.array(S)


def oracle_c_alpha(case, p, diag_p, resid_p):
    """``(c, alpha)`` of problem ``p`` on the diagonal ``diag_p`` as tests/test_gpu_batch_leave_one_out.py obtains them:
    ``diag(RefSolver.solve(I))`` and ``RefSolver.solve(r)``."""
    N = len(diag_p)
    r = ref.RefSolver()
    r.compute(0.0, *coeffs_of(case, p), *NO_GENERAL, case["t"][p], diag_p)
    return np.diag(r.solve(np.eye(N))).copy(), np.asarray(r.solve(resid_p)).reshape(N)


def oracle_gradient(case, s, Psi, resid=None):
    """``(g[B, K], S[B, K])`` of every problem from the oracle's c and alpha on the host-formed diagonal."""
    B, K = s.shape
    d = host_diag(case["diag"], s, Psi)
    P = np.broadcast_to(Psi, (B, K, Psi.shape[-1]))
    resid = case["y"] if resid is None else resid
    g, S = np.empty((B, K)), np.empty((B, K))
    for p in range(B):
        c, a = oracle_c_alpha(case, p, d[p], resid[p])
        g[p], S[p] = noise_gradient(P[p], a, c)
    return g, S
