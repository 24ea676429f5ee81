# -*- coding: utf-8 -*-
"""Inputs of the amplitude model's tests (test_batch_amplitude_cpu.py, test_gpu_batch_amplitude.py): band-indicator and
non-indicator bases, amplitudes of one sign per problem that keep ``|s|`` away from zero, the NumPy statement of the model
(``host_scale``, ``host_series``, ``log_sum``) and of its gradients."""
import math

import numpy as np

from _noise_cases import oracle_c_alpha

S_MIN = 0.25        # the tests assert min |s| >= S_MIN on every input they use


def band_basis(B, N, K, per, seed=0):
    """The indicators of K bands with a random assignment of the samples: ``(B, K, N)`` (``per``: an assignment per
    problem) or ``(K, N)``.  Every band holds a sample when N >= K."""
    rng = np.random.RandomState(3000 + seed)

    def one():
        band = rng.randint(0, K, N)
        band[rng.permutation(N)[:min(K, N)]] = np.arange(min(K, N))
        return (band[None, :] == np.arange(K)[:, None]).astype(np.float64)

    return np.ascontiguousarray(np.stack([one() for _ in range(B)]) if per else one())


def smooth_basis(B, N, K, per, seed=0):
    """A non-indicator basis: ``Gamma_k >= 0`` and ``sum_k Gamma_k >= 0.5`` -- ``Gamma_0`` in [0.5, 1], the others random
    in [0, 1] times a slow modulation."""
    rng = np.random.RandomState(3500 + seed)
    x = np.linspace(0.0, 1.0, N)

    def one():
        rows = [0.5 + 0.5 * rng.rand(N)]
        for k in range(1, K):
            rows.append(rng.rand(N) * (0.5 + 0.5 * np.cos((k + 1) * x + rng.rand())) ** 2)
        return np.stack(rows)

    return np.ascontiguousarray(np.stack([one() for _ in range(B)]) if per else one())


def amplitudes(B, K, seed=0):
    """``a`` (B, K): one sign per problem, magnitudes in [0.5, 2] with band-to-band ratios up to 4; problem 0 is positive,
    problem 1 (if there is one) negative, the others random."""
    rng = np.random.RandomState(4000 + seed)
    a = 0.5 * 4.0 ** rng.rand(B, K)
    sign = np.where(rng.rand(B) < 0.5, -1.0, 1.0)
    sign[0] = 1.0
    if B > 1:
        sign[1] = -1.0
    return a * sign[:, None]


def host_scale(a, Gamma):
    """The expression the device's scale is the bits of: ``a_0 * Gamma_0 + a_1 * Gamma_1 + ...`` in this order, (B, N)."""
    B, K = a.shape
    G = np.broadcast_to(Gamma, (B, K, Gamma.shape[-1]))
    s = a[:, 0, None] * G[:, 0]
    for k in range(1, K):
        s = s + a[:, k, None] * G[:, k]
    return s


def host_series(r, d, s):
    """``(y', d')``: ``r / s`` and ``d / (s * s)``, each (B, N)."""
    return r / s, d / (s * s)


def log_sum(s, lengths=None):
    """``L[b] = sum_n log|s[b, n]|`` over each problem's length, summed with ``math.fsum``; and ``sum_n |log|s_n||``, the
    scale its deviations are measured against."""
    B, N = s.shape
    lens = [N] * B if lengths is None else lengths
    L = np.array([math.fsum(np.log(np.abs(s[b, :n]))) for b, n in enumerate(lens)])
    A = np.array([math.fsum(np.abs(np.log(np.abs(s[b, :n])))) for b, n in enumerate(lens)])
    return L, A


def amplitude_gradient(Gamma_b, alpha, c, yp, dp, s):
    """``(g[K], S[K])`` of one problem: ``g_k = sum_n Gamma_k[n] (alpha_n y'_n + d'_n (c_n - alpha_n^2) - 1) / s_n`` and the
    scale ``S_k = sum_n |Gamma_k[n]| (|alpha_n y'_n| + d'_n (c_n + alpha_n^2) + 1) / |s_n|``, summed with ``math.fsum``."""
    f = (alpha * yp + dp * (c - alpha * alpha) - 1.0) / s
    w = (np.abs(alpha * yp) + dp * (c + alpha * alpha) + 1.0) / np.abs(s)
    K = Gamma_b.shape[0]
    return (np.array([math.fsum(Gamma_b[k] * f) for k in range(K)]),
            np.array([math.fsum(np.abs(Gamma_b[k]) * w) for k in range(K)]))


def mean_gradient_scaled(Phi_b, alpha, s):
    """``grad_mean_weights`` with amplitudes in force: ``g_k = sum_n Phi_k[n] alpha'_n / s_n``, scale with absolute values."""
    K = Phi_b.shape[0]
    return (np.array([math.fsum(Phi_b[k] * alpha / s) for k in range(K)]),
            np.array([math.fsum(np.abs(Phi_b[k] * alpha / s)) for k in range(K)]))


def noise_gradient_scaled(Psi_b, alpha, c, s):
    """``grad_noise_weights`` with amplitudes in force: ``g_k = 1/2 sum_n Psi_k[n] (alpha'_n^2 - c'_n) / s_n^2``, scale
    ``1/2 sum_n |Psi_k[n]| (alpha'_n^2 + c'_n) / s_n^2``."""
    K = Psi_b.shape[0]
    return (np.array([0.5 * math.fsum(Psi_b[k] * (alpha * alpha - c) / (s * s)) for k in range(K)]),
            np.array([0.5 * math.fsum(np.abs(Psi_b[k]) * (alpha * alpha + c) / (s * s)) for k in range(K)]))


def oracle_gradient(case, a, Gamma, resid=None, diag=None):
    """``(g[B, K], S[B, K])`` of every problem from the oracle's c and alpha (``RefSolver``) on the host-formed series."""
    B, K = a.shape
    s = host_scale(a, Gamma)
    yp, dp = host_series(case["y"] if resid is None else resid, case["diag"] if diag is None else diag, s)
    G = np.broadcast_to(Gamma, (B, K, Gamma.shape[-1]))
    g, S = np.empty((B, K)), np.empty((B, K))
    for p in range(B):
        c, al = oracle_c_alpha(case, p, dp[p], yp[p])
        g[p], S[p] = amplitude_gradient(G[p], al, c, yp[p], dp[p], s[p])
    return g, S
