# -*- coding: utf-8 -*-
"""Shared by the tests of the linear mean's generalised-least-squares fit (fit_mean_weights / clr_gram_solve): the basis the
accuracy cases use, the long-double Cholesky solve they are held against, and the forward bound of the small solve."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def fit_basis(t, K):
    """``[1, 2u - 1, sin 6 pi u, cos 6 pi u, sin 12 pi u, cos 12 pi u, ...]`` with ``u = (t - t_min) / (t_max - t_min)``
    at the times ``t`` (..., N) -> (..., K, N).  Well conditioned on the bench family: every Cholesky pivot of the
    unit-diagonal Gram matrix is >= 0.99 there."""
    t = np.asarray(t, dtype=np.float64)
    lo, hi = t.min(axis=-1, keepdims=True), t.max(axis=-1, keepdims=True)
    u = (t - lo) / (hi - lo)
    rows = [np.ones_like(u), 2.0 * u - 1.0]
    j = 1
    while len(rows) < K:
        rows.append(np.sin(6.0 * np.pi * j * u))
        rows.append(np.cos(6.0 * np.pi * j * u))
        j += 1
    return np.stack(rows[:K], axis=-2)


def ld_cholesky(A):
    """The lower Cholesky factor of a symmetric positive definite matrix in long double (unpivoted)."""
    A = np.asarray(A, dtype=LD)
    K = A.shape[0]
    L = np.zeros((K, K), dtype=LD)
    for j in range(K):
        p = A[j, j] - np.sum(L[j, :j] * L[j, :j])
        assert p > 0, "not positive definite"
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, K):
            L[i, j] = (A[i, j] - np.sum(L[i, :j] * L[j, :j])) / L[j, j]
    return L


def ld_tri_solve(L, b, transpose=False):
    K = L.shape[0]
    x = np.zeros(K, dtype=LD)
    order = range(K - 1, -1, -1) if transpose else range(K)
    for i in order:
        if transpose:
            x[i] = (b[i] - np.sum(L[i + 1:, i] * x[i + 1:])) / L[i, i]
        else:
            x[i] = (b[i] - np.sum(L[i, :i] * x[:i])) / L[i, i]
    return x


def ld_fit(S, w0):
    """From one bordered Gram matrix ``[[G, d], [d^T, q]]`` (any float type) and the start weights, in long double:
    ``dict(weights, covariance, logdet_gram, quad, kappa_s)`` -- ``w0 + G^-1 d``, ``G^-1``, ``log det G``,
    ``q - d^T G^-1 d`` and the 2-norm condition number of the unit-diagonal ``G_s`` (float)."""
    S = np.asarray(S, dtype=LD)
    K = S.shape[0] - 1
    G, d, q = S[:K, :K], S[:K, K], S[K, K]
    s = 1 / np.sqrt(np.diag(G))
    Gs = G * s[:, None] * s[None, :]
    L = ld_cholesky(Gs)
    delta = s * ld_tri_solve(L, ld_tri_solve(L, s * d), transpose=True)
    inv = np.empty((K, K), dtype=LD)
    for k in range(K):
        e = np.zeros(K, dtype=LD)
        e[k] = 1
        inv[:, k] = ld_tri_solve(L, ld_tri_solve(L, e), transpose=True)
    cov = inv * s[:, None] * s[None, :]
    logdet = np.sum(np.log(np.diag(G))) + 2 * np.sum(np.log(np.diag(L)))
    return dict(weights=np.asarray(w0, dtype=LD) + delta, covariance=cov, logdet_gram=logdet, quad=q - np.sum(d * delta),
                kappa_s=float(np.linalg.cond(Gs.astype(np.float64))))


def small_solve_bound(K, kappa_s):
    """The first-order forward bound of a K x K Cholesky solve, (3 K + 1) 2^-52 kappa_2(G_s) (Higham, Accuracy and
    Stability of Numerical Algorithms, theorem 10.4), relative to 1 + |value|."""
    return (3 * K + 1) * EPS * kappa_s


def small_solve_errors(truth, weights, covariance, logdet_gram, quad):
    """Deviations of a small solve's float64 results from ``ld_fit``'s, each relative to ``1 + |value|``, entry by
    entry: ``dict(name -> float)``."""
    cov_t = truth["covariance"]
    return dict(
        weights=float(np.max(np.abs(weights - truth["weights"]) / (1 + np.abs(truth["weights"])))),
        covariance=float(np.max(np.abs(covariance - cov_t) / (1 + np.abs(cov_t)))),
        logdet_gram=float(abs(logdet_gram - truth["logdet_gram"]) / (1 + abs(truth["logdet_gram"]))),
        quad=float(abs(quad - truth["quad"]) / (1 + abs(truth["quad"]))))
