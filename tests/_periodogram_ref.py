# -*- coding: utf-8 -*-
"""The dense NumPy reference of ``BatchedGP.periodogram``: ``K`` from the six coefficient arrays plus ``diag + jitter``, the
bordered Gram matrix of the columns ``(cos, sin)`` / ``(1, cos, sin)`` and a residual by ``np.linalg.solve``, and ``power``,
``coef``, ``cov`` by ``np.linalg.solve`` on the unscaled ``G``.  O(N^3): series of a thousand samples."""
import collections

import numpy as np

DenseFit = collections.namedtuple("DenseFit", ["gram", "power", "coef", "cov", "kappa"])


def dense_K(coeffs, t, diag, jitter=0.0):
    """``K[i, j] = k(|t_i - t_j|) + (diag_i + jitter) delta_ij`` of one problem (terms.py: RealTerm / ComplexTerm)."""
    ar, cr, ac, bc, cc, dc = [np.asarray(v, dtype=float) for v in coeffs]
    tau = np.abs(t[:, None] - t[None, :])[..., None]
    K = np.sum(ar * np.exp(-cr * tau), axis=-1)
    K = K + np.sum(np.exp(-cc * tau) * (ac * np.cos(dc * tau) + bc * np.sin(dc * tau)), axis=-1)
    return K + np.diag(np.asarray(diag, dtype=float) + jitter)


def columns(t, omega, t_ref, offset):
    """``X[N, K]``: ``np.cos(omega * (t - t_ref))``, ``np.sin(...)``, behind a column of ones with the offset."""
    arg = omega * (t - t_ref)
    cols = [np.cos(arg), np.sin(arg)]
    if offset:
        cols.insert(0, np.ones(len(t)))
    return np.stack(cols, axis=1)


def fit_from_gram(S, offset):
    """power, coef, cov and the condition number of the unit-diagonal ``G`` from one bordered matrix."""
    K = S.shape[0] - 1
    G, d = S[:K, :K], S[:K, K]
    coef = np.linalg.solve(G, d)
    cov = np.linalg.solve(G, np.eye(K))
    power = 0.5 * (d @ coef)
    if offset:
        power = power - 0.5 * d[0] * d[0] / G[0, 0]
    s = 1.0 / np.sqrt(np.diag(G))
    return power, coef, cov, np.linalg.cond(G * s[:, None] * s[None, :])


def dense_grams(K, t, r, omega, t_ref=0.0):
    """The bordered matrices of the columns ``(1, cos, sin)`` and ``r`` at every frequency, ``[F, 4, 4]``, from ONE
    ``np.linalg.solve`` with all columns; the matrices without the offset are ``[:, 1:, 1:]``."""
    omega = np.atleast_1d(np.asarray(omega, dtype=float))
    F = len(omega)
    X = np.concatenate([columns(t, w, t_ref, False) for w in omega] + [np.ones((len(t), 1)), r[:, None]], axis=1)
    KX = np.linalg.solve(K, X)
    A = X.T @ KX
    A = 0.5 * (A + A.T)
    gram = np.empty((F, 4, 4))
    for f in range(F):
        idx = [2 * F, 2 * f, 2 * f + 1, 2 * F + 1]
        gram[f] = A[np.ix_(idx, idx)]
    return gram


def fit_from_grams(gram, offset):
    """A :class:`DenseFit` from ``dense_grams``' matrices."""
    g = gram if offset else gram[:, 1:, 1:]
    fits = [fit_from_gram(S, offset) for S in g]
    return DenseFit(g.copy(), np.array([f[0] for f in fits]), np.stack([f[1] for f in fits]), np.stack([f[2] for f in fits]),
                    np.array([f[3] for f in fits]))


def dense_periodogram(K, t, r, omega, t_ref=0.0, offset=False):
    """A :class:`DenseFit` of one problem at the frequencies ``omega[F]``: ``gram[F, K + 1, K + 1]``, ``power[F]``,
    ``coef[F, K]``, ``cov[F, K, K]``, ``kappa[F]``."""
    return fit_from_grams(dense_grams(K, t, r, omega, t_ref), offset)


def scan_frequencies(t, F=7):
    """``F`` frequencies between ``4 pi / T`` and ``pi / median(dt)``, geometrically spaced (irrational ratios: no
    frequency sits on a multiple of another)."""
    T = t[-1] - t[0]
    return np.geomspace(4.0 * np.pi / T, np.pi / np.median(np.diff(t)), F)
