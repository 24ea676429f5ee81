# -*- coding: utf-8 -*-
"""The joint posterior at sorted points (csrc/clr_bcond_kernels.h) in plain NumPy, for one problem: its own factorisation,
no product code.  Slot n holds ``phi[n]`` (the decay n -> n+1), ``u[n] = u(t_n)``, ``W[n]``, ``D[n]``; ``u(x)``, ``v(x)``
are the feature rows at a point, ``c`` the rows' decay rates, ``m_j = #{n : t_n <= x_j}`` (``m`` below)::

    S+_n = S_n + D_n W_n W_n^T ,  S_{n+1} = Phi_n S+_n Phi_n ,  S_0 = 0
    Q_n  = u_n u_n^T / D_n + F_n^T Q_{n+1} F_n ,  Q_N = 0 ,  F_n = Phi_n (I - W_n u_n^T)
    e_j  = v(x_j) - psi o (S+_{m-1} (psi o u(x_j))) ,  psi = exp(-c (x_j - t_{m-1}))          (m = 0: v(x_j))
    r_j  = u(x_j) - psi' o (Q_m (psi' o e_j)) ,       psi' = exp(-c (t_m - x_j))              (m = N: u(x_j))
    T_j  = decay to x_{j+1} . prod_{n = m_j}^{m_{j+1} - 1} (I - W_n u_n^T) decay to t_n       (x_j -> x_{j+1})
    C_ij = r_j^T T_{j-1} ... T_i e_i   (i <= j) ,   C_jj = r_j^T e_j
    C + reg I = L diag(d) L^T ,  L_ji = r_j^T T_{j-1} ... T_i omega_i :
        d_j = r_j^T e_j + reg - r_j^T G_j r_j ,  omega_j = (e_j - G_j r_j) / d_j ,  G_{j+1} = T_j (G_j + d_j omega_j omega_j^T) T_j^T
    a draw: z_j = sqrt(d_j) n_j ,  f_j = z_j + r_j^T gamma_j ,  gamma_{j+1} = T_j (gamma_j + omega_j z_j)
"""
import numpy as np

from _predict_terms_recurrence import features

NOT_POSITIVE_DEFINITE = 1


def generators(coeffs, t, diag, xs):
    """(e[M, J], r[M, J], T[M - 1, J, J], k0) at the ascending points ``xs``."""
    ar, cr, ac, bc, cc, dc = [np.asarray(v, dtype=float) for v in coeffs]
    coeffs = (ar, cr, ac, bc, cc, dc)
    J, N, M = len(ar) + 2 * len(ac), len(t), len(xs)
    assert np.all(np.diff(xs) >= 0)
    c = np.concatenate([cr, np.repeat(cc, 2)])
    k0 = float(np.sum(ar) + np.sum(ac))
    u, v = np.empty((N, J)), np.empty((N, J))
    for n in range(N):
        u[n], v[n] = features(coeffs, t[n])
    phi = np.exp(-c[None, :] * np.diff(t)[:, None])
    W, D, Sp = np.empty((N, J)), np.empty(N), np.empty((N, J, J))
    S = np.zeros((J, J))
    for n in range(N):
        Su = S @ u[n]
        D[n] = k0 + diag[n] - u[n] @ Su
        W[n] = (v[n] - Su) / D[n]
        Sp[n] = S + D[n] * np.outer(W[n], W[n])
        if n + 1 < N:
            S = np.outer(phi[n], phi[n]) * Sp[n]
    Q = np.zeros((N + 1, J, J))
    Q[N - 1] = np.outer(u[N - 1], u[N - 1]) / D[N - 1]
    for n in range(N - 2, -1, -1):
        F = phi[n][:, None] * (np.eye(J) - np.outer(W[n], u[n]))
        Q[n] = np.outer(u[n], u[n]) / D[n] + F.T @ Q[n + 1] @ F
    ms = np.searchsorted(t, xs, side="right")
    e, r = np.empty((M, J)), np.empty((M, J))
    for j, x in enumerate(xs):
        m = int(ms[j])
        ux, vx = features(coeffs, x)
        e[j], r[j] = vx, ux
        if m > 0:
            psi = np.exp(-c * (x - t[m - 1]))
            e[j] = vx - psi * (Sp[m - 1] @ (psi * ux))
        if m < N:
            psip = np.exp(-c * (t[m] - x))
            r[j] = ux - psip * (Q[m] @ (psip * e[j]))
    T = np.empty((max(M - 1, 0), J, J))
    for j in range(M - 1):
        A, at = np.eye(J), xs[j]
        for n in range(int(ms[j]), int(ms[j + 1])):
            A = np.exp(-c * (t[n] - at))[:, None] * A
            A = A - np.outer(W[n], u[n] @ A)
            at = t[n]
        T[j] = np.exp(-c * (xs[j + 1] - at))[:, None] * A
    return e, r, T, k0


def covariance(e, r, T):
    """C[M, M] by the pair formula: for source i walk h <- T_{j-1} h from e_i."""
    M = len(e)
    C = np.empty((M, M))
    for i in range(M):
        h = e[i].copy()
        C[i, i] = r[i] @ h
        for j in range(i + 1, M):
            h = T[j - 1] @ h
            C[i, j] = C[j, i] = r[j] @ h
    return C


def factor(e, r, T, k0, regularize=0.0, min_pivot=1e-10):
    """(d[M], omega[M, J], status): the pivots (0 where the point is a function of the earlier ones) and the generators of
    L; status NOT_POSITIVE_DEFINITE where a pivot is below -min_pivot k(0) or not finite."""
    M, J = e.shape
    d, om = np.zeros(M), np.zeros((M, J))
    G = np.zeros((J, J))
    for j in range(M):
        Gr = G @ r[j]
        dj = r[j] @ e[j] + regularize - r[j] @ Gr
        if not np.isfinite(dj) or dj < -min_pivot * k0:
            return d, om, NOT_POSITIVE_DEFINITE
        if abs(dj) > min_pivot * k0:
            d[j] = dj
            om[j] = (e[j] - Gr) / dj
        if j + 1 < M:
            G = T[j] @ (G + d[j] * np.outer(om[j], om[j])) @ T[j].T
    return d, om, 0


def draw(r, T, d, om, normals):
    """f[size, M] = L diag(d)^1/2 n for ``normals[size, M]``."""
    normals = np.atleast_2d(normals)
    size, M = normals.shape
    out = np.empty((size, M))
    for s in range(size):
        g = np.zeros(r.shape[1])
        for j in range(M):
            z = np.sqrt(d[j]) * normals[s, j]
            out[s, j] = z + r[j] @ g
            if j + 1 < M:
                g = T[j] @ (g + om[j] * z)
    return out


def dense_covariance(coeffs, t, diag, xs):
    """k(x, x') - k*^T K^-1 k*' from the dense matrices."""
    ar, cr, ac, bc, cc, dc = [np.asarray(v, dtype=float) for v in coeffs]

    def k(tau):
        tau = np.abs(np.asarray(tau, dtype=float))[..., None]
        return np.sum(ar * np.exp(-cr * tau), axis=-1) + np.sum(np.exp(-cc * tau) * (ac * np.cos(dc * tau) + bc * np.sin(dc * tau)), axis=-1)

    K = k(t[:, None] - t[None, :]) + np.diag(diag)
    ks = k(t[:, None] - xs[None, :])
    return k(xs[:, None] - xs[None, :]) - ks.T @ np.linalg.solve(K, ks)
