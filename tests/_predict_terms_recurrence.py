# -*- coding: utf-8 -*-
"""The masked recurrences of component separation (csrc/clr_bterms_kernels.h) in plain NumPy, for one problem: its own
factorisation, its own solve, no product code.  Slot n holds ``phi[n]`` (the decay n -> n+1), ``u[n] = u(t_n)``, ``W[n]``,
``D[n]``; ``u(x)``, ``v(x)`` are the feature rows at a point, ``c`` the rows' decay rates, ``m = #{n : t_n <= x}``::

    S+_n = S_n + D_n W_n W_n^T ,  S_{n+1} = Phi_n S+_n Phi_n ,  S_0 = 0
    Q_n  = u_n u_n^T / D_n + F_n^T Q_{n+1} F_n ,  Q_N = 0 ,  F_n = Phi_n (I - W_n u_n^T)   (F_{N-1} = 0)
    p+_n = phi_{n-1} o p+_{n-1} + v(t_n) alpha_n ,   b_n = phi_n o b_{n+1} + u_n alpha_n ,  b_N = 0
    w = psi o u_g(x) ,  mean_g = w^T p+_{m-1} + (psi' o v_g(x))^T b_m
    left = w^T S+_{m-1} w ,  e = v_g(x) - psi o (S+_{m-1} w) ,  e' = psi' o e ,  var_g = k_g(0) - left - e'^T Q_m e'
"""
import numpy as np


def features(coeffs, x):
    """(u(x), v(x)): real rows (a, 1), complex pairs (a cos + b sin, a sin - b cos), (cos, sin) at the absolute phase."""
    ar, cr, ac, bc, cc, dc = coeffs
    cd, sd = np.cos(dc * x), np.sin(dc * x)
    u = np.concatenate([ar, np.stack([ac * cd + bc * sd, ac * sd - bc * cd], axis=1).reshape(-1)])
    v = np.concatenate([np.ones(len(ar)), np.stack([cd, sd], axis=1).reshape(-1)])
    return u, v


def row_masks(groups, JR, JC):
    """(G, T) 0/1 over the coefficient terms -> (G, J) over the rows: a complex term owns its cos and its sin row."""
    groups = np.asarray(groups, dtype=bool)
    return np.concatenate([groups[:, :JR], np.repeat(groups[:, JR:], 2, axis=1)], axis=1)


def predict_terms_by_recurrence(coeffs, t, diag, r, xs, groups):
    """(mean[G, M], var[G, M]) of the groups' processes at ``xs`` given the residual ``r`` at ``t``."""
    ar, cr, ac, bc, cc, dc = [np.asarray(v, dtype=float) for v in coeffs]
    coeffs = (ar, cr, ac, bc, cc, dc)
    JR, JC = len(ar), len(ac)
    J, N = JR + 2 * JC, len(t)
    c = np.concatenate([cr, np.repeat(cc, 2)])
    amp = np.concatenate([ar, ac])
    masks = row_masks(groups, JR, JC)
    k0 = float(np.sum(ar) + np.sum(ac))
    u = np.empty((N, J))
    v = np.empty((N, J))
    for n in range(N):
        u[n], v[n] = features(coeffs, t[n])
    phi = np.exp(-c[None, :] * np.diff(t)[:, None])                   # phi[n]: n -> n + 1
    # the factorisation and its forward state
    W, D, Sp = np.empty((N, J)), np.empty(N), np.empty((N, J, J))
    S = np.zeros((J, J))
    for n in range(N):
        Su = S @ u[n]
        D[n] = k0 + diag[n] - u[n] @ Su
        W[n] = (v[n] - Su) / D[n]
        Sp[n] = S + D[n] * np.outer(W[n], W[n])
        if n + 1 < N:
            S = np.outer(phi[n], phi[n]) * Sp[n]
    # alpha = K^-1 r
    z, g = np.empty(N), np.zeros(J)
    for n in range(N):
        z[n] = r[n] - u[n] @ g
        if n + 1 < N:
            g = phi[n] * (g + W[n] * z[n])
    alpha, k = z / D, np.zeros(J)
    for n in range(N - 2, -1, -1):
        k = phi[n] * (k + u[n + 1] * alpha[n + 1])
        alpha[n] -= W[n] @ k
    # Q_n, n = 0 .. N (Q_N = 0); p+_n; b_n, n = 0 .. N (b_N = 0)
    Q = np.zeros((N + 1, J, J))
    Q[N - 1] = np.outer(u[N - 1], u[N - 1]) / D[N - 1]
    for n in range(N - 2, -1, -1):
        F = phi[n][:, None] * (np.eye(J) - np.outer(W[n], u[n]))
        Q[n] = np.outer(u[n], u[n]) / D[n] + F.T @ Q[n + 1] @ F
    pp = np.empty((N, J))
    pp[0] = v[0] * alpha[0]
    for n in range(1, N):
        pp[n] = phi[n - 1] * pp[n - 1] + v[n] * alpha[n]
    bb = np.zeros((N + 1, J))
    bb[N - 1] = u[N - 1] * alpha[N - 1]
    for n in range(N - 2, -1, -1):
        bb[n] = phi[n] * bb[n + 1] + u[n] * alpha[n]
    # the points
    G, M = len(masks), len(xs)
    mean, var = np.empty((G, M)), np.empty((G, M))
    for i, x in enumerate(xs):
        m = int(np.searchsorted(t, x, side="right"))                  # samples with t_n <= x
        ux, vx = features(coeffs, x)
        psi = np.exp(-c * (x - t[m - 1])) if m > 0 else np.zeros(J)
        psip = np.exp(-c * (t[m] - x)) if m < N else np.zeros(J)
        for q, mask in enumerate(masks):
            ug, vg = np.where(mask, ux, 0.0), np.where(mask, vx, 0.0)
            kg0 = float(np.sum(amp[np.asarray(groups[q], dtype=bool)]))
            w = psi * ug
            mu, left, e = 0.0, 0.0, vg
            if m > 0:
                mu += w @ pp[m - 1]
                Sw = Sp[m - 1] @ w
                left = w @ Sw
                e = vg - psi * Sw
            quad = 0.0
            if m < N:
                mu += (psip * vg) @ bb[m]
                ep = psip * e
                quad = ep @ Q[m] @ ep
            mean[q, i] = mu
            var[q, i] = kg0 - left - quad
    return mean, var
