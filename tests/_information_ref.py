# -*- coding: utf-8 -*-
"""References for the information matrix of the innovations form (``BatchedGP.information``), NumPy only.

With ``z = L^-1 r`` the one-step-ahead innovations and ``D`` their variances, for two directions i, j

    I[i][j] = sum_n 1/2 (d_i D_n / D_n)(d_j D_n / D_n) + (d_i z_n)(d_j z_n) / D_n .

``dense_info``  from the Cholesky factor ``K = G G^T`` and the analytic ``d K / d coefficient``: with ``A_i = G^-1 d_i K
                G^-T`` and ``e = G^-1 r``:  ``d_i D_n / D_n = (A_i)_nn`` and ``d_i z_n / sqrt D_n = -(Phi(A_i) e)_n + 1/2 e_n
                (A_i)_nn``, ``Phi`` the lower triangle with the diagonal halved.  O(N^3) per direction.
``seq_info``    the sequential recurrence with one tangent per direction, the arithmetic of the device's forward mode.
Directions in the order of the batched gradient's columns -- jitter, a_real, c_real, a_comp, b_comp, c_comp, d_comp --
then the constant mean (``d D = 0``, ``d r = -1``).
"""
import numpy as np

try:
    from scipy.linalg import solve_triangular as _solve_triangular
except ImportError:                                        # (NumPy alone: a general solve of the triangular system)
    _solve_triangular = None


def solve_lower(G, b):
    """``G^-1 b`` for a lower-triangular ``G``."""
    if _solve_triangular is not None:
        return _solve_triangular(G, b, lower=True)
    return np.linalg.solve(G, b)


def kernel_and_partials(t, diag, ar, cr, ac, bc, cc, dc, jit):
    """``K`` and the list of ``d K / d direction`` in the gradient's order."""
    t = np.asarray(t, dtype=np.float64)
    tau = np.abs(t[:, None] - t[None, :])
    N = len(t)
    K = np.diag(np.asarray(diag, dtype=np.float64) + jit)
    d_ar, d_cr, d_ac, d_bc, d_cc, d_dc = [], [], [], [], [], []
    for a, c in zip(ar, cr):
        e = np.exp(-c * tau)
        K = K + a * e
        d_ar.append(e)
        d_cr.append(-a * tau * e)
    for a, b, c, d in zip(ac, bc, cc, dc):
        e, co, si = np.exp(-c * tau), np.cos(d * tau), np.sin(d * tau)
        K = K + e * (a * co + b * si)
        d_ac.append(e * co)
        d_bc.append(e * si)
        d_cc.append(-tau * e * (a * co + b * si))
        d_dc.append(tau * e * (-a * si + b * co))
    return K, [np.eye(N)] + d_ar + d_cr + d_ac + d_bc + d_cc + d_dc


def dense_info(K, dK, r, mean=False):
    N = len(r)
    G = np.linalg.cholesky(K)
    e = solve_lower(G, r)
    rows = []
    for Mx in dK:
        A = solve_lower(G, solve_lower(G, Mx).T).T
        d = np.diag(A).copy()
        Phi = np.tril(A, -1) + np.diag(0.5 * d)
        rows.append(np.concatenate([d / np.sqrt(2.0), -Phi @ e + 0.5 * e * d]))
    if mean:
        rows.append(np.concatenate([np.zeros(N), -solve_lower(G, np.ones(N))]))
    R = np.array(rows)
    return R @ R.T


def dense_information(t, diag, y, ar, cr, ac, bc, cc, dc, jit, mean=False):
    K, dK = kernel_and_partials(t, diag, ar, cr, ac, bc, cc, dc, jit)
    return dense_info(K, dK, np.asarray(y, dtype=np.float64), mean)


def seq_info(t, diag, y, ar, cr, ac, bc, cc, dc, jit, mean=False):
    JR, JC = len(ar), len(ac)
    J, N = JR + 2 * JC, len(t)
    NG = 1 + 2 * JR + 4 * JC + (1 if mean else 0)
    o = 1 + 2 * JR

    def feats(n):
        u, v, phi = np.zeros(J), np.zeros(J), np.zeros(J)
        du, dv, dphi = np.zeros((NG, J)), np.zeros((NG, J)), np.zeros((NG, J))
        dx = t[n + 1] - t[n] if n + 1 < N else 0.0
        tn = t[n]
        for j in range(JR):
            u[j], v[j], phi[j] = ar[j], 1.0, np.exp(-cr[j] * dx)
            du[1 + j, j] = 1.0
            dphi[1 + JR + j, j] = -dx * phi[j]
        for k in range(JC):
            a, b, c, d = ac[k], bc[k], cc[k], dc[k]
            cs, sn = np.cos(d * tn), np.sin(d * tn)
            i0, i1 = JR + 2 * k, JR + 2 * k + 1
            u[i0], u[i1] = a * cs + b * sn, a * sn - b * cs
            v[i0], v[i1] = cs, sn
            p = np.exp(-c * dx)
            phi[i0] = phi[i1] = p
            du[o + k, i0], du[o + k, i1] = cs, sn
            du[o + JC + k, i0], du[o + JC + k, i1] = sn, -cs
            dphi[o + 2 * JC + k, i0] = dphi[o + 2 * JC + k, i1] = -dx * p
            du[o + 3 * JC + k, i0], du[o + 3 * JC + k, i1] = tn * (-a * sn + b * cs), tn * (a * cs + b * sn)
            dv[o + 3 * JC + k, i0], dv[o + 3 * JC + k, i1] = -tn * sn, tn * cs
        return u, v, phi, du, dv, dphi

    S, f = np.zeros((J, J)), np.zeros(J)
    dS, df = np.zeros((NG, J, J)), np.zeros((NG, J))
    da = np.zeros(NG)
    da[0] = 1.0
    da[1:1 + JR] = 1.0
    da[o:o + JC] = 1.0
    info = np.zeros((NG, NG))
    k0 = float(np.sum(ar)) + float(np.sum(ac))
    for n in range(N):
        u, v, phi, du, dv, dphi = feats(n)
        q = S @ u
        D = diag[n] + jit + k0 - u @ q
        x = y[n] - u @ f
        z = v - q
        w = z / D
        dq = dS @ u + du @ S.T
        dD = da - (du @ q + dq @ u)
        dx = -(du @ f + df @ u)
        if mean:
            dx[NG - 1] -= 1.0
        dz = dv - dq
        dw = (dz - np.outer(dD, w)) / D
        ra, rb = dD / D, dx / np.sqrt(D)
        info += 0.5 * np.outer(ra, ra) + np.outer(rb, rb)
        Sn, g = S + np.outer(z, w), f + w * x
        pp = np.outer(phi, phi)
        dSn = dS + dz[:, :, None] * w[None, None, :] + z[None, :, None] * dw[:, None, :]
        dpp = dphi[:, :, None] * phi[None, None, :] + phi[None, :, None] * dphi[:, None, :]
        dS = dpp * Sn[None] + pp[None] * dSn
        dg = df + dw * x + np.outer(dx, w)
        df = dphi * g[None] + phi[None] * dg
        S, f = pp * Sn, phi * g
    return info


def case(N, JR, JC, seed):
    """One well-conditioned problem: ``(t, diag, y, ar, cr, ac, bc, cc, dc, jit)``; y is drawn from the model plus 0.3."""
    r = np.random.default_rng(seed)
    t = np.sort(r.uniform(0, N * 0.1, N))
    diag = r.uniform(0.01, 0.05, N)
    ar, cr = r.uniform(0.5, 2, JR), r.uniform(0.05, 2, JR)
    ac, cc, dc = r.uniform(0.5, 2, JC), r.uniform(0.05, 1, JC), r.uniform(0.5, 6, JC)
    bc = np.minimum(ac * r.uniform(0, 0.3, JC), 0.9 * ac * cc / dc) if JC else ac.copy()
    jit = 0.02
    K, _ = kernel_and_partials(t, diag, ar, cr, ac, bc, cc, dc, jit)
    y = np.linalg.cholesky(K) @ r.standard_normal(N) + 0.3
    return t, diag, y, ar, cr, ac, bc, cc, dc, jit


def scaled_dev(a, ref):
    """max |a - ref| / sqrt(ref_ii ref_jj)"""
    d = np.sqrt(np.abs(np.diag(ref)))
    sc = np.outer(d, d) + 1e-300
    return float(np.max(np.abs(a - ref) / sc))
