# -*- coding: utf-8 -*-
"""The per-sample amplitude model of batched plans, the part that needs no GPU: the entries are declared and exported, the
basis and amplitude arguments are checked before the library is called, and the statement of the model

    K_y = S K S + D ,  S = diag(s) ,  s = sum_k a_k Gamma_k
    loglike(K_y, r) = loglike'(K + diag(d / s^2), r / s) - sum_n log|s_n|
    d loglike / d a_k = sum_n Gamma_k[n] (alpha'_n y'_n + d'_n (c'_n - alpha'_n^2) - 1) / s_n

(alpha' = K'^-1 y', c' = diag(K'^-1)) is held against a dense evaluation of ``S K S + D`` in 40 digits.

The last test is where the bar of tests/test_gpu_batch_amplitude.py on the gradient -- 1e-10 S_k with
S_k = sum_n |Gamma_k[n]| (|alpha'_n y'_n| + d'_n (c'_n + alpha'_n^2) + 1) / |s_n| -- is shown to be met by the
double-precision oracle alone with a margin of 100, on the GPU tests' families and bases: c' and alpha' from ``RefSolver``
(as the GPU tests obtain them) against the dense 1/2 alpha^T dK alpha - 1/2 tr(K^-1 dK) of ``S K S + D`` from a 40-digit
inverse at N = 48.  Measured: 7.3e-15 S_k at worst for grad_amplitudes (13000 times inside the bar), 1.1e-14 / 4.1e-14 of
their scales for the amplitude-aware mean / noise gradients."""
import numpy as np
import pytest

import __graft_entry__ as entry
from celerite_amd import batch
from oracle import dense
from _cases import NO_GENERAL, synthetic, coeffs_of, within
from _noise_cases import noise_basis, noise_weights, host_diag, oracle_c_alpha
from _amplitude_cases import (S_MIN, amplitude_gradient, amplitudes, band_basis, host_scale, host_series, log_sum,
                              mean_gradient_scaled, noise_gradient_scaled, smooth_basis)

NEW_SYMBOLS = ["clr_batch_set_amplitude_basis", "clr_batch_set_amplitudes", "clr_batch_get_log_amplitude_sum",
               "clr_batch_grad_amplitudes", "clr_batch_get_amplitude_project_ms", "clr_sharded_set_amplitude_basis",
               "clr_sharded_set_amplitudes", "clr_sharded_get_log_amplitude_sum", "clr_sharded_grad_amplitudes"]


def test_the_new_entries_are_declared_and_exported():
    declared = entry.declared_symbols()
    lib = batch._load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert "CLR_MAX_AMPLITUDE_BASIS 16" in open(entry.ROOT + "/include/celerite_hip.h").read()


@pytest.mark.parametrize("cls", [batch.BatchedGP, batch.ShardedBatchedGP])
def test_the_methods_and_the_constant_are_on_both_plan_classes(cls):
    for name in ("set_amplitude_basis", "set_amplitudes", "log_amplitude_sum", "grad_amplitudes", "amplitude_project_ms"):
        assert callable(getattr(cls, name)), name
    assert batch.MAX_AMPLITUDE_BASIS == 16
    assert "(alpha'_n y'_n + d'_n (c'_n - alpha'_n^2) - 1) / s_n" in cls.grad_amplitudes.__doc__
    assert "materialising run" in cls.grad_amplitudes.__doc__
    assert "s[b, n] = sum_k a[b, k] Gamma_k[b, n]" in cls.set_amplitude_basis.__doc__
    assert "LATENT" in cls.set_amplitudes.__doc__


def test_amplitude_basis_arg_shapes_limit_finiteness_and_lengths():
    B, N, K = 5, 40, 3
    rng = np.random.RandomState(0)
    shared, per = rng.randn(K, N), rng.randn(B, K, N)
    a, stride, k = batch._amplitude_basis_arg(shared, B, N)
    assert (stride, k) == (0, K) and a.flags.c_contiguous and np.array_equal(a, shared)
    a, stride, k = batch._amplitude_basis_arg(per, B, N)
    assert (stride, k) == (K * N, K) and np.array_equal(a, per)
    assert batch._amplitude_basis_arg(None, B, N) == (None, 0, 0)
    assert batch._amplitude_basis_arg(rng.randn(16, N), B, N)[2] == batch.MAX_AMPLITUDE_BASIS
    for shape in [(N,), (B, K, N + 1), (B + 1, K, N), (17, N), (B, 17, N), (K, N + 1), (0, N)]:
        with pytest.raises(ValueError, match="dimension mismatch"):
            batch._amplitude_basis_arg(np.zeros(shape), B, N)
    for bad in (np.nan, np.inf, -np.inf):
        for arr, at in ((shared, (1, 17)), (per, (4, 2, 39))):
            x = arr.copy()
            x[at] = bad
            with pytest.raises(ValueError, match="non-finite amplitude basis"):
                batch._amplitude_basis_arg(x, B, N)
    # per-problem lengths in force: the rest of a row is never looked at and may hold anything
    lens = np.array([40, 1, 17, 39, 25])
    x = per.copy()
    for b, n in enumerate(lens):
        x[b, :, n:] = np.nan
    assert batch._amplitude_basis_arg(x, B, N, lens)[2] == K
    x[2, 1, 16] = np.nan                                  # the last sample of problem 2
    with pytest.raises(ValueError, match="non-finite"):
        batch._amplitude_basis_arg(x, B, N, lens)
    x = shared.copy()
    x[0, 39] = np.inf                                     # a shared basis: checked up to the longest problem
    with pytest.raises(ValueError, match="non-finite"):
        batch._amplitude_basis_arg(x, B, N, lens)
    assert batch._amplitude_basis_arg(x, B, N, np.minimum(lens, 39))[2] == K


@pytest.mark.parametrize("cls", [batch.BatchedGP, batch.ShardedBatchedGP])
def test_the_front_end_refuses_before_the_library(cls):
    """No plan exists (there is no device): every check comes before anything touches the handle."""
    plan = object.__new__(cls)
    plan.B, plan.N, plan.J_real, plan.J_comp = 3, 10, 1, 0
    with pytest.raises(ValueError, match="no amplitude basis"):
        plan.set_amplitudes(np.ones((3, 2)))
    with pytest.raises(RuntimeError, match="set_amplitude_basis"):
        plan.grad_amplitudes()
    with pytest.raises(ValueError, match="dimension mismatch"):
        plan.set_amplitude_basis(np.zeros((17, 10)))
    with pytest.raises(ValueError, match="non-finite"):
        plan.set_amplitude_basis(np.full((2, 10), np.nan))
    plan._amplitude_K = 2
    with pytest.raises(ValueError, match="non-finite amplitude"):
        plan.set_amplitudes(np.array([1.0, np.nan]))
    with pytest.raises(ValueError, match="dimension mismatch"):
        plan.set_amplitudes(np.ones((3, 3)))


def test_the_generators_keep_the_scale_away_from_zero():
    B, N = 4, 130
    for K in (1, 3, 16):
        for per in (False, True):
            for G in (band_basis(B, N, K, per, seed=K), smooth_basis(B, N, K, per, seed=K)):
                a = amplitudes(B, K, seed=K)
                s = host_scale(a, G)
                assert np.abs(s).min() >= S_MIN and (s[0] > 0).all() and (s[1] < 0).all()
                assert (np.abs(a) >= 0.5).all() and (np.abs(a) <= 2.0).all()
    G = band_basis(B, N, 3, True, seed=1)
    assert set(np.unique(G)) == {0.0, 1.0} and (G.sum(axis=1) == 1.0).all() and (G.sum(axis=2) > 0).all()
    G = smooth_basis(B, N, 3, True, seed=1)
    assert (G >= 0).all() and (G.sum(axis=1) >= 0.5).all() and len(np.unique(G)) > N


# ---- the statement against the dense S K S + D in 40 digits ---------------------------------------------------------

def _mp_setup(case, p, s, D, r, dps=40):
    """``(mp, Ky, Kinv, alpha)`` of the data-unit matrix ``S K S + D`` of problem ``p``: K's entries are the fp64 kernel
    values, the scaling, the inverse and the solve run in ``dps`` digits."""
    import mpmath as mp

    mp.mp.dps = dps
    N = len(s)
    K0 = dense.dense_matrix(0.0, *coeffs_of(case, p), *NO_GENERAL, case["t"][p], np.zeros(N))
    Ky = mp.matrix(N, N)
    for i in range(N):
        for j in range(N):
            Ky[i, j] = mp.mpf(float(s[i])) * mp.mpf(float(K0[i, j])) * mp.mpf(float(s[j]))
        Ky[i, i] += mp.mpf(float(D[i]))
    Kinv = mp.inverse(Ky)
    alpha = Kinv * mp.matrix([mp.mpf(float(v)) for v in r])
    return mp, K0, Ky, Kinv, alpha


def _mp_loglike(mp, Ky, alpha, r):
    N = len(r)
    quad = mp.fsum(mp.mpf(float(r[i])) * alpha[i] for i in range(N))
    return -(quad + mp.log(mp.det(Ky)) + N * mp.log(2 * mp.pi)) / 2


CASES = [(1, 0, "bench"), (2, 1, "accuracy"), (2, 3, "bench"), (1, 10, "bench")]


@pytest.mark.parametrize("JR,JC,family", CASES)
def test_the_log_likelihood_identity_against_the_dense_matrix_in_40_digits(JR, JC, family):
    """``loglike(S K S + D, r) = loglike(K + diag(D / s^2), r / s) - sum log|s|``, both sides factorised in 40 digits
    (``mp_logdet_quad``): the right side on the HOST-FORMED series ``r / s`` and ``D / (s * s)`` in double with ``log_sum``'s
    L, so what remains is rounding in double of the right side's inputs: the quotients, L, and -- the largest -- the
    diagonal ``k(0) + d'_n`` of ``dense_matrix``, rounded to 1e-16 absolute where d' is 1e-2 .. 1e-1: it moves the quadratic
    form by sum_n alpha'_n^2 1e-16 with alpha' up to 1 / d', some 1e-11 absolute on a loglike of order 1e2.  Nothing here
    runs through LAPACK, so the figure does not depend on the machine.  Bar 1e-12 of |loglike| (measured: 2.1e-13)."""
    B, N, K = 3, 48, 3
    case = synthetic(B, N, JR, JC, family, seed=200 + JR + JC)
    for G in (band_basis(B, N, K, True, seed=1), smooth_basis(B, N, K, False, seed=2)):
        a = amplitudes(B, K, seed=JR)
        s = host_scale(a, G)
        assert np.abs(s).min() >= S_MIN
        yp, dp = host_series(case["y"], case["diag"], s)
        L, _ = log_sum(s)
        for p in range(B):
            Kp = dense.dense_matrix(0.0, *coeffs_of(case, p), *NO_GENERAL, case["t"][p], dp[p])
            ld, quad = dense.mp_logdet_quad(Kp, yp[p])
            got = -0.5 * (quad + ld + N * np.log(2 * np.pi)) - L[p]
            mp, _, Ky, _, alpha = _mp_setup(case, p, s[p], case["diag"][p], case["y"][p])
            want = _mp_loglike(mp, Ky, alpha, case["y"][p])
            within("amplitude model: loglike' - L vs the dense S K S + D in 40 digits", abs(float(mp.mpf(got) - want) / float(want)),
                   1e-12, (JR, JC, family, p))


@pytest.mark.parametrize("JR,JC,family", CASES)
def test_the_double_oracle_meets_the_three_gradient_bars_with_a_margin_of_100(JR, JC, family):
    """The GPU tests hold ``grad_amplitudes()`` -- and ``grad_mean_weights()`` / ``grad_noise_weights()`` with amplitudes in
    force -- to 1e-10 of their scales against sums over the double oracle's c' and alpha'.  Here those references against
    the dense truth of ``K_y = S K S + D`` from a 40-digit inverse, with a linear mean and a noise model in force and a
    non-indicator basis: d K_y / d a_k = G_k K S + S K G_k (G_k = diag(Gamma_k)), d K_y / d s_k = diag(Psi_k), d r / d w_k =
    -Phi_k, each in 1/2 alpha^T dK alpha - 1/2 tr(K_y^-1 dK) or Phi_k^T alpha.  Within 1e-12 of the scale (bar / 100); the
    largest deviations are printed."""
    B, N, K = 2, 48, 3
    case = synthetic(B, N, JR, JC, family, seed=300 + JR + JC)
    Phi = np.stack([np.ones(N), np.linspace(-1.0, 1.0, N)])
    w = np.random.RandomState(5).uniform(-0.5, 0.5, (B, 2))
    resid = case["y"] - (w[:, 0, None] * Phi[0] + w[:, 1, None] * Phi[1])
    Psi = noise_basis(case["diag"], K, True, seed=2)
    D = host_diag(case["diag"], noise_weights(B, K, seed=2), Psi)
    for G in (band_basis(B, N, K, False, seed=3), smooth_basis(B, N, K, True, seed=4)):
        a = amplitudes(B, K, seed=JC)
        s = host_scale(a, G)
        assert np.abs(s).min() >= S_MIN
        yp, dp = host_series(resid, D, s)
        Gb = np.broadcast_to(G, (B, K, N))
        for p in range(B):
            c, al = oracle_c_alpha(case, p, dp[p], yp[p])
            ga, Sa = amplitude_gradient(Gb[p], al, c, yp[p], dp[p], s[p])
            gm, Sm = mean_gradient_scaled(Phi, al, s[p])
            gn, Sn = noise_gradient_scaled(Psi[p], al, c, s[p])
            mp, K0, Ky, Kinv, alpha = _mp_setup(case, p, s[p], D[p], resid[p])
            # u = K S alpha and the diagonal of K S Kinv, for d K_y / d a_k = G_k K S + S K G_k
            Sal = [mp.mpf(float(s[p, n])) * alpha[n] for n in range(N)]
            KS_al = [mp.fsum(mp.mpf(float(K0[n, m])) * Sal[m] for m in range(N)) for n in range(N)]
            KS_Kinv_diag = [mp.fsum(mp.mpf(float(K0[n, m])) * mp.mpf(float(s[p, m])) * Kinv[m, n] for m in range(N)) for n in range(N)]
            for k in range(K):
                want = mp.fsum(mp.mpf(float(Gb[p, k, n])) * (alpha[n] * KS_al[n] - KS_Kinv_diag[n]) for n in range(N))
                within("double oracle's amplitude gradient vs the 40-digit dense truth / S_k (bar / 100)",
                       abs(float(mp.mpf(float(ga[k])) - want)) / Sa[k], 1e-12, (JR, JC, family, p, k))
                want = mp.fsum(mp.mpf(float(Psi[p, k, n])) * (alpha[n] * alpha[n] - Kinv[n, n]) for n in range(N)) / 2
                within("double oracle's noise gradient with amplitudes vs the 40-digit dense truth / scale (bar / 100)",
                       abs(float(mp.mpf(float(gn[k])) - want)) / Sn[k], 1e-12, (JR, JC, family, p, k))
            for k in range(2):
                want = mp.fsum(mp.mpf(float(Phi[k, n])) * alpha[n] for n in range(N))
                within("double oracle's mean gradient with amplitudes vs the 40-digit dense truth / scale (bar / 100)",
                       abs(float(mp.mpf(float(gm[k])) - want)) / Sm[k], 1e-12, (JR, JC, family, p, k))


def test_one_amplitude_for_all_samples_against_a_central_difference():
    """K = 1, Gamma = 1: d loglike / d a by central differences of the dense log-likelihood of ``a^2 K + D``.  A step
    h = 1e-4 on a ~ 1 leaves a truncation error ~ h^2 and a rounding error ~ 1e-16 |loglike| / h ~ 1e-10; bar 1e-6 S_0."""
    N = 40
    case = synthetic(2, N, 2, 1, "accuracy", seed=9)
    G = np.ones((1, N))
    h = 1e-4

    def loglike(p, a):
        s = host_scale(np.array([[a]]), G)[0]
        K0 = dense.dense_matrix(0.0, *coeffs_of(case, p), *NO_GENERAL, case["t"][p], np.zeros(N))
        return dense.dense_log_likelihood(s[:, None] * K0 * s[None, :] + np.diag(case["diag"][p]), case["y"][p])[0]

    for p, a0 in enumerate((1.3, -0.7)):
        s = host_scale(np.array([[a0]]), G)[0]
        yp, dp = host_series(case["y"][p], case["diag"][p], s)
        c, al = oracle_c_alpha(case, p, dp, yp)
        g, S = amplitude_gradient(G, al, c, yp, dp, s)
        fd = (loglike(p, a0 + h) - loglike(p, a0 - h)) / (2 * h)
        within("amplitude gradient, K = 1, Gamma = 1, vs a central difference of the dense log-likelihood / S_0",
               abs(g[0] - fd) / S[0], 1e-6, p)
