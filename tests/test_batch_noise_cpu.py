# -*- coding: utf-8 -*-
"""The linear noise model of batched plans, the part that needs no GPU: the entries are declared and exported, the basis
and weights arguments are checked before the library is called, and the model

    diag_eff = diag + sum_k s_k Psi_k ,   d loglike / d s_k = 1/2 sum_n Psi_k[n] (alpha_n^2 - c_n)

(alpha = K^-1 r, c = diag(K^-1)) is stated in NumPy and held against the dense oracle (oracle/dense.py).

The last test is where the bar of tests/test_gpu_batch_noise.py on the gradient -- 1e-10 S_k with
S_k = 1/2 sum_n |Psi_k[n]| (alpha_n^2 + c_n) -- is shown to be met by the double-precision oracle alone, with a margin of
100, on the input families the GPU tests use: c and alpha from ``RefSolver`` (as the GPU tests obtain them) against a
40-digit inverse of the same dense matrix at N = 48.  Measured: 5.5e-14 S_k at worst over the 96 partials, 1800 times
inside the bar."""
import inspect

import numpy as np
import pytest

import __graft_entry__ as entry
from celerite_amd import batch
from oracle import dense
from _cases import NO_GENERAL, synthetic, coeffs_of, within
from _noise_cases import host_diag, noise_basis, noise_gradient, noise_weights, oracle_c_alpha

NEW_SYMBOLS = ["clr_batch_set_noise_basis", "clr_batch_set_noise_weights", "clr_batch_grad_noise_weights",
               "clr_batch_get_noise_project_ms", "clr_sharded_set_noise_basis", "clr_sharded_set_noise_weights",
               "clr_sharded_grad_noise_weights"]


def test_the_new_entries_are_declared_and_exported():
    declared = entry.declared_symbols()
    lib = batch._load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("cls", [batch.BatchedGP, batch.ShardedBatchedGP])
def test_the_methods_are_on_both_plan_classes(cls):
    for name in ("set_noise_basis", "set_noise_weights", "grad_noise_weights", "noise_project_ms"):
        assert callable(getattr(cls, name)), name
    for name in ("evaluate", "evaluate_parameters"):
        sig = inspect.signature(getattr(cls, name))
        assert sig.parameters["noise_weights"].default is None and "mean_weights" in sig.parameters
    assert "1/2 sum_n Psi_k[b, n] (alpha_n^2 - c_n)" in cls.grad_noise_weights.__doc__
    assert "materialising run" in cls.grad_noise_weights.__doc__
    assert "diag[b, n] + sum_k s[b, k] Psi_k[b, n]" in cls.set_noise_basis.__doc__


def test_noise_basis_arg_shapes_limit_and_finiteness():
    B, N, K = 5, 40, 3
    rng = np.random.RandomState(0)
    shared, per = rng.randn(K, N), rng.randn(B, K, N)
    a, stride, k = batch._noise_basis_arg(shared, B, N)
    assert (stride, k) == (0, K) and a.flags.c_contiguous and np.array_equal(a, shared)
    a, stride, k = batch._noise_basis_arg(per, B, N)
    assert (stride, k) == (K * N, K) and np.array_equal(a, per)
    assert batch._noise_basis_arg(None, B, N) == (None, 0, 0)
    assert batch._noise_basis_arg(rng.randn(16, N), B, N)[2] == batch.MAX_NOISE_BASIS == 16
    for shape in [(N,), (B, K, N + 1), (B + 1, K, N), (17, N), (B, 17, N), (K, N + 1), (0, N)]:
        with pytest.raises(ValueError, match="dimension mismatch"):
            batch._noise_basis_arg(np.zeros(shape), B, N)
    for bad in (np.nan, np.inf, -np.inf):
        for arr, at in ((shared, (1, 17)), (per, (4, 2, 39))):
            x = arr.copy()
            x[at] = bad
            with pytest.raises(ValueError, match="non-finite"):
                batch._noise_basis_arg(x, B, N)
    # per-problem lengths in force: the rest of a row is never looked at and may hold anything
    lens = np.array([40, 1, 17, 39, 25])
    x = per.copy()
    for b, n in enumerate(lens):
        x[b, :, n:] = np.nan
    assert batch._noise_basis_arg(x, B, N, lens)[2] == K
    x[2, 1, 16] = np.nan                                  # the last sample of problem 2
    with pytest.raises(ValueError, match="non-finite"):
        batch._noise_basis_arg(x, B, N, lens)
    x = shared.copy()
    assert batch._noise_basis_arg(x, B, N, lens)[2] == K  # (a shared basis: checked up to the longest problem)
    x[0, 39] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        batch._noise_basis_arg(x, B, N, lens)
    assert batch._noise_basis_arg(x, B, N, np.minimum(lens, 39))[2] == K


def test_noise_weights_arg():
    B, K = 4, 3
    one = np.arange(3.0)
    a = batch._noise_weights_arg(one, B, K)
    assert a.shape == (B, K) and a.flags.c_contiguous and (a == one).all()
    full = np.arange(12.0).reshape(B, K)
    assert np.array_equal(batch._noise_weights_arg(full, B, K), full)
    for bad in (np.zeros(4), np.zeros((B, K + 1)), np.zeros((B + 1, K)), 1.0):
        with pytest.raises(ValueError, match="dimension mismatch"):
            batch._noise_weights_arg(bad, B, K)
    with pytest.raises(ValueError, match="no noise basis"):          # weights without a basis
        batch._noise_weights_arg(np.zeros(0), B, 0)
    for bad in (np.nan, np.inf):
        x = full.copy()
        x[2, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            batch._noise_weights_arg(x, B, K)


@pytest.mark.parametrize("cls", [batch.BatchedGP, batch.ShardedBatchedGP])
def test_the_front_end_refuses_before_the_library(cls):
    """No plan exists (there is no device): every check comes before anything touches the handle."""
    plan = object.__new__(cls)
    plan.B, plan.N, plan.J_real, plan.J_comp = 3, 10, 1, 0
    with pytest.raises(ValueError, match="no noise basis"):
        plan.set_noise_weights(np.zeros((3, 2)))
    with pytest.raises(RuntimeError, match="set_noise_basis"):
        plan.grad_noise_weights()
    with pytest.raises(ValueError, match="dimension mismatch"):
        plan.set_noise_basis(np.zeros((17, 10)))
    with pytest.raises(ValueError, match="non-finite"):
        plan.set_noise_basis(np.full((2, 10), np.nan))
    tabs = [np.ones((3, 1)), np.ones((3, 1))] + [np.empty((3, 0))] * 4
    with pytest.raises(ValueError, match="no noise basis"):
        plan.evaluate(*tabs, noise_weights=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="no noise basis"):
        plan.evaluate_parameters(np.zeros((3, 2)), noise_weights=np.zeros(2))
    plan._noise_K = 2
    with pytest.raises(ValueError, match="non-finite"):
        plan.set_noise_weights(np.array([0.0, np.nan]))
    with pytest.raises(ValueError, match="dimension mismatch"):
        plan.set_noise_weights(np.zeros((3, 3)))


# ---- the model and its gradient against the dense oracle -----------------------------------------------------------

def _dense_gradient(case, p, d, r, Psi):
    """1/2 sum Psi_k (alpha^2 - c) from a dense inverse of the kernel matrix on the diagonal d."""
    K = dense.dense_matrix(0.0, *coeffs_of(case, p), *NO_GENERAL, case["t"][p], d)
    Kinv = np.linalg.inv(K)
    return noise_gradient(Psi, Kinv @ r, np.diag(Kinv).copy())


@pytest.mark.parametrize("JR,JC", [(1, 0), (2, 1), (2, 3)])
def test_gradient_formula_against_central_differences_of_the_dense_log_likelihood(JR, JC):
    """d loglike / d s_k by central differences of ``dense_log_likelihood`` on ``diag + sum_k s_k Psi_k``: a step h = 1e-4
    on weights of order 0.3 leaves a truncation error ~ h^2 and a rounding error ~ 1e-16 |loglike| / h ~ 1e-10; the bar is
    1e-6 of S_k (measured: 3.4e-10)."""
    B, N, K = 2, 40, 3
    case = synthetic(B, N, JR, JC, "accuracy", seed=5 + JR)
    Psi = noise_basis(case["diag"], K, per=True, seed=1)
    s = noise_weights(B, K, seed=1)
    h = 1e-4
    for p in range(B):
        d = host_diag(case["diag"], s, Psi)[p]
        assert (d > 0).all()
        g, S = _dense_gradient(case, p, d, case["y"][p], Psi[p])
        for k in range(K):
            ll = []
            for sign in (1.0, -1.0):
                sk = s.copy()
                sk[p, k] += sign * h
                Kd = dense.dense_matrix(0.0, *coeffs_of(case, p), *NO_GENERAL, case["t"][p], host_diag(case["diag"], sk, Psi)[p])
                ll.append(dense.dense_log_likelihood(Kd, case["y"][p])[0])
            within("noise gradient formula vs central differences of the dense log-likelihood / S_k",
                   abs(g[k] - (ll[0] - ll[1]) / (2 * h)) / S[k], 1e-6, (JR, JC, p, k))


def test_one_basis_function_of_ones_is_the_jitter_partial():
    """Psi = 1: d K / d s is the identity, the jitter's partial of ``mp_grad_log_likelihood`` (40 digits, dense).  Bar
    1e-12 S_0: the double inverse of a well-conditioned 40 x 40 matrix (measured: below 1e-16)."""
    N = 40
    case = synthetic(1, N, 1, 1, "accuracy", seed=9)
    jitter = 0.3
    _, g0 = dense.mp_grad_log_likelihood(jitter, *coeffs_of(case, 0), *NO_GENERAL, case["t"][0], case["y"][0], case["diag"][0])
    g, S = _dense_gradient(case, 0, case["diag"][0] + jitter, case["y"][0], np.ones((1, N)))
    within("noise gradient, Psi = 1, vs the jitter partial of mp_grad_log_likelihood / S_0", abs(g[0] - g0[0]) / S[0], 1e-12)


def _mp_c_alpha(Kd, r, dps=40):
    import mpmath as mp

    mp.mp.dps = dps
    n = len(r)
    K = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            K[i, j] = mp.mpf(float(Kd[i, j]))
    Kinv = mp.inverse(K)
    alpha = Kinv * mp.matrix([mp.mpf(float(v)) for v in r])
    return [Kinv[i, i] for i in range(n)], [alpha[i] for i in range(n)]


@pytest.mark.parametrize("family", ["bench", "accuracy"])
@pytest.mark.parametrize("JR,JC", [(1, 0), (2, 1), (2, 3), (1, 10)])
def test_the_double_oracle_meets_the_gradient_bar_with_a_margin_of_100(JR, JC, family):
    """The GPU tests hold ``grad_noise_weights()`` to 1e-10 S_k of 1/2 sum Psi_k (alpha0^2 - c0) with c0, alpha0 from the
    double-precision oracle.  That reference itself must sit well inside the bar: here its gradient against the same sum
    from a 40-digit inverse of the dense matrix (its fp64 entries), on the GPU tests' families, bases and weights at
    N = 48: within 1e-12 S_k."""
    import mpmath as mp

    B, N, K = 2, 48, 3
    case = synthetic(B, N, JR, JC, family, seed=300 + JR + JC)
    for per in (False, True):
        Psi = noise_basis(case["diag"], K, per, seed=2)
        s = noise_weights(B, K, seed=2)
        d = host_diag(case["diag"], s, Psi)
        P = np.broadcast_to(Psi, (B, K, N))
        for p in range(B):
            c, a = oracle_c_alpha(case, p, d[p], case["y"][p])
            g, S = noise_gradient(P[p], a, c)
            Kd = dense.dense_matrix(0.0, *coeffs_of(case, p), *NO_GENERAL, case["t"][p], d[p])
            cq, aq = _mp_c_alpha(Kd, case["y"][p])
            for k in range(K):
                gq = mp.fsum(mp.mpf(float(P[p, k, n])) * (aq[n] * aq[n] - cq[n]) for n in range(N)) / 2
                within("double oracle's noise gradient vs the 40-digit dense inverse / S_k (bar / 100)",
                       abs(float(mp.mpf(float(g[k])) - gq)) / S[k], 1e-12, (JR, JC, family, per, p, k))
