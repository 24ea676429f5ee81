# -*- coding: utf-8 -*-
"""The generalised-least-squares fit of a linear mean's weights, the parts that need no GPU: the exported symbols, the
small solve (clr_gram_solve: the routine the device runs per problem) against a long-double Cholesky, the MeanFit
likelihood arithmetic and the Python-side argument checks."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__
from celerite_amd import batch
from _mean_fit import LD, ld_fit, small_solve_bound, small_solve_errors

SYMBOLS = ["clr_batch_fit_mean_weights", "clr_sharded_fit_mean_weights", "clr_gram_solve", "clr_batch_set_mean_fit_tile",
           "clr_batch_get_mean_fit_ms"]


def test_the_new_symbols_are_declared_and_exported():
    declared = __graft_entry__.declared_symbols()
    lib = batch._load()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name


def _spd(rng, K, scales=None):
    """A random bordered Gram matrix [[G, d], [d^T, q]] with G = A^T A / n + I (kappa_2 of the scaled G is a few), then
    rows and columns of G and d scaled by ``scales``; q large enough to keep the bordered matrix positive definite."""
    A = rng.randn(4 * K + 3, K)
    G = A.T @ A / A.shape[0] + np.eye(K)
    d = rng.randn(K)
    if scales is not None:
        G = G * scales[:, None] * scales[None, :]
        d = d * scales
    S = np.empty((K + 1, K + 1))
    S[:K, :K] = 0.5 * (G + G.T)
    S[:K, K] = S[K, :K] = d
    S[K, K] = float(d @ np.linalg.solve(G, d)) * (1.0 + rng.uniform(0.01, 2.0)) + 0.1
    return S


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("K", [1, 2, 5, 16])
def test_gram_solve_against_a_long_double_cholesky(K, scaled):
    """Unit-scaled matrices, and matrices whose rows and columns carry scales over 10^-6 .. 10^6 (the equilibration
    absorbs them: the bound is in kappa_2 of the SCALED matrix), at the first-order forward bound of the solve.  Largest
    deviation seen: 0.78 of the bound (K = 16, scaled: the covariance)."""
    rng = np.random.RandomState(100 + K + 50 * scaled)
    n = 20
    S = np.stack([_spd(rng, K, 10.0 ** rng.uniform(-6, 6, K) if scaled else None) for _ in range(n)])
    w0 = rng.uniform(-1.5, 1.5, (n, K))
    w, cov, quad, ld, st = batch.gram_solve(S, w0)
    assert (st == 0).all()
    worst = 0.0
    for p in range(n):
        truth = ld_fit(S[p], w0[p])
        assert truth["kappa_s"] < 50.0
        bound = small_solve_bound(K, truth["kappa_s"])
        err = small_solve_errors(truth, w[p], cov[p], ld[p], quad[p])
        print(K, scaled, p, "kappa_s %.3g bound %.3g" % (truth["kappa_s"], bound), err)
        for name, e in err.items():
            assert e <= bound, (name, e, bound, p)
            worst = max(worst, e / bound)
        assert np.array_equal(cov[p], cov[p].T)
    print("largest deviation / bound: %.3g" % worst)
    # zero start weights when none are given; a single matrix without the leading axis
    w1, _, q1, _, _ = batch.gram_solve(S[0])
    wz, _, qz, _, _ = batch.gram_solve(S[:1], np.zeros((1, K)))
    assert np.array_equal(w1, wz) and np.array_equal(q1, qz)


def test_gram_solve_profiled_quadratic_form_survives_cancellation():
    """A residual the basis explains to one part in 10^9: q - d^T G^-1 d is 10^-9 q (q of order 1, so that the long-double
    truth is good to 10^-19), and still good to the bound relative to 1 + |value| -- the quadratic form is evaluated
    around its minimum in twice the working precision.  q - d^T delta in float64 would be off by 10^-16 q: one digit."""
    rng = np.random.RandomState(7)
    K = 4
    S = _spd(rng, K)
    x = np.linalg.solve(S[:K, :K], S[:K, K])
    S[K, K] = float(np.sum(S[:K, K].astype(LD) * x.astype(LD))) * (1 + 1e-9)
    truth = ld_fit(S, np.zeros(K))
    _, _, quad, _, st = batch.gram_solve(S)
    assert st[0] == 0 and 0 < float(truth["quad"]) < 1e-8 * S[K, K]
    err = abs(quad[0] - truth["quad"]) / (1 + abs(truth["quad"]))
    print("quad %.6e truth %.6e deviation %.3g" % (quad[0], float(truth["quad"]), err))
    assert err <= small_solve_bound(K, truth["kappa_s"])
    assert abs(quad[0] - truth["quad"]) <= 1e-6 * truth["quad"]      # ... and to six digits of its own size


def test_gram_solve_refusals():
    rng = np.random.RandomState(5)
    K = 5
    good = _spd(rng, K)
    w0 = rng.uniform(-1, 1, (4, K))
    dup = good.copy()                     # row / column 2 a copy of row / column 0: rank deficient
    dup[2, :] = dup[0, :]
    dup[:, 2] = dup[:, 0]
    dup[2, 2] = dup[0, 0]
    zero = good.copy()
    zero[1, 1] = 0.0
    neg = good.copy()
    neg[3, 3] = -good[3, 3]
    S = np.stack([good, dup, zero, neg])
    w, cov, quad, ld, st = batch.gram_solve(S, w0)
    assert st.tolist() == [0, batch.CLR_NOT_POSITIVE_DEFINITE, batch.CLR_NOT_POSITIVE_DEFINITE, batch.CLR_NOT_POSITIVE_DEFINITE]
    assert np.isfinite(w[0]).all() and np.isfinite(cov[0]).all() and np.isfinite(quad[0]) and np.isfinite(ld[0])
    for p in (1, 2, 3):
        assert np.array_equal(w[p], w0[p])
        assert np.isnan(cov[p]).all() and np.isnan(quad[p]) and np.isnan(ld[p])
    # a refused neighbour changes nothing of a problem's bits
    alone = batch.gram_solve(good, w0[0])
    for a, b in zip(alone, (w, cov, quad, ld, st)):
        assert np.array_equal(a[0], b[0])
    # a NaN or infinite diagonal is refused, never factored
    for bad in (np.nan, np.inf):
        m = good.copy()
        m[0, 0] = bad
        assert batch.gram_solve(m)[4][0] == batch.CLR_NOT_POSITIVE_DEFINITE
    # min_pivot is the bar of the scaled pivots: every matrix fails 0.999..., the duplicate passes none
    assert batch.gram_solve(good, min_pivot=0.0)[4][0] == 0
    nearly = good.copy()
    nearly[2, :] = nearly[0, :]
    nearly[:, 2] = nearly[:, 0]
    nearly[2, 2] = nearly[0, 0] * (1 + 1e-6)          # scaled pivot ~ 1e-6
    assert batch.gram_solve(nearly, min_pivot=1e-10)[4][0] == 0
    assert batch.gram_solve(nearly, min_pivot=1e-3)[4][0] == batch.CLR_NOT_POSITIVE_DEFINITE


@pytest.mark.parametrize("bad", [np.nan, np.inf, -1.0, -1e-300, 1.0, 2.0])
def test_min_pivot_is_validated(bad):
    S = _spd(np.random.RandomState(1), 3)
    with pytest.raises(ValueError, match="min_pivot"):
        batch.gram_solve(S, min_pivot=bad)
    lib = batch._load()                   # the library's own check, past the Python layer's
    out = np.empty(3)
    assert lib.clr_gram_solve(1, 3, batch._ptr(S), None, C.c_double(bad), batch._ptr(out), None, None, None,
                              None) == batch.CLR_INVALID_ARGUMENT
    assert lib.clr_gram_solve(1, 0, batch._ptr(S), None, C.c_double(0.0), None, None, None, None,
                              None) == batch.CLR_INVALID_ARGUMENT
    assert lib.clr_gram_solve(1, 17, batch._ptr(S), None, C.c_double(0.0), None, None, None, None,
                              None) == batch.CLR_INVALID_ARGUMENT


def test_mean_fit_likelihood_arithmetic():
    """loglike = -1/2 (quad + log det K + N log 2 pi); loglike_marginal = loglike - 1/2 log det G + 1/2 K log 2 pi."""
    N, K = 10, 2
    quad = np.array([3.0, 8.0, np.nan])
    logdet_K = np.array([1.5, -2.0, 0.25])
    ld_gram = np.array([0.5, 4.0, np.nan])
    w, cov, gram = np.zeros((3, K)), np.zeros((3, K, K)), np.zeros((3, K + 1, K + 1))
    st = np.array([0, 0, 2], dtype=np.int32)
    fit = batch._mean_fit(w, cov, gram, quad, ld_gram, st, logdet_K, N)
    assert isinstance(fit, batch.MeanFit)
    assert fit._fields == ("weights", "covariance", "gram", "quad", "logdet_gram", "loglike", "loglike_marginal", "status")
    l2pi = 1.8378770664093453              # log 2 pi
    assert fit.loglike[0] == pytest.approx(-0.5 * (3.0 + 1.5 + 10 * l2pi), rel=1e-15)
    assert fit.loglike[1] == pytest.approx(-0.5 * (8.0 - 2.0 + 10 * l2pi), rel=1e-15)
    assert fit.loglike_marginal[0] == pytest.approx(fit.loglike[0] - 0.25 + l2pi, rel=1e-15)
    assert fit.loglike_marginal[1] == pytest.approx(fit.loglike[1] - 2.0 + l2pi, rel=1e-15)
    assert np.isnan(fit.loglike[2]) and np.isnan(fit.loglike_marginal[2])
    assert fit.weights is w and fit.status is st and fit.gram is gram


@pytest.mark.parametrize("cls", [batch.BatchedGP, batch.ShardedBatchedGP])
def test_python_side_argument_checks(cls):
    plan = object.__new__(cls)
    plan.B, plan.N, plan._mean_K, plan._mean_w, plan._h = 3, 100, 0, None, None
    with pytest.raises(RuntimeError, match="no basis"):
        plan.fit_mean_weights()
    plan._mean_K = 2
    for bad in (np.nan, -1.0, 1.0):
        with pytest.raises(ValueError, match="min_pivot"):
            plan.fit_mean_weights(min_pivot=bad)
    with pytest.raises(ValueError):
        batch.gram_solve(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError):
        batch.gram_solve(np.zeros((1, 18, 18)))
