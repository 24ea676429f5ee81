# -*- coding: utf-8 -*-
"""Leave-one-out on batched plans, the parts that need no GPU: the exported symbols, the methods' signatures on both plan
classes, and ``batch.leave_one_out_from`` -- the identities

    y_n - mu_-n = alpha_n / c_n ,  sigma^2_-n = 1 / c_n ,  log p(y_n | y_-n) = -1/2 log(2 pi / c_n) - 1/2 alpha_n^2 / c_n

with ``c = diag(K^-1)`` and ``alpha = K^-1 r`` from the oracle -- against brute-force deletion of every sample from the
dense kernel matrix.

Bars (N = 130): variance 1e-11 relative, residual 1e-13 sigma, logpdf 1e-11 relative; measured 3e-13, 2e-15 and 1.5e-13 --
the bars are the measured values rounded up by one to two decades for another BLAS."""
import inspect

import numpy as np
import pytest

import __graft_entry__
from celerite_amd import batch
from oracle import ref
from _cases import NO_GENERAL, synthetic, coeffs_of, within

SYMBOLS = ["clr_batch_leave_one_out", "clr_batch_get_leave_one_out_ms", "clr_sharded_leave_one_out"]


def test_the_new_symbols_are_declared_and_exported():
    declared = __graft_entry__.declared_symbols()
    lib = batch._load()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("cls", [batch.BatchedGP, batch.ShardedBatchedGP])
def test_the_methods_are_on_both_plan_classes(cls):
    assert list(inspect.signature(cls.inverse_diagonal).parameters) == ["self"]
    sig = inspect.signature(cls.leave_one_out)
    assert list(sig.parameters) == ["self", "arrays"] and sig.parameters["arrays"].default is True
    assert batch.LeaveOneOut._fields == ("residual", "variance", "logpdf", "kinv_diag", "alpha", "status")


def dense_kernel(case, p):
    """K_p = k_p(|t_i - t_j|) + diag by the six-coefficient formula (terms.py: RealTerm / ComplexTerm get_value)."""
    ar, cr, ac, bc, cc, dc = coeffs_of(case, p)
    t = case["t"][p]
    tau = np.abs(t[:, None] - t[None, :])[..., None]
    K = np.sum(ar * np.exp(-cr * tau), axis=-1) + np.sum(np.exp(-cc * tau) * (ac * np.cos(dc * tau) + bc * np.sin(dc * tau)), axis=-1)
    return K + np.diag(case["diag"][p])


def by_deletion(K, r):
    """(y_n - mu_-n, sigma^2_-n) of every sample: the conditional of sample n on all the others, one dense solve each."""
    N = len(r)
    res, var = np.empty(N), np.empty(N)
    for n in range(N):
        keep = np.arange(N) != n
        sol = np.linalg.solve(K[np.ix_(keep, keep)], np.stack([r[keep], K[keep, n]], axis=1))
        res[n] = r[n] - K[n, keep] @ sol[:, 0]
        var[n] = K[n, n] - K[n, keep] @ sol[:, 1]
    return res, var


@pytest.mark.parametrize("family", ["bench", "accuracy"])
@pytest.mark.parametrize("JR,JC", [(1, 1), (2, 3), (4, 4)])
def test_leave_one_out_from_against_brute_force_deletion(JR, JC, family):
    N = 130
    case = synthetic(2, N, JR, JC, family, seed=60 + JR + 5 * JC)
    for p in range(2):
        s = ref.RefSolver()
        s.compute(0.0, *coeffs_of(case, p), *NO_GENERAL, case["t"][p], case["diag"][p])
        r = case["y"][p] - 0.3
        c = np.diag(s.solve(np.eye(N))).copy()
        alpha = np.asarray(s.solve(r)).reshape(N)
        residual, variance, logpdf = batch.leave_one_out_from(c, alpha)
        res0, var0 = by_deletion(dense_kernel(case, p), r)
        logpdf0 = float(np.sum(-0.5 * np.log(2.0 * np.pi * var0) - 0.5 * res0 ** 2 / var0))
        tag = "leave_one_out_from vs deletion (%d, %d), %s family" % (JR, JC, family)
        within(tag + ": variance, relative", np.max(np.abs(variance - var0) / var0), 1e-11, p)
        within(tag + ": residual, of sigma", np.max(np.abs(residual - res0) / np.sqrt(var0)), 1e-13, p)
        within(tag + ": logpdf, relative", abs(logpdf - logpdf0) / abs(logpdf0), 1e-11, p)


def test_leave_one_out_from_shapes_and_summation_order():
    """(N,) and (B, N) inputs give the same bits per problem; the sum is the device's: 256 strided partial sums in order,
    then the tree -- restated here with plain loops; N = 700 is no multiple of 256."""
    rng = np.random.RandomState(5)
    c = rng.uniform(0.5, 30.0, (3, 700))
    a = rng.randn(3, 700)
    res, var, lp = batch.leave_one_out_from(c, a)
    assert res.shape == var.shape == (3, 700) and lp.shape == (3,)
    assert np.array_equal(res, a / c) and np.array_equal(var, 1.0 / c)
    for p in range(3):
        r1, v1, l1 = batch.leave_one_out_from(c[p], a[p])
        assert np.array_equal(r1, res[p]) and np.array_equal(v1, var[p]) and l1 == lp[p]
        terms = -0.5 * np.log(6.283185307179586 / c[p]) - 0.5 * a[p] * a[p] / c[p]
        part = [0.0] * 256
        for n in range(700):
            part[n % 256] = part[n % 256] + terms[n]
        w = 128
        while w:
            for i in range(w):
                part[i] = part[i] + part[i + w]
            w //= 2
        assert part[0] == lp[p]
    with pytest.raises(ValueError):
        batch.leave_one_out_from(c, a[:2])
