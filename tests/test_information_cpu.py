# -*- coding: utf-8 -*-
"""The information matrix's references against each other, its expectation property, and the host-side chain
(no GPU).  The bars here are the REFERENCES' yardstick (tests/_information_ref.py), not the device's:
dense against recurrence measured <= 7e-14 of sqrt(I_ii I_jj) at these shapes, the expectation within 1.5 %."""
import os
import re

import numpy as np
import pytest

from celerite_amd import batch

import _information_ref as iref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 1, 0), (2, 0, 1), (63, 0, 1), (64, 2, 3), (65, 1, 0), (130, 2, 3), (130, 0, 4), (130, 8, 0)]


@pytest.mark.parametrize("N,JR,JC", SHAPES)
@pytest.mark.parametrize("mean", [False, True])
def test_dense_against_recurrence(N, JR, JC, mean):
    c = iref.case(N, JR, JC, 10 + N + JR)
    Id = iref.dense_information(*c, mean=mean)
    Is = iref.seq_info(*c, mean=mean)
    dev = iref.scaled_dev(Id, Is)
    print("N %d JR %d JC %d mean %d: dense vs recurrence %.2e" % (N, JR, JC, mean, dev))
    assert dev < 1e-12
    assert np.array_equal(Id, Id.T)


def test_expectation_is_the_fisher_information():
    t, diag, y, ar, cr, ac, bc, cc, dc, jit = iref.case(60, 1, 1, 5)
    K, dK = iref.kernel_and_partials(t, diag, ar, cr, ac, bc, cc, dc, jit)
    Ki = np.linalg.inv(K)
    F = np.array([[0.5 * np.trace(Ki @ A @ Ki @ B) for B in dK] for A in dK])
    G = np.linalg.cholesky(K)
    rng = np.random.default_rng(3)
    acc, draws = 0.0, 4000
    for _ in range(draws):
        acc = acc + iref.dense_info(K, dK, G @ rng.standard_normal(60))
    acc /= draws
    dev = iref.scaled_dev(acc, F)
    print("mean over %d draws against 1/2 tr(K^-1 K_i K^-1 K_j): %.4f" % (draws, dev))
    assert dev < 0.05


def test_padded_tail_adds_nothing():
    # the plan's padding rule (t held, diag = 1e300, y = 0) against the truncated series
    t, diag, y, ar, cr, ac, bc, cc, dc, jit = iref.case(130, 2, 3, 77)
    nb = 71
    tp, dp, yp = t.copy(), diag.copy(), y.copy()
    tp[nb:], dp[nb:], yp[nb:] = t[nb - 1], 1e300, 0.0
    Ia = iref.seq_info(t[:nb], diag[:nb], y[:nb], ar, cr, ac, bc, cc, dc, jit, mean=True)
    Ib = iref.seq_info(tp, dp, yp, ar, cr, ac, bc, cc, dc, jit, mean=True)
    assert iref.scaled_dev(Ib, Ia) < 1e-13


@pytest.mark.parametrize("mean", [False, True])
def test_chain_information_against_loop(mean):
    rng = np.random.default_rng(11)
    B, P, JR, JC = 3, 4, 1, 2
    NC = 2 * JR + 4 * JC
    M = 1 + NC + (1 if mean else 0)
    R = rng.standard_normal((B, M, 2 * M))
    info = R @ R.transpose(0, 2, 1)
    jac, jj = rng.standard_normal((B, P, NC)), rng.standard_normal((B, P))
    got = batch.chain_information(info, jac, jj, mean_partial=mean)
    Q = P + (1 if mean else 0)
    assert got.shape == (B, Q, Q)
    for b in range(B):
        for p in range(Q):
            for q in range(Q):
                def row(k):
                    v = np.zeros(M)
                    if k < P:
                        v[0] = jj[b, k]
                        v[1:1 + NC] = jac[b, k]
                    else:
                        v[-1] = 1.0
                    return v
                want = sum(row(p)[i] * info[b, i, j] * row(q)[j] for i in range(M) for j in range(M))
                assert abs(got[b, p, q] - want) <= 1e-12 * (1.0 + abs(want))
    if mean:                                               # the mean passes through
        assert np.allclose(got[:, -1, -1], info[:, -1, -1], rtol=1e-15, atol=0.0)


def test_chain_information_refuses_wrong_shapes():
    info, jac, jj = np.zeros((2, 7, 7)), np.zeros((2, 3, 6)), np.zeros((2, 3))
    batch.chain_information(info, jac, jj)
    for bad in ((np.zeros((2, 8, 8)), jac, jj, False), (info, jac, jj, True), (info, np.zeros((3, 3, 6)), np.zeros((3, 3)), False),
                (info, jac, np.zeros((2, 4)), False), (np.zeros((2, 7, 6)), jac, jj, False)):
        with pytest.raises(ValueError, match="dimension mismatch"):
            batch.chain_information(bad[0], bad[1], bad[2], mean_partial=bad[3])


def test_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "celerite_hip.h")).read()
    names = ("clr_batch_information", "clr_sharded_information", "clr_batch_set_information_tile",
             "clr_sharded_set_information_tile")
    lib = batch._load()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
    for cls in (batch.BatchedGP, batch.ShardedBatchedGP):
        for name in ("information", "set_information_tile", "information_parameters"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
