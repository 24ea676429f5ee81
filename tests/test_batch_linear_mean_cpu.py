# -*- coding: utf-8 -*-
"""The linear mean model of batched plans, the part that needs no GPU: the entries are declared and exported, the
basis / weights arguments are checked before the library is called, and a constant and a linear mean in one call are
refused."""
import numpy as np
import pytest

import __graft_entry__ as entry
from celerite_amd import batch

NEW_SYMBOLS = ["clr_batch_set_mean_basis", "clr_batch_set_mean_weights", "clr_batch_grad_mean_weights",
               "clr_batch_get_mean_project_ms", "clr_sharded_set_mean_basis", "clr_sharded_set_mean_weights",
               "clr_sharded_grad_mean_weights"]


def test_the_new_entries_are_declared_and_exported():
    declared = entry.declared_symbols()
    lib = batch._load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name


def test_basis_arg_shapes_and_strides():
    B, N, K = 5, 40, 3
    rng = np.random.RandomState(0)
    shared = rng.randn(K, N)
    a, stride, k = batch._basis_arg(shared, B, N)
    assert (stride, k) == (0, K) and a.flags.c_contiguous and a.dtype == np.float64 and np.array_equal(a, shared)
    per = rng.randn(B, K, N)
    a, stride, k = batch._basis_arg(per, B, N)
    assert (stride, k) == (K * N, K) and np.array_equal(a, per)
    # a transposed view is made contiguous, a list is converted
    a, stride, k = batch._basis_arg(np.asfortranarray(shared), B, N)
    assert a.flags.c_contiguous and np.array_equal(a, shared)
    assert batch._basis_arg([[1.0] * N], B, N)[1:] == (0, 1)
    assert batch._basis_arg(None, B, N) == (None, 0, 0)
    assert batch._basis_arg(rng.randn(16, N), B, N)[2] == 16


@pytest.mark.parametrize("shape", ["(N,)", "(B, K, N + 1)", "(B + 1, K, N)", "(17, N)", "(B, 17, N)", "(K, N + 1)", "(0, N)"])
def test_basis_arg_refuses_bad_shapes(shape):
    B, N, K = 5, 40, 3
    with pytest.raises(ValueError, match="dimension mismatch"):
        batch._basis_arg(np.zeros(eval(shape)), B, N)


def test_weights_arg_broadcasts_one_row():
    B, K = 4, 3
    w = np.arange(3.0)
    a = batch._weights_arg(w, B, K)
    assert a.shape == (B, K) and a.flags.c_contiguous and (a == w).all()
    full = np.arange(12.0).reshape(B, K)
    assert np.array_equal(batch._weights_arg(full, B, K), full)
    for bad in (np.zeros(4), np.zeros((B, K + 1)), np.zeros((B + 1, K)), 1.0):
        with pytest.raises(ValueError, match="dimension mismatch"):
            batch._weights_arg(bad, B, K)
    with pytest.raises(ValueError, match="dimension mismatch"):      # no basis set: K = 0
        batch._weights_arg(np.zeros(0), B, 0)


@pytest.mark.parametrize("cls", [batch.BatchedGP, batch.ShardedBatchedGP])
def test_a_constant_and_a_linear_mean_in_one_call_are_refused_before_the_library(cls):
    """No plan exists (there is no device): the check comes before anything touches the handle."""
    plan = object.__new__(cls)
    plan.B, plan.N, plan.J_real, plan.J_comp = 3, 10, 1, 0
    tabs = [np.ones((3, 1)), np.ones((3, 1))] + [np.empty((3, 0))] * 4
    with pytest.raises(ValueError, match="mutually exclusive"):
        plan.evaluate(*tabs, mean=0.5, mean_weights=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="mutually exclusive"):
        plan.evaluate_parameters(np.zeros((3, 2)), mean=np.zeros(3), mean_weights=np.zeros(2))


def test_predict_needs_the_basis_at_the_prediction_points():
    plan = object.__new__(batch.BatchedGP)
    plan.B, plan.N, plan._mean_K = 2, 10, 2
    plan._mean_w = np.array([[1.0, 2.0], [3.0, -1.0]])
    with pytest.raises(ValueError, match="mean_basis"):
        batch._linear_mean_at(plan, None, 4)
    basis = np.array([[1.0, 1.0, 1.0, 1.0], [0.0, 0.5, 1.0, 1.5]])
    m = batch._linear_mean_at(plan, basis, 4)
    assert np.array_equal(m, plan._mean_w[:, 0, None] * basis[0] + plan._mean_w[:, 1, None] * basis[1])
    with pytest.raises(ValueError, match="dimension mismatch"):
        batch._linear_mean_at(plan, basis[:1], 4)
    plan._mean_K = 0
    assert batch._linear_mean_at(plan, None, 4) is None
