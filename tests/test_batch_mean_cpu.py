# -*- coding: utf-8 -*-
"""The constant mean of the batched path on the host side: chain_gradient's mean column, the mean's argument checks,
and the ABI entries the header declares."""
import numpy as np
import pytest

from celerite_amd import batch, terms


def test_chain_gradient_appends_the_mean_partial_last():
    """chain_gradient(grad, jac, jitter_jac, dmean): the kernel's parameters as before, then d loglike / d mu as the
    last column -- the order of GP(kernel, mean=c, fit_mean=True).get_parameter_vector() (celerite.py:224-227)."""
    from celerite_amd import GP

    k = terms.RealTerm(0.1, 0.5) + terms.ComplexTerm(0.6, 0.7, 1.0) + terms.JitterTerm(log_sigma=-1.0)
    rng = np.random.RandomState(7)
    draws = k.get_parameter_vector()[None, :] + 0.1 * rng.randn(5, 6)
    jac, jit_jac = batch.kernel_coefficient_jacobian_table(k, draws)
    w = rng.randn(5, 7)
    dmean = rng.randn(5)
    g0 = batch.chain_gradient(w, jac, jit_jac)
    g = batch.chain_gradient(w, jac, jit_jac, dmean)
    assert g.shape == (5, 7)
    assert np.array_equal(g[:, :6], g0) and np.array_equal(g[:, 6], dmean)
    gp = GP(k, mean=0.3, fit_mean=True)
    assert len(gp.get_parameter_vector()) == g.shape[1] and gp.get_parameter_names()[-1].endswith("value")
    with pytest.raises(ValueError):
        batch.chain_gradient(w, jac, jit_jac, dmean[:3])


def test_mean_argument_forms():
    """A scalar is one value for every problem (stride 0), (B,) one per problem (stride 1), None no mean; any other
    shape is refused before the library is called."""
    m, s = batch._mean_arg(0.5, 4)
    assert s == 0 and m.shape == (1,) and m[0] == 0.5
    m, s = batch._mean_arg(np.arange(4.0), 4)
    assert s == 1 and m.shape == (4,)
    assert batch._mean_arg(None, 4) == (None, 0)
    for bad in (np.zeros(3), np.zeros((4, 1)), np.zeros((2, 2))):
        with pytest.raises(ValueError):
            batch._mean_arg(bad, 4)


def test_mean_entry_points_are_declared_and_exported():
    import __graft_entry__ as entry

    names = entry.declared_symbols()
    lib = batch._load()
    for s in ("clr_batch_set_mean", "clr_batch_evaluate_mean", "clr_batch_grad_mean", "clr_sharded_set_mean",
              "clr_sharded_evaluate_mean", "clr_sharded_grad_mean"):
        assert s in names and hasattr(lib, s), s
