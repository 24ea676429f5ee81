# -*- coding: utf-8 -*-
"""Component separation on batched plans (``predict_terms``; ``clr_batch_predict_terms``), the parts that need no GPU: the
masked recurrences of csrc/clr_bterms_kernels.h restated in NumPy (tests/_predict_terms_recurrence.py, no product code)
against dense algebra, ``CompiledKernel.groups``, the argument checks and the exported symbols.

Dense reference: ``k_g*^T K^-1 r`` and ``k_g(0) - k_g*^T K^-1 k_g*`` with ``k_g`` from ``oracle.dense.kernel_value`` on the
coefficients with the amplitudes outside the group zeroed, ``K`` from ``oracle.dense.dense_matrix``.  Bar: 1e-12 k(0) of
the full kernel (for the mean: times max|alpha| N, the size of the sum).  Measured (N = 40, 2 real + 2 complex terms, five
groups, nine points): the variance 2.7e-15 k(0), the mean 1.0e-15 of the bar's scale."""
import inspect
import types

import numpy as np
import pytest

import __graft_entry__
from celerite_amd import batch, terms
from oracle import dense
from _cases import NO_GENERAL, within
from _predict_terms_recurrence import predict_terms_by_recurrence

SYMBOLS = ["clr_batch_predict_terms", "clr_sharded_predict_terms"]
PLAN_CLASSES = [batch.BatchedGP, batch.ShardedBatchedGP]


def test_the_new_symbols_are_declared_and_exported():
    declared = __graft_entry__.declared_symbols()
    lib = batch._load()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("cls", PLAN_CLASSES)
def test_the_signature_is_on_both_plan_classes(cls):
    sig = inspect.signature(cls.predict_terms)
    assert list(sig.parameters) == ["self", "xs", "groups", "return_var"]
    assert sig.parameters["groups"].default is None and sig.parameters["return_var"].default is False


@pytest.mark.parametrize("cls", PLAN_CLASSES)
def test_argument_errors_come_before_the_library_is_touched(cls):
    """On a stub that is no plan (no handle: anything past the checks fails otherwise).  T = 2 + 1 = 3 terms."""
    stub = types.SimpleNamespace(B=3, N=10, J_real=2, J_comp=1)
    xs = np.zeros(5)
    for bad in (np.zeros((2, 5)), np.zeros((3, 5, 1))):
        with pytest.raises(ValueError, match="dimension mismatch"):
            cls.predict_terms(stub, bad)
    with pytest.raises(ValueError, match="out of range"):
        cls.predict_terms(stub, xs, groups=[[0], [3]])
    with pytest.raises(ValueError, match="out of range"):
        cls.predict_terms(stub, xs, groups=[[-1]])
    with pytest.raises(ValueError, match="repeated"):
        cls.predict_terms(stub, xs, groups=[[0, 1, 0]])
    with pytest.raises(ValueError, match="groups is empty"):
        cls.predict_terms(stub, xs, groups=[])
    with pytest.raises(ValueError, match="integers"):
        cls.predict_terms(stub, xs, groups=[[0.5]])
    with pytest.raises(ValueError, match="integers"):
        cls.predict_terms(stub, xs, groups=[[True, False, True]])
    with pytest.raises(ValueError, match="sequence of sequences"):
        cls.predict_terms(stub, xs, groups=[0, 1])
    for bad in (np.zeros((2, 4), dtype=bool), np.zeros(3, dtype=bool), np.zeros((0, 3), dtype=bool), np.zeros((1, 2, 3), dtype=bool)):
        with pytest.raises(ValueError, match="boolean array"):
            cls.predict_terms(stub, xs, groups=bad)
    for ok in (None, [[0], [1, 2], []], np.ones((2, 3), dtype=bool), ((0, 1, 2),)):              # (accepted: no plan)
        with pytest.raises(Exception) as err:
            cls.predict_terms(stub, xs, groups=ok, return_var=True)
        assert not isinstance(err.value, ValueError)


def test_groups_become_one_byte_per_term():
    assert np.array_equal(batch._term_groups(None, 3), np.eye(3, dtype=np.uint8))
    m = batch._term_groups([[2, 0], [], (1,)], 3)
    assert m.dtype == np.uint8 and m.flags["C_CONTIGUOUS"]
    assert np.array_equal(m, [[1, 0, 1], [0, 0, 0], [0, 1, 0]])
    b = np.array([[True, False, True], [False, False, False]])
    assert np.array_equal(batch._term_groups(b, 3), b.astype(np.uint8))


def test_compiled_kernel_groups():
    """One tuple of coefficient-term indices per top-level summand: real ids as they are, complex ids after J_real."""
    real = terms.RealTerm(log_a=0.1, log_c=-0.3)
    over = terms.SHOTerm(log_S0=0.1, log_Q=np.log(0.2), log_omega0=0.5)           # Q < 1/2: two real terms
    under = terms.SHOTerm(log_S0=0.1, log_Q=np.log(3.0), log_omega0=0.5)          # one complex term
    prod = terms.RealTerm(log_a=-0.2, log_c=0.1) * terms.ComplexTerm(log_a=0.3, log_c=-0.1, log_d=0.7)
    jit = terms.JitterTerm(log_sigma=-2.0)
    nested = terms.RealTerm(log_a=0.0, log_c=0.4) + terms.ComplexTerm(log_a=-0.4, log_c=0.2, log_d=1.1)
    kernel = real + over + under + prod + jit + nested                            # (sums flatten: seven summands)
    prog = batch.compile_kernel(kernel)
    assert (prog.J_real, prog.J_comp) == (4, 3)
    # reals: real 0, over 1 2, nested's real 3; complex: under 0, prod 1, nested's 2 -> 4, 5, 6
    assert prog.groups == ((0,), (1, 2), (4,), (5,), (), (3,), (6,))
    flat = sorted(k for g in prog.groups for k in g)
    assert flat == list(range(prog.J_real + prog.J_comp))
    # the groups index kernel.coefficients: a summand's own coefficients are the rows its group names
    a_all = np.concatenate([kernel.coefficients[0], kernel.coefficients[2]])
    for sub, g in zip(kernel.terms, prog.groups):
        c = sub.coefficients
        assert np.array_equal(np.sort(np.concatenate([c[0], c[2]])), np.sort(a_all[list(g)]))
    # no sum: one group; a product of sums: all the terms it expands to; a lone jitter term: the empty group
    assert batch.compile_kernel(under).groups == ((0,),)
    assert batch.compile_kernel(over).groups == ((0, 1),)
    two = (terms.RealTerm(log_a=0.1, log_c=0.2) + terms.ComplexTerm(log_a=0.1, log_c=0.2, log_d=0.3)) * nested
    p2 = batch.compile_kernel(two)
    assert p2.groups == (tuple(range(p2.J_real + p2.J_comp)),) and (p2.J_real, p2.J_comp) == (1, 4)
    assert batch.compile_kernel(jit).groups == ((),)
    assert batch.compile_kernel(prod + real).groups == ((1,), (0,))
    assert batch._term_groups(prog.groups, 7).shape == (7, 7)


def test_the_masked_recurrences_against_dense_algebra():
    rng = np.random.RandomState(7)
    N = 40
    t = np.sort(rng.uniform(0.0, 10.0, N))
    diag = rng.uniform(0.05, 0.2, N) ** 2
    r = np.sin(1.3 * t) + 0.1 * rng.randn(N)
    coeffs = (np.array([1.2, 0.4]), np.array([0.3, 1.1]), np.array([0.8, 0.3]), np.array([0.1, -0.05]),
              np.array([0.2, 0.6]), np.array([1.7, 4.1]))
    T = 4
    groups = np.zeros((5, T), dtype=bool)
    groups[0, 0] = True                 # a single real term
    groups[1, 2] = True                 # a single complex term
    groups[2, [1, 3]] = True            # a mixed pair
    groups[3, :] = True                 # all
    #      4: empty
    xs = np.array([t[0] - 1.5, t[0], t[17], 0.5 * (t[17] + t[18]), 0.3 * t[5] + 0.7 * t[6], t[N - 1], t[N - 1] + 0.7,
                   t[0] - 1e-9, t[N - 1] + 30.0])
    mean, var = predict_terms_by_recurrence(coeffs, t, diag, r, xs, groups)
    K = dense.dense_matrix(0.0, *coeffs, *NO_GENERAL, t, diag)
    alpha = np.linalg.solve(K, r)
    k0 = float(np.sum(coeffs[0]) + np.sum(coeffs[2]))
    mean_scale = k0 * np.max(np.abs(alpha)) * N
    for q, g in enumerate(groups):
        ar = np.where(g[:2], coeffs[0], 0.0)
        ac, bc = np.where(g[2:], coeffs[2], 0.0), np.where(g[2:], coeffs[3], 0.0)
        masked = (ar, coeffs[1], ac, bc, coeffs[4], coeffs[5])
        ks = dense.kernel_value(*masked, xs[:, None] - t[None, :])                 # (M, N)
        kg0 = float(dense.kernel_value(*masked, 0.0))
        m0 = ks @ alpha
        v0 = kg0 - np.sum(ks * np.linalg.solve(K, ks.T).T, axis=1)
        within("predict_terms recurrence, mean / (k(0) max|alpha| N)", np.max(np.abs(mean[q] - m0)) / mean_scale, 1e-12, q)
        within("predict_terms recurrence, var / k(0)", np.max(np.abs(var[q] - v0)) / k0, 1e-12, q)
    assert np.all(mean[4] == 0.0) and np.all(var[4] == 0.0)
    # the variance of a group is not the sum of its terms': the reason groups are an input
    singles = np.eye(T, dtype=bool)
    _, vs = predict_terms_by_recurrence(coeffs, t, diag, r, xs, singles)
    assert np.max(np.abs(vs.sum(axis=0) - var[3])) > 1e-3 * k0
    ms, _ = predict_terms_by_recurrence(coeffs, t, diag, r, xs, singles)
    assert np.max(np.abs(ms.sum(axis=0) - mean[3])) <= 1e-12 * mean_scale
