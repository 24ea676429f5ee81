# -*- coding: utf-8 -*-
"""One-step-ahead residuals and causal forecasts on batched plans (``one_step_ahead``, ``forecast``;
``clr_batch_one_step_ahead``, ``clr_batch_forecast``), the parts that need no GPU: the exported symbols, the signatures on
both plan classes, the argument checks, the host-side properties of ``OneStepAhead``, and a NumPy restatement of the two
identities the kernels of csrc/clr_bfilter_kernels.h implement, on the oracle's factor.

In slot notation (slot n: ``phi[n]`` the decay n -> n+1, ``u[n] = U~(t_n)``, ``W[n]``, ``D[n]``), with ``u(x)`` the
reference's feature row at a point x, ``c`` the rows' decay rates and ``m = #{n : t_n < x}``::

    z_n = r_n - u[n] . g_n ,  g+_n = g_n + W[n] z_n ,  g_{n+1} = phi[n] o g+_n ,  g_0 = 0
    S+_n = S_n + D_n W_n W_n^T ,  S_{n+1} = Phi_n S+_n Phi_n ,  S_0 = 0
    psi = exp(-c (x - t_{m-1})) ,  w = psi o u(x)
    mean(x) = w^T g+_{m-1} ,  var(x) = k(0) - w^T S+_{m-1} w                 (m = 0: mean 0, var k(0))

held against ``RefSolver`` on the truncated series ``t[:m]`` per point (``predict`` and ``k(0) - k* . solve(k*)``).

Bars: the mean 1e-10 of max|y|, the variance 1e-10 k(0) (the project's PREDICT bar).  Measured (N = 700, 42 points, three
shapes, both families): the mean at most 2.6e-15 of max|y|, the variance 7.6e-15 k(0); sum z^2 / D against the oracle's
``dot_solve`` 1.3e-15 relative, ``L (z / sqrt D)`` back to r within 2.7e-16 of max|r| (those two under 1e-12, the
project's ``dot_L`` bar)."""
import inspect
import types

import numpy as np
import pytest

import __graft_entry__
from celerite_amd import batch
from oracle import ref
from _cases import NO_GENERAL, synthetic, coeffs_of, within

PREDICT = 1e-10
SYMBOLS = ["clr_batch_one_step_ahead", "clr_batch_forecast", "clr_sharded_one_step_ahead", "clr_sharded_forecast"]
PLAN_CLASSES = [batch.BatchedGP, batch.ShardedBatchedGP]


def test_the_new_symbols_are_declared_and_exported():
    declared = __graft_entry__.declared_symbols()
    lib = batch._load()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("cls", PLAN_CLASSES)
def test_the_signatures_are_on_both_plan_classes(cls):
    sig = inspect.signature(cls.one_step_ahead)
    assert list(sig.parameters) == ["self", "b"] and sig.parameters["b"].default is None
    sig = inspect.signature(cls.forecast)
    assert list(sig.parameters) == ["self", "xs", "return_var", "mean_basis"]
    assert sig.parameters["return_var"].default is False and sig.parameters["mean_basis"].default is None


@pytest.mark.parametrize("cls", PLAN_CLASSES)
def test_argument_errors_come_before_the_library_is_touched(cls):
    """On a stub that is no plan (no handle: anything past the checks fails otherwise)."""
    stub = types.SimpleNamespace(B=3, N=10)
    for bad in (np.zeros(10), np.zeros((2, 10)), np.zeros((3, 9)), np.zeros((3, 2, 9)), np.zeros((3, 2, 2, 10))):
        with pytest.raises(ValueError, match="dimension mismatch"):
            cls.one_step_ahead(stub, bad)
    for bad in (np.zeros((2, 5)), np.zeros((3, 5, 1))):
        with pytest.raises(ValueError, match="dimension mismatch"):
            cls.forecast(stub, bad)
    with pytest.raises(ValueError, match="mean_basis without a linear mean"):
        cls.forecast(stub, np.zeros(5), mean_basis=np.zeros((2, 5)))
    linear = types.SimpleNamespace(B=3, N=10, _mean_K=2, _mean_w=np.ones((3, 2)))
    with pytest.raises(ValueError, match="a linear mean is in force"):
        cls.forecast(linear, np.zeros(5), return_var=True)
    with pytest.raises(ValueError, match="dimension mismatch"):
        cls.forecast(linear, np.zeros(5), mean_basis=np.zeros((3, 5)))
    for call in (lambda: cls.one_step_ahead(stub), lambda: cls.forecast(stub, np.zeros(5))):     # (accepted: no plan)
        with pytest.raises(Exception) as err:
            call()
        assert not isinstance(err.value, ValueError)


def test_the_result_type_and_its_host_side_properties():
    rng = np.random.RandomState(0)
    z, D = rng.randn(2, 5), rng.uniform(0.5, 2.0, (2, 5))
    osa = batch.OneStepAhead(z, D, np.zeros(2, dtype=np.int32))
    assert osa._fields == ("innovation", "variance", "status")
    assert np.array_equal(osa.standardized, z / np.sqrt(D))
    assert np.allclose(osa.log_density, -0.5 * (np.log(2 * np.pi * D) + z * z / D), rtol=1e-15, atol=0)
    z3 = rng.randn(2, 3, 5)
    osa3 = batch.OneStepAhead(z3, D, np.zeros(2, dtype=np.int32))
    assert osa3.standardized.shape == (2, 3, 5) and np.array_equal(osa3.standardized[:, 1], z3[:, 1] / np.sqrt(D))
    assert osa3.log_density.shape == (2, 3, 5)


# ---------------------------------------------------------------------------------------------------------------------
# the identities on the oracle's factor
# ---------------------------------------------------------------------------------------------------------------------

def kernel_value(case, p, tau):
    """k_p(tau) by the six-coefficient formula (terms.py: RealTerm / ComplexTerm get_value)."""
    ar, cr, ac, bc, cc, dc = coeffs_of(case, p)
    tau = np.abs(np.asarray(tau, dtype=float))[..., None]
    return np.sum(ar * np.exp(-cr * tau), axis=-1) + np.sum(np.exp(-cc * tau) * (ac * np.cos(dc * tau) + bc * np.sin(dc * tau)), axis=-1)


def features(case, p, x):
    """(u(x), c): the reference's U~ row at x (cholesky.h:129-147) and the rows' decay rates."""
    ar, cr, ac, bc, cc, dc = coeffs_of(case, p)
    cd, sd = np.cos(dc * x), np.sin(dc * x)
    u = np.concatenate([ar, np.stack([ac * cd + bc * sd, ac * sd - bc * cd], axis=1).reshape(-1)])
    return u, np.concatenate([cr, np.repeat(cc, 2)])


def filter_by_recurrence(case, p, pts):
    """(z[N], D[N], mean[M], var[M], solver, k(0)) by the two forward recurrences on the oracle's factor."""
    t, y = case["t"][p], case["y"][p]
    s = ref.RefSolver()
    s.compute(0.0, *coeffs_of(case, p), *NO_GENERAL, t, case["diag"][p])
    ok, N, J, _, phi, _, W, D = s.state()
    assert ok and N == len(t)
    u = np.stack([features(case, p, tn)[0] for tn in t], axis=1)        # slot n: U~(t_n) (the factor stores it from n = 1)
    assert np.allclose(u[:, 1:], s.state()[5], rtol=0, atol=1e-12 * np.max(np.abs(u)))
    c = features(case, p, 0.0)[1]
    z, gp, Sp = np.empty(N), np.empty((N, J)), np.empty((N, J, J))
    g, S = np.zeros(J), np.zeros((J, J))
    for n in range(N):
        z[n] = y[n] - u[:, n] @ g
        gp[n] = g + W[:, n] * z[n]
        Sp[n] = S + D[n] * np.outer(W[:, n], W[:, n])
        if n + 1 < N:
            g = phi[:, n] * gp[n]
            S = np.outer(phi[:, n], phi[:, n]) * Sp[n]
    k0 = float(np.sum(case["a_real"][p]) + np.sum(case["a_comp"][p]))
    mean, var = np.empty(len(pts)), np.empty(len(pts))
    for i, x in enumerate(pts):
        m = int(np.searchsorted(t, x, side="left"))                   # samples with t_n < x
        if m == 0:
            mean[i], var[i] = 0.0, k0
            continue
        w = np.exp(-c * (x - t[m - 1])) * features(case, p, x)[0]
        mean[i] = w @ gp[m - 1]
        var[i] = k0 - w @ Sp[m - 1] @ w
    return z, D, mean, var, s, k0


def truncated_oracle(case, p, pts):
    """(mean[M], var[M]) of ``p(f(x) | y_n : t_n < x)``: ``RefSolver`` on ``t[:m]``, ``m = searchsorted(t, x, "left")``,
    per point; m = 0 is the prior and m = 1 the closed form of one sample (the reference wants two)."""
    t, y, diag = case["t"][p], case["y"][p], case["diag"][p]
    k0 = float(np.sum(case["a_real"][p]) + np.sum(case["a_comp"][p]))
    mean, var = np.empty(len(pts)), np.empty(len(pts))
    for i, x in enumerate(pts):
        m = int(np.searchsorted(t, x, side="left"))
        if m == 0:
            mean[i], var[i] = 0.0, k0
        elif m == 1:
            k = float(kernel_value(case, p, x - t[0]))
            mean[i], var[i] = k * y[0] / (k0 + diag[0]), k0 - k * k / (k0 + diag[0])
        else:
            r = ref.RefSolver()
            r.compute(0.0, *coeffs_of(case, p), *NO_GENERAL, t[:m], diag[:m])
            kstar = kernel_value(case, p, x - t[:m])
            mean[i] = r.predict(y[:m], np.array([x]))[0]
            var[i] = k0 - kstar @ r.solve(kstar)[:, 0]
    return mean, var


@pytest.mark.parametrize("family", ["bench", "accuracy"])
@pytest.mark.parametrize("JR,JC", [(2, 3), (1, 0), (0, 4)])
def test_the_identities_against_the_oracle(JR, JC, family):
    """About 40 unsorted points reaching 5 % past both ends, with ``t[0]``, ``t[-1]`` and interior data times among them;
    the innovations through the oracle's ``dot_solve`` and ``dot_L``."""
    N = 700
    case = synthetic(1, N, JR, JC, family, seed=300 + JR + 5 * JC)
    t, y = case["t"][0], case["y"][0]
    rng = np.random.RandomState(11 + JR + 3 * JC)
    lo, hi = t[0], t[-1]
    pad = 0.05 * (hi - lo)
    pts = np.concatenate([rng.uniform(lo - pad, hi + pad, 30), [lo - pad, hi + pad, t[0], t[-1]], t[3::97]])
    pts = pts[rng.permutation(len(pts))]
    assert 38 <= len(pts) <= 45 and np.sum(pts < lo) >= 1 and np.sum(pts > hi) >= 1 and np.sum(np.isin(pts, t)) >= 9
    z, D, mean, var, s, k0 = filter_by_recurrence(case, 0, pts)
    want_mean, want_var = truncated_oracle(case, 0, pts)
    tag = "NumPy identity vs oracle (%d, %d), %s family" % (JR, JC, family)
    dev_mean = np.max(np.abs(mean - want_mean)) / np.max(np.abs(y))
    dev_var = np.max(np.abs(var - want_var)) / k0
    quad = s.dot_solve(y)
    dev_quad = abs(np.sum(z * z / D) - quad) / abs(quad)
    dev_L = np.max(np.abs(s.dot_L(z / np.sqrt(D))[:, 0] - y)) / np.max(np.abs(y))
    print("%s: mean %.3e of max|y|, var %.3e k(0), sum z^2/D %.3e relative, L (z / sqrt D) - r %.3e of max|r|"
          % (tag, dev_mean, dev_var, dev_quad, dev_L))
    within("causal forecast, " + tag + ": mean, of max|y|", dev_mean, PREDICT)
    within("causal forecast, " + tag + ": var, of k(0)", dev_var, PREDICT)
    within("one step ahead, " + tag + ": sum z^2 / D vs dot_solve (relative)", dev_quad, 1e-12)
    within("one step ahead, " + tag + ": L (z / sqrt D) vs r, of max|r|", dev_L, 1e-12)
