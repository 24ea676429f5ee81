# -*- coding: utf-8 -*-
"""The predictive variance by recurrence (``predict(xs, return_var=True, method="recurrence")``,
``clr_batch_predict_var_recurrence``), the parts that need no GPU: the exported symbols, the ``method`` argument on both
plan classes, and a NumPy restatement of the identity the kernels of csrc/clr_bpredvar_rec_kernels.h implement, on the
oracle's factor.

In slot notation (slot n: ``phi[n]`` the decay n -> n+1, ``u[n] = U~(t_n)``, ``W[n]``, ``D[n]``), with ``v(x) = (1..,
cos d x, sin d x)``, ``u(x)`` the reference's feature rows at a point x, ``c`` the rows' decay rates and m the number of
samples with ``t_n <= x``::

    S+_n = S_n + D_n W_n W_n^T ,  S_{n+1} = Phi_n S+_n Phi_n ,  S_0 = 0
    Q_n  = u_n u_n^T / D_n + F_n^T Q_{n+1} F_n ,  F_n = Phi_n (I - W_n u_n^T) ,  Q_N = 0
    psi  = exp(-c (x - t_{m-1})) ,  S^x = psi psi^T o S+_{m-1}                   (m = 0: S^x = 0)
    e    = v(x) - S^x u(x) ,  e' = exp(-c (t_m - x)) o e
    var(x) = k(0) - u(x)^T S^x u(x) - e'^T Q_m e'                                (m = N: the last term is 0)

held against the oracle value ``k(0) - sum k* o solve(k*)`` (celerite.py:465-470 on the oracle's factor).

Bar: 1e-10 k(0), the project's PREDICT bar.  Measured (N = 700, 42 points): at most 5.4e-15 k(0) over the three shapes and
both families."""
import inspect

import numpy as np
import pytest

import __graft_entry__
from celerite_amd import batch
from oracle import ref
from _cases import NO_GENERAL, synthetic, coeffs_of, within

PREDICT = 1e-10
SYMBOLS = ["clr_batch_predict_var_recurrence", "clr_sharded_predict_var_recurrence"]


def test_the_new_symbols_are_declared_and_exported():
    declared = __graft_entry__.declared_symbols()
    lib = batch._load()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("cls", [batch.BatchedGP, batch.ShardedBatchedGP])
def test_the_method_argument_is_on_both_plan_classes(cls):
    """``method="solve"`` is the default; any other string than the two routes raises ValueError before anything is
    loaded or touched -- shown on a stub that is no plan at all, with and without ``return_var``."""
    sig = inspect.signature(cls.predict)
    assert list(sig.parameters) == ["self", "xs", "return_var", "mean_basis", "method"]
    assert sig.parameters["method"].default == "solve"
    stub = object()
    for return_var in (True, False):
        for bad in ("nonsense", "", "Recurrence", None):
            with pytest.raises(ValueError, match="method"):
                cls.predict(stub, np.zeros(3), return_var=return_var, method=bad)
    for good in ("solve", "recurrence"):      # (accepted: the stub fails later, as no plan)
        with pytest.raises(Exception) as err:
            cls.predict(stub, np.zeros(3), return_var=True, method=good)
        assert not (isinstance(err.value, ValueError) and "method" in str(err.value))


# ---------------------------------------------------------------------------------------------------------------------
# the identity on the oracle's factor
# ---------------------------------------------------------------------------------------------------------------------

def kernel_value(case, p, tau):
    """k_p(tau) by the six-coefficient formula (terms.py: RealTerm / ComplexTerm get_value)."""
    ar, cr, ac, bc, cc, dc = coeffs_of(case, p)
    tau = np.abs(np.asarray(tau, dtype=float))[..., None]
    return np.sum(ar * np.exp(-cr * tau), axis=-1) + np.sum(np.exp(-cc * tau) * (ac * np.cos(dc * tau) + bc * np.sin(dc * tau)), axis=-1)


def features(case, p, x):
    """(u(x), v(x), c): the reference's U~, V~ rows at x (cholesky.h:129-147) and the rows' decay rates."""
    ar, cr, ac, bc, cc, dc = coeffs_of(case, p)
    cd, sd = np.cos(dc * x), np.sin(dc * x)
    u = np.concatenate([ar, np.stack([ac * cd + bc * sd, ac * sd - bc * cd], axis=1).reshape(-1)])
    v = np.concatenate([np.ones(len(ar)), np.stack([cd, sd], axis=1).reshape(-1)])
    return u, v, np.concatenate([cr, np.repeat(cc, 2)])


def variance_by_recurrence(case, p, pts):
    """var at ``pts`` (any order) by the two matrix recurrences on the oracle's factor, in the local frame."""
    t = case["t"][p]
    s = ref.RefSolver()
    s.compute(0.0, *coeffs_of(case, p), *NO_GENERAL, t, case["diag"][p])
    ok, N, J, _, phi, _, W, D = s.state()
    assert ok and N == len(t)
    u = np.stack([features(case, p, tn)[0] for tn in t], axis=1)        # slot n: U~(t_n) (the factor stores it from n = 1)
    assert np.allclose(u[:, 1:], s.state()[5], rtol=0, atol=1e-12 * np.max(np.abs(u)))
    c = features(case, p, 0.0)[2]
    # S+_n for every n
    Sp = np.empty((N, J, J))
    S = np.zeros((J, J))
    for n in range(N):
        Sp[n] = S + D[n] * np.outer(W[:, n], W[:, n])
        if n + 1 < N:
            S = np.outer(phi[:, n], phi[:, n]) * Sp[n]
    # Q_n for n = 0 .. N
    Q = np.zeros((N + 1, J, J))
    Q[N - 1] = np.outer(u[:, N - 1], u[:, N - 1]) / D[N - 1]      # (the last sample's transition is 0)
    for n in range(N - 2, -1, -1):
        F = phi[:, n][:, None] * (np.eye(J) - np.outer(W[:, n], u[:, n]))
        Q[n] = np.outer(u[:, n], u[:, n]) / D[n] + F.T @ Q[n + 1] @ F
    k0 = float(np.sum(case["a_real"][p]) + np.sum(case["a_comp"][p]))
    var = np.empty(len(pts))
    for i, x in enumerate(pts):
        m = int(np.searchsorted(t, x, side="right"))                  # samples with t_n <= x
        ux, vx, _ = features(case, p, x)
        if m == 0:
            Sx = np.zeros((J, J))
        else:
            psi = np.exp(-c * (x - t[m - 1]))
            Sx = np.outer(psi, psi) * Sp[m - 1]
        e = vx - Sx @ ux
        right = 0.0
        if m < N:
            ep = np.exp(-c * (t[m] - x)) * e
            right = ep @ Q[m] @ ep
        var[i] = k0 - ux @ Sx @ ux - right
    return var, s, k0


@pytest.mark.parametrize("family", ["bench", "accuracy"])
@pytest.mark.parametrize("JR,JC", [(2, 3), (1, 0), (0, 4)])
def test_the_identity_against_the_oracle(JR, JC, family):
    """About 40 points reaching 5 % past both ends, with exact data times (the first and the last sample among them),
    in no particular order."""
    N = 700
    case = synthetic(1, N, JR, JC, family, seed=300 + JR + 5 * JC)
    t = case["t"][0]
    rng = np.random.RandomState(11 + JR + 3 * JC)
    lo, hi = t[0], t[-1]
    pad = 0.05 * (hi - lo)
    pts = np.concatenate([rng.uniform(lo - pad, hi + pad, 30), [lo - pad, hi + pad, t[0], t[-1]], t[3::97]])
    pts = pts[rng.permutation(len(pts))]
    assert 38 <= len(pts) <= 45 and np.sum(pts < lo) >= 1 and np.sum(pts > hi) >= 1 and np.sum(np.isin(pts, t)) >= 9
    var, s, k0 = variance_by_recurrence(case, 0, pts)
    kstar = kernel_value(case, 0, pts[None, :] - t[:, None])
    want = k0 - np.sum(kstar * s.solve(kstar), axis=0)
    dev = np.max(np.abs(var - want)) / k0
    print("identity vs oracle (%d, %d), %s family: max |var - oracle| / k(0) = %.3e" % (JR, JC, family, dev))
    within("predictive variance by recurrence, NumPy identity vs oracle (%d, %d), %s family, of k(0)" % (JR, JC, family), dev, PREDICT)
