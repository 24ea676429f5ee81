# -*- coding: utf-8 -*-
"""No GPU: the identities behind ``BatchedGP.predict_cov`` / ``sample_conditional`` (csrc/clr_bcond_kernels.h) restated in
NumPy (tests/_conditional_recurrence.py, no product code) against the dense ``k(x, x') - k*^T K^-1 k*'`` at every narrow
kernel shape, and the argument checks of the two Python methods that need no device.

Measured (N = 60, 31 points, both families, all 24 shapes): the pair formula and ``A A^T`` of the linear-time factor are
within 3.5e-15 k(0) of the dense value; the bar is a decade above, 4e-14 k(0)."""
import numpy as np
import pytest

from _cases import ALL_WIDTH_SHAPES, synthetic, coeffs_of, within
import _conditional_recurrence as cond
from _predict_terms_recurrence import predict_terms_by_recurrence

BAR = 4e-14
N = 60
_MODEL = {}


def points_of(t, seed):
    """31 ascending points: 22 random ones reaching 5 % past both ends, both ends, five exact data times, and two points
    1e-9 of the span apart inside one gap."""
    rng = np.random.RandomState(seed)
    lo, hi = t[0], t[-1]
    pad = 0.05 * (hi - lo)
    mid = 0.5 * (t[30] + t[31])
    xs = np.sort(np.concatenate([rng.uniform(lo - pad, hi + pad, 22), [lo - pad, hi + pad], t[::13], [mid, mid + 1e-9 * (hi - lo)]]))
    assert len(xs) == 31 and xs[0] < lo and xs[-1] > hi
    return xs


def model(JR, JC, family):
    """The generators, the covariance by the pair formula and the dense value of one problem, computed once."""
    key = (JR, JC, family)
    if key not in _MODEL:
        case = synthetic(1, N, JR, JC, family, seed=7 + JR + 9 * JC)
        t, diag, co = case["t"][0], case["diag"][0], coeffs_of(case, 0)
        xs = points_of(t, 3)
        e, r, T, k0 = cond.generators(co, t, diag, xs)
        _MODEL[key] = dict(case=case, xs=xs, e=e, r=r, T=T, k0=k0, C=cond.covariance(e, r, T),
                           dense=cond.dense_covariance(co, t, diag, xs))
    return _MODEL[key]


@pytest.mark.parametrize("family", ["bench", "accuracy"])
@pytest.mark.parametrize("JR,JC", ALL_WIDTH_SHAPES)
def test_pair_formula_is_the_dense_covariance(JR, JC, family):
    m = model(JR, JC, family)
    assert np.array_equal(m["C"], m["C"].T)
    within("conditional model: pair formula vs dense covariance, of k(0)", np.max(np.abs(m["C"] - m["dense"])) / m["k0"], BAR, (JR, JC, family))


@pytest.mark.parametrize("family", ["bench", "accuracy"])
@pytest.mark.parametrize("JR,JC", ALL_WIDTH_SHAPES)
def test_linear_time_factor_reproduces_the_covariance(JR, JC, family):
    """``A = L diag(d)^1/2`` from the draw recurrence on the identity; ``A A^T = C + reg I`` at reg = 0 and 1e-8 k(0); a draw
    from other normals is ``A n``."""
    m = model(JR, JC, family)
    M = len(m["xs"])
    for reg in (0.0, 1e-8 * m["k0"]):
        d, om, st = cond.factor(m["e"], m["r"], m["T"], m["k0"], regularize=reg, min_pivot=1e-13)
        assert st == 0 and (d > 0).all()
        A = cond.draw(m["r"], m["T"], d, om, np.eye(M)).T
        assert np.array_equal(np.triu(A, 1), np.zeros((M, M)))
        within("conditional model: A A^T vs dense covariance + reg, of k(0)",
               np.max(np.abs(A @ A.T - m["dense"] - reg * np.eye(M))) / m["k0"], BAR, (JR, JC, family, reg))
        n = np.random.RandomState(5).standard_normal((3, M))
        f = cond.draw(m["r"], m["T"], d, om, n)
        within("conditional model: a draw vs A n, of sqrt k(0)", np.max(np.abs(f - n @ A.T)) / np.sqrt(m["k0"]), 1e-13, (JR, JC, family))


@pytest.mark.parametrize("JR,JC", ALL_WIDTH_SHAPES)
def test_diagonal_is_the_recurrence_variance(JR, JC):
    m = model(JR, JC, "accuracy")
    case = m["case"]
    T = JR + JC
    var = predict_terms_by_recurrence(coeffs_of(case, 0), case["t"][0], case["diag"][0], case["y"][0], m["xs"], np.ones((1, T), dtype=bool))[1][0]
    within("conditional model: diag(C) vs the recurrence variance, of k(0)", np.max(np.abs(np.diag(m["C"]) - var)) / m["k0"], BAR, (JR, JC))


@pytest.mark.parametrize("JR,JC", [(1, 0), (2, 3), (0, 4), (8, 0)])
def test_a_repeated_point_has_a_degenerate_pivot(JR, JC):
    """A point given twice: the second pivot is within the bar of zero, its omega is 0, and the two columns of every draw
    are equal to rounding; without the rule the factor would divide by a pivot of rounding size.  A pivot below
    -min_pivot k(0) refuses the problem."""
    case = synthetic(1, N, JR, JC, "accuracy", seed=11)
    t, diag, co = case["t"][0], case["diag"][0], coeffs_of(case, 0)
    xs = np.sort(np.concatenate([points_of(t, 4)[::3], [t[17] + 0.3 * (t[18] - t[17])] * 2]))
    rep = int(np.flatnonzero(np.diff(xs) == 0)[0]) + 1
    e, r, T, k0 = cond.generators(co, t, diag, xs)
    d, om, st = cond.factor(e, r, T, k0)
    assert st == 0 and d[rep] == 0.0 and not om[rep].any() and (np.delete(d, rep) > 0).all()
    n = np.random.RandomState(2).standard_normal((4, len(xs)))
    f = cond.draw(r, T, d, om, n)
    # the second column is r^T (gamma + omega z) against z + r^T gamma: r^T omega = (r^T e - r^T G r) / d is 1 up to the
    # rounding of a difference of numbers of size k(0) over d, 64 roundings at most at width 8, times z = sqrt(d) n
    bar = 64 * np.finfo(float).eps * k0 / np.sqrt(d[rep - 1]) * np.max(np.abs(n))
    within("conditional model: the two columns of a repeated point, of their bar", np.max(np.abs(f[:, rep] - f[:, rep - 1])) / bar, 1.0, (JR, JC))
    A = cond.draw(r, T, d, om, np.eye(len(xs))).T
    within("conditional model: A A^T with a repeated point, of k(0)", np.max(np.abs(A @ A.T - cond.dense_covariance(co, t, diag, xs))) / k0, BAR, (JR, JC))
    assert cond.factor(e, r, T, k0, regularize=-0.5 * (r[0] @ e[0]) - k0)[2] == cond.NOT_POSITIVE_DEFINITE


class _Plan(object):
    """What the argument checks read of a plan; the library is never reached."""
    B, N, J_real, J_comp, _h = 3, 200, 1, 1, None

    def predict(self, xs, mean_basis=None):
        raise AssertionError("the device was reached")


def _unreachable(status):
    raise AssertionError("the library was reached")


def test_argument_checks_need_no_device():
    from celerite_amd import batch
    plan, xs = _Plan(), np.linspace(0.0, 1.0, 5)
    call = lambda **kw: batch._sample_conditional(plan, "clr_batch_sample_conditional", _unreachable, kw.pop("xs", xs), kw.pop("size", None),
                                                  kw.pop("regularize", 0.0), kw.pop("min_pivot", 1e-10), kw.pop("mean_basis", None),
                                                  kw.pop("random", None), kw.pop("normals", None), False)
    for bad in (dict(xs=np.zeros((2, 5))), dict(xs=np.zeros((3, 2, 5))), dict(size=0), dict(size=-1), dict(size=1.5), dict(size=True),
                dict(min_pivot=-1e-3), dict(min_pivot=1.0), dict(min_pivot=np.nan), dict(regularize=-1.0), dict(regularize=np.inf),
                dict(normals=np.zeros((3, 4))), dict(normals=np.zeros((3, 5)), size=2), dict(normals=np.zeros((3, 2, 5))),
                dict(mean_basis=np.ones((1, 5)))):
        with pytest.raises(ValueError):
            call(**bad)
    for bad in (np.zeros((2, 5)), np.zeros((3, 2, 5))):
        with pytest.raises(ValueError):
            batch._predict_cov(plan, "clr_batch_predict_cov", _unreachable, bad)
    for cls in (batch.BatchedGP, batch.ShardedBatchedGP):
        for name in ("predict_cov", "sample_conditional", "set_conditional_tile"):
            assert callable(getattr(cls, name)), (cls, name)
