# -*- coding: utf-8 -*-
"""`-m gpu`: the causal half of a batched plan's factor -- ``BatchedGP.one_step_ahead`` (``clr_batch_one_step_ahead``: the
innovations ``z = L^-1 r`` and their variances ``D``) and ``BatchedGP.forecast`` (``clr_batch_forecast``: mean and variance
at a point given the samples strictly before it) -- at every narrow kernel shape in both factor layouts, at the chunk
edges, against each other, across a long gap, across tiles, under both mean models, across reuse of the cached state, with
several right-hand sides, on the library-trig kernels, on wide plans, sharded, and where they refuse.

Oracle values: ``z`` is the forward substitution in NumPy on ``RefSolver.state()``, ``D`` the oracle's; a forecast is
``RefSolver`` on the truncated series ``t[:m]``, ``m = searchsorted(t, x, "left")``, per point (m = 0: the prior; m = 1: the
closed form of one sample).  The identities themselves are pinned in NumPy by tests/test_filter_cpu.py.

Bars: ``variance`` against the oracle's ``D`` 1e-11 relative (test_gpu_batch.py: test_materialised_factor_matches_oracle_state);
``innovation`` 1e-10 (narrow) and 2e-11 (wide) of the largest entry, the solve bars of tests/test_gpu_batch_consumers.py;
the forecast mean 1e-10 of the largest entry, that file's predict bar; the forecast variance 1e-10 k(0).

Largest deviations seen on the MI355X (all tests of this file): ``innovation`` 3.8e-14 of the largest entry on narrow plans
and 5.2e-15 on wide ones; ``variance`` 5.3e-13 relative (narrow), 5.6e-14 (wide); the forecast mean 4.1e-15 of the largest;
the forecast variance 2.3e-14 k(0), and 1.0e-8 k(0) on the library-trig kernels at t ~ 3e8 (the phase's rounding); the
forecast at the samples against ``y - innovation`` 4.0e-16 of the largest |y| and against ``variance - diag - jitter``
3.3e-15 k(0); ``dot_L(z / sqrt D)`` back to ``b`` within 2.4e-16 of the largest entry."""
import ctypes as C

import numpy as np
import pytest

from celerite_amd import batch
from oracle import ref
from _cases import ALL_WIDTH_SHAPES, synthetic, coeffs_of, within, grad_family_long_gap, edge_points

pytestmark = pytest.mark.gpu

NARROW_SOLVE, WIDE_SOLVE, DOT, PREDICT, D_BAR = 1e-10, 2e-11, 1e-12, 1e-10, 1e-11
PHASE_ROUNDING = 1e-6          # tests/test_gpu_batch_consumers.py: test_narrow_consumers_on_the_library_trig_kernels
NOGEN = (np.empty(0), np.empty((0, 0)), np.empty((0, 0)))
NARROW_B, NARROW_N, NARROW_CHUNKS, L = 4, 700, (22, 32), 32    # set_chunks(24): chunks of 32 samples, the last one 28
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def kernel_value(case, p, tau):
    """k_p(tau) by the six-coefficient formula (terms.py: RealTerm / ComplexTerm get_value)."""
    ar, cr, ac, bc, cc, dc = coeffs_of(case, p)
    tau = np.abs(np.asarray(tau, dtype=float))[..., None]
    return np.sum(ar * np.exp(-cr * tau), axis=-1) + np.sum(np.exp(-cc * tau) * (ac * np.cos(dc * tau) + bc * np.sin(dc * tau)), axis=-1)


def k_zero(case, p):
    return float(np.sum(case["a_real"][p]) + np.sum(case["a_comp"][p]))


def oracle_solver(case, p, m=None):
    r = ref.RefSolver()
    r.compute(0.0, *coeffs_of(case, p), *NOGEN, case["t"][p][:m], case["diag"][p][:m])
    return r


def oracle_innovations(case, p, rhs):
    """(z[nrhs, N], D[N]): the forward substitution of cholesky.h:240-249 before its division, on the oracle's factor."""
    _, N, J, _, phi, u, W, D = oracle_solver(case, p).state()
    b = np.atleast_2d(rhs)
    z = np.empty(b.shape)
    f = np.zeros((J, b.shape[0]))
    z[:, 0] = b[:, 0]
    for n in range(1, N):
        f = phi[:, n - 1, None] * (f + W[:, n - 1, None] * z[:, n - 1])
        z[:, n] = b[:, n] - u[:, n - 1] @ f
    return z, D


def oracle_forecast(case, p, pts, resid=None):
    """(mean[M], var[M]) of ``p(f(x) | r_n : t_n < x)`` by ``RefSolver`` on the truncated series, per point."""
    t, diag = case["t"][p], case["diag"][p]
    y = case["y"][p] if resid is None else resid
    k0 = k_zero(case, p)
    mean, var = np.empty(len(pts)), np.empty(len(pts))
    for i, x in enumerate(pts):
        m = int(np.searchsorted(t, x, side="left"))
        if m == 0:
            mean[i], var[i] = 0.0, k0
        elif m == 1:
            k = float(kernel_value(case, p, x - t[0]))
            mean[i], var[i] = k * y[0] / (k0 + diag[0]), k0 - k * k / (k0 + diag[0])
        else:
            r = oracle_solver(case, p, m)
            kstar = kernel_value(case, p, x - t[:m])
            mean[i] = r.predict(y[:m], np.array([x]))[0]
            var[i] = k0 - kstar @ r.solve(kstar)[:, 0]
    return mean, var


def points_of(pts, p):
    return pts[p] if pts.ndim == 2 else pts


def check_forecast(tag, case, pts, mean, var, resid=None, model=None, bar_mean=PREDICT, bar_var=PREDICT, skip=()):
    """Every problem against the truncated oracle; ``resid``: what the oracle conditions on (y less the model at the
    samples), ``model``: the mean model at the points, (B, M)."""
    B = case["t"].shape[0]
    worst = [0.0, 0.0]
    for p in range(B):
        if p in skip:
            continue
        x = points_of(pts, p)
        r = case["y"][p] if resid is None else resid[p]
        want_mean, want_var = oracle_forecast(case, p, x, r)
        if model is not None:
            want_mean = want_mean + model[p]
        scale = np.max(np.abs(want_mean)) or np.max(np.abs(r))       # (of the largest, as the predict bar is taken)
        if mean is not None:
            dev = np.max(np.abs(mean[p] - want_mean)) / scale
            worst[0] = max(worst[0], dev) if dev == dev else float("nan")
            within(tag + ": forecast mean vs truncated oracle, of the largest", dev, bar_mean, p)
        if var is not None:
            dev = np.max(np.abs(var[p] - want_var)) / k_zero(case, p)
            worst[1] = max(worst[1], dev) if dev == dev else float("nan")
            within(tag + ": forecast var vs truncated oracle, of k(0)", dev, bar_var, p)
    print("%s: mean %.3e of the largest, var %.3e k(0)" % (tag, worst[0], worst[1]))


def check_innovations(tag, case, osa, rhs=None, bar=NARROW_SOLVE, skip=()):
    B = case["t"].shape[0]
    worst = [0.0, 0.0]
    for p in range(B):
        if p in skip:
            continue
        b = case["y"][p] if rhs is None else rhs[p]
        z0, D0 = oracle_innovations(case, p, b)
        z = np.atleast_2d(osa.innovation[p])
        dz = float(np.max(np.abs(z - z0)) / np.max(np.abs(z0)))
        dD = float(np.max(np.abs(osa.variance[p] - D0) / np.abs(D0)))
        worst = [max(worst[0], dz), max(worst[1], dD)]
        within(tag + ": innovation vs oracle forward substitution, of the largest entry", dz, bar, p)
        within(tag + ": variance vs oracle D (relative)", dD, D_BAR, p)
    print("%s: innovation %.3e of the largest entry, variance %.3e relative" % (tag, worst[0], worst[1]))


def narrow_plan(case, JR, JC, layout, chunks=24, expect=NARROW_CHUNKS, cls=batch.BatchedGP, **kw):
    B, N = case["t"].shape
    plan = cls(B, N, JR, JC, **kw)
    plan.set_chunks(chunks)
    if expect and cls is batch.BatchedGP:
        assert plan.chunks == expect and N % expect[1] != 0      # a ragged last chunk
    if layout:
        plan.set_factor_layout(layout)
    plan.set_series(case["t"], case["diag"], case["y"])
    plan.set_coefficients(*coeffs_of(case))
    return plan


# ---------------------------------------------------------------------------------------------------------------------
# 1. every narrow shape, both factor layouts, both families
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["reference", "lean"])
@pytest.mark.parametrize("JR,JC", ALL_WIDTH_SHAPES)
def test_filter_at_every_narrow_shape(JR, JC, layout):
    """The kernels are compiled per (J_real, J_comp), factor layout, trig flavour and with / without points and variance
    (``bfilter_forward_kernel`` in csrc/clr_bfilter_kernels.h): all 24 shapes, both layouts, both families, 22 chunks with
    a ragged last one of 28.  ``one_step_ahead()`` against the oracle, and ``sum log D`` / ``sum z^2 / D`` against the plan's
    own log det and quadratic form; ``forecast`` with and without ``return_var`` at shared sorted points, per-problem points
    and an unsorted permutation of the shared ones, which must give the sorted result permuted, bit for bit."""
    B, N = NARROW_B, NARROW_N
    for family in ("bench", "accuracy"):
        case = synthetic(B, N, JR, JC, family, seed=500 + 9 * JC + JR)
        shared, own, perm = edge_points(case, np.random.RandomState(40 + JR + 7 * JC))
        plan = narrow_plan(case, JR, JC, layout)
        try:
            assert plan.chunks == (22, 32) and N - 21 * 32 == 28
            ll, ld, q, st = plan.log_likelihood(materialize=True)
            assert (st == 0).all()
            osa = plan.one_step_ahead()
            mean_only = plan.forecast(shared)
            mean, var = plan.forecast(shared, return_var=True)
            mean_own, var_own = plan.forecast(own, return_var=True)
            mean_perm, var_perm = plan.forecast(shared[perm], return_var=True)
            mean_perm_only = plan.forecast(shared[perm])
        finally:
            plan.close()
        tag = "filter (%s layout, %s family)" % (layout, family)
        assert (osa.status == 0).all() and osa.innovation.shape == (B, N) and osa.variance.shape == (B, N)
        assert np.array_equal(mean_only, mean), tag
        assert np.array_equal(mean_perm, mean[:, perm]) and np.array_equal(var_perm, var[:, perm]), tag
        assert np.array_equal(mean_perm_only, mean_perm), tag
        check_innovations(tag, case, osa)
        within(tag + ": sum log D vs the plan's log det (relative)", np.max(np.abs(np.sum(np.log(osa.variance), axis=1) - ld) / np.abs(ld)), 1e-10)
        within(tag + ": sum z^2 / D vs the plan's quadratic form (relative)",
               np.max(np.abs(np.sum(osa.innovation ** 2 / osa.variance, axis=1) - q) / np.abs(q)), 1e-10)
        within(tag + ": sum log_density vs the plan's log-likelihood (relative)", np.max(np.abs(np.sum(osa.log_density, axis=1) - ll) / np.abs(ll)), 1e-10)
        check_forecast(tag + ", shared points", case, shared, mean, var)
        check_forecast(tag + ", per-problem points", case, own, mean_own, var_own)


# ---------------------------------------------------------------------------------------------------------------------
# 2. consistency: the forecast at the data times, and past the last sample
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC,layout", [(2, 3, "lean"), (4, 2, "reference"), (1, 0, "lean")])
def test_forecast_at_the_samples_is_the_one_step_ahead_prediction(JR, JC, layout):
    """``forecast(t, return_var=True)`` with ``xs = t`` of shape (B, N) equals ``y - innovation`` and ``variance - diag -
    jitter`` to the forecast bars (the points take psi from the library exp, the samples the stored phi: to rounding, not
    bit for bit); points beyond the last sample equal ``predict(xs, return_var=True)`` on both variance routes within two
    PREDICT bars."""
    B, N = NARROW_B, NARROW_N
    jitter = 0.01
    for family in ("bench", "accuracy"):
        case = synthetic(B, N, JR, JC, family, seed=90 + JR)
        span = case["t"].max() - case["t"].min()
        beyond = case["t"][:, -1:] + span * np.array([1e-6, 1e-3, 0.01, 0.05])[None, :]
        plan = narrow_plan(case, JR, JC, layout)
        try:
            plan.set_coefficients(*coeffs_of(case), jitter=jitter)
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            osa = plan.one_step_ahead()
            mean, var = plan.forecast(case["t"], return_var=True)
            fm, fv = plan.forecast(beyond, return_var=True)
            pm, pv = plan.predict(beyond, return_var=True)
            pv_rec = plan.predict(beyond, return_var=True, method="recurrence")[1]
        finally:
            plan.close()
        tag = "forecast at the samples (%d, %d) %s, %s family" % (JR, JC, layout, family)
        for p in range(B):
            ymax, k0 = np.max(np.abs(case["y"][p])), k_zero(case, p)
            within(tag + ": mean vs y - innovation, of the largest |y|", np.max(np.abs(mean[p] - (case["y"][p] - osa.innovation[p]))) / ymax, PREDICT, p)
            within(tag + ": var vs variance - diag - jitter, of k(0)", np.max(np.abs(var[p] - (osa.variance[p] - case["diag"][p] - jitter))) / k0, PREDICT, p)
            within(tag + ": beyond the end, mean vs predict, of the largest |y|", np.max(np.abs(fm[p] - pm[p])) / ymax, 2 * PREDICT, p)
            within(tag + ": beyond the end, var vs predict_var (solve), of k(0)", np.max(np.abs(fv[p] - pv[p])) / k0, 2 * PREDICT, p)
            within(tag + ": beyond the end, var vs predict_var (recurrence), of k(0)", np.max(np.abs(fv[p] - pv_rec[p])) / k0, 2 * PREDICT, p)


# ---------------------------------------------------------------------------------------------------------------------
# 3. a long gap
# ---------------------------------------------------------------------------------------------------------------------

def test_forecast_across_a_long_gap():
    """``grad_family_long_gap``'s times with the gap stretched until ``exp(-c gap)`` underflows for every row: points deep
    inside the gap give the prior -- mean 0 and var k(0) exactly, no NaN from an underflowing psi --, points just inside
    and beyond it the oracle's values."""
    JR, JC, B, N = 2, 3, 2, 700
    one = [grad_family_long_gap(N, JR, JC, seed=s) for s in range(B)]
    case = {k: np.stack([o[k] for o in one]) for k in one[0]}
    k = int(0.37 * N)
    gap0 = case["t"][:, k] - case["t"][:, k - 1]
    case["t"][:, k:] += 1000.0 * gap0[:, None]                     # c gap = 2e3 .. 2e4: exp underflows
    cmin = np.minimum(case["c_real"].min(axis=1), case["c_comp"].min(axis=1))
    assert (np.exp(-cmin * 500.0 * gap0) == 0.0).all()
    deep = case["t"][:, k - 1, None] + gap0[:, None] * np.array([500.0, 700.0, 999.0])[None, :]
    near = np.stack([np.concatenate([[case["t"][p, k - 1] + 1e-3 * gap0[p]], case["t"][p, k:k + 3], [case["t"][p, -1] + gap0[p]]]) for p in range(B)])
    pts = np.sort(np.concatenate([deep, near], axis=1), axis=1)
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        mean, var = plan.forecast(pts, return_var=True)
        dm, dv = plan.forecast(deep, return_var=True)
    finally:
        plan.close()
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    assert (dm == 0.0).all() and np.allclose(dv, [[k_zero(case, p)] for p in range(B)], rtol=1e-15, atol=0)
    check_forecast("forecast across a long gap", case, pts, mean, var)


# ---------------------------------------------------------------------------------------------------------------------
# 4. tiles
# ---------------------------------------------------------------------------------------------------------------------

def test_forecast_does_not_depend_on_the_tile():
    """Tiles of 1, of 7 (M = 40: a ragged last tile) and the automatic tile give the same bits, with and without var."""
    JR, JC, B, N, M = 2, 3, 3, 700, 40
    case = synthetic(B, N, JR, JC, "accuracy", seed=24)
    xs = np.sort(np.random.RandomState(3).uniform(case["t"].min() - 10.0, case["t"].max() + 10.0, M))
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        got, plain = {}, {}
        for tile in (1, 7, 0):
            plan.set_predict_tile(tile)
            got[tile] = plan.forecast(xs, return_var=True)
            plain[tile] = plan.forecast(xs)
    finally:
        plan.close()
    for tile in (1, 7):
        assert np.array_equal(got[tile][0], got[0][0]) and np.array_equal(got[tile][1], got[0][1]), tile
        assert np.array_equal(plain[tile], got[0][0]), tile
    check_forecast("forecast across tiles", case, xs, got[0][0], got[0][1])


# ---------------------------------------------------------------------------------------------------------------------
# 5. means
# ---------------------------------------------------------------------------------------------------------------------

def test_filter_under_both_mean_models():
    """A constant mean per problem, then a linear mean (K = 3) with ``mean_basis``: the oracle runs on y less the model
    and the model at the points is added.  After new values a second call equals a fresh plan's, bit for bit: the start
    states of g follow the residual and are never kept."""
    JR, JC, B, N = 2, 3, NARROW_B, NARROW_N
    case = synthetic(B, N, JR, JC, "bench", seed=23)
    shared, own, perm = edge_points(case, np.random.RandomState(9))
    rng = np.random.RandomState(4)
    mu1, mu2 = np.linspace(-1.0, 2.0, B), rng.uniform(-3.0, 3.0, B)
    tn = case["t"][0] / case["t"].max()
    Phi = np.stack([np.ones(N), tn, np.sin(7.0 * tn)])
    sx = shared / case["t"].max()
    Phi_x = np.stack([np.ones(len(shared)), sx, np.sin(7.0 * sx)])
    w1, w2 = rng.uniform(-0.5, 0.5, (B, 3)), rng.uniform(-0.5, 0.5, (B, 3))
    out = {}
    plan = narrow_plan(case, JR, JC, "lean")
    fresh = narrow_plan(case, JR, JC, "lean")
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        assert (fresh.log_likelihood(materialize=True)[3] == 0).all()
        plain = plan.forecast(shared, return_var=True)
        plan.set_mean(mu1)
        out["const 1"] = plan.one_step_ahead(), plan.forecast(shared, return_var=True)
        plan.set_mean(mu2)
        out["const 2"] = plan.one_step_ahead(), plan.forecast(shared, return_var=True)
        fresh.set_mean(mu2)
        out["const 2 fresh"] = fresh.one_step_ahead(), fresh.forecast(shared, return_var=True)
        for q in (plan, fresh):
            q.set_mean(None)
            q.set_mean_basis(Phi)
        plan.set_mean_weights(w1)
        out["linear 1"] = plan.one_step_ahead(), plan.forecast(shared, return_var=True, mean_basis=Phi_x)
        plan.set_mean_weights(w2)
        out["linear 2"] = plan.one_step_ahead(), plan.forecast(shared, return_var=True, mean_basis=Phi_x)
        fresh.set_mean_weights(w2)
        out["linear 2 fresh"] = fresh.one_step_ahead(), fresh.forecast(shared, return_var=True, mean_basis=Phi_x)
        with pytest.raises(ValueError, match="a linear mean is in force"):
            plan.forecast(shared)
    finally:
        plan.close()
        fresh.close()
    for key in ("const 2", "linear 2"):
        (a, fa), (b, fb) = out[key], out[key + " fresh"]
        assert np.array_equal(a.innovation, b.innovation) and np.array_equal(a.variance, b.variance), key
        assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1]), key
    ones = np.ones((1, len(shared)))
    for key, resid, model in (("const 1", case["y"] - mu1[:, None], mu1[:, None] * ones), ("const 2", case["y"] - mu2[:, None], mu2[:, None] * ones),
                              ("linear 1", case["y"] - w1 @ Phi, w1 @ Phi_x), ("linear 2", case["y"] - w2 @ Phi, w2 @ Phi_x)):
        osa, (mean, var) = out[key]
        assert np.array_equal(var, plain[1]) and not np.array_equal(mean, plain[0]), key      # (a mean changes the residual, not K)
        check_innovations("filter under a mean, " + key, case, osa, rhs=resid)
        check_forecast("filter under a mean, " + key, case, shared, mean, var, resid=resid, model=model)


# ---------------------------------------------------------------------------------------------------------------------
# 6. reuse of the cached state
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["lean", "reference"])
def test_filter_reuses_and_renews_the_cached_state(layout):
    """``forecast``, ``solve()``, ``predict(method="recurrence")``, ``leave_one_out()``, ``one_step_ahead()`` and ``forecast``
    again, interleaved: each returns the bits a fresh plan returns for that call alone (the chunk maps, the forward start
    states of S and the backward start matrices are shared; none may go stale).  After a second materialising run with
    other coefficients everything follows the new factor."""
    JR, JC, B, N = 2, 3, NARROW_B, NARROW_N
    case = synthetic(B, N, JR, JC, "bench", seed=12)
    other = synthetic(B, N, JR, JC, "bench", seed=13)
    other["t"], other["diag"], other["y"] = case["t"], case["diag"], case["y"]
    shared, own, perm = edge_points(case, np.random.RandomState(5))
    calls = {"forecast": lambda q: plan_forecast(q, own), "solve": lambda q: (q.solve(),),
             "predict": lambda q: q.predict(own, return_var=True, method="recurrence"),
             "loo": lambda q: q.leave_one_out()[3:5], "osa": lambda q: q.one_step_ahead()[:2]}

    def plan_forecast(q, xs):
        return q.forecast(xs, return_var=True)

    alone = {}
    for name, call in calls.items():
        q = narrow_plan(case, JR, JC, layout)
        try:
            assert (q.log_likelihood(materialize=True)[3] == 0).all()
            alone[name] = call(q)
        finally:
            q.close()
    plan = narrow_plan(case, JR, JC, layout)
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        seq = [(name, calls[name](plan)) for name in ("forecast", "solve", "predict", "loo", "osa", "forecast", "predict", "solve", "osa")]
        mean_only = plan.forecast(own)
        plan.set_coefficients(*coeffs_of(other))
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        renewed = plan.forecast(own, return_var=True)
        renewed_osa = plan.one_step_ahead()
    finally:
        plan.close()
    for name, got in seq:
        for a, b in zip(got, alone[name]):
            assert np.array_equal(a, b), name
    assert np.array_equal(mean_only, alone["forecast"][0])
    assert not np.array_equal(renewed[0], alone["forecast"][0]) and not np.array_equal(renewed[1], alone["forecast"][1])
    check_forecast("filter (%s layout), first factor" % layout, case, own, *alone["forecast"])
    check_forecast("filter (%s layout), after a new materialising run" % layout, other, own, *renewed)
    check_innovations("filter (%s layout), after a new materialising run" % layout, other, renewed_osa)


# ---------------------------------------------------------------------------------------------------------------------
# 7. right-hand sides
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC,layout", [(2, 3, "lean"), (3, 1, "reference")])
def test_one_step_ahead_of_several_right_hand_sides(JR, JC, layout):
    """``b`` of shape (B, 3, N) and (B, N): against the oracle per column; ``dot_L(z / sqrt D)`` returns ``b`` within the
    consumers' ``dot_L`` bar; the call before and after a solve gives the same bits."""
    B, N = NARROW_B, NARROW_N
    case = synthetic(B, N, JR, JC, "accuracy", seed=31 + JR)
    rng = np.random.RandomState(17)
    b3, b1 = rng.randn(B, 3, N), rng.randn(B, N)
    plan = narrow_plan(case, JR, JC, layout)
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        osa3 = plan.one_step_ahead(b3)
        x = plan.solve(b3)
        osa3_again = plan.one_step_ahead(b3)
        osa1 = plan.one_step_ahead(b1)
        back = plan.dot_L(osa3.standardized)
    finally:
        plan.close()
    assert osa3.innovation.shape == (B, 3, N) and osa3.variance.shape == (B, N) and osa1.innovation.shape == (B, N)
    assert np.array_equal(osa3.innovation, osa3_again.innovation) and np.isfinite(x).all()
    tag = "one_step_ahead (%d, %d) %s" % (JR, JC, layout)
    check_innovations(tag + ", three rhs", case, osa3, rhs=b3)
    check_innovations(tag + ", one rhs", case, osa1, rhs=b1)
    for p in range(B):
        within(tag + ": dot_L(z / sqrt D) vs b, of the largest entry", np.max(np.abs(back[p] - b3[p])) / np.max(np.abs(b3[p])), DOT, p)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the library-trig instantiations
# ---------------------------------------------------------------------------------------------------------------------

def test_filter_on_the_library_trig_kernels():
    """A series offset to t ~ 3e8: max|d| max|t| >= CLR_FAST_TRIG_LIMIT, so the lean plan regenerates phi, u with the
    library sincos (``bfilter_go<true, false>``) and the points' features take it too.  The forecast variance against the
    oracle under the phase-rounding bar of tests/test_gpu_batch_consumers.py: the oracle's ``k*`` comes from the relative
    phase ``d (x - t_n)``, the kernels evaluate a point at its absolute phase ``d x``, rounded at 3e8 (measured 1.0e-8
    k(0)).  The innovations and the forecast mean, whose oracle takes absolute phases too, stay under the ordinary bars
    (measured 4.8e-16 and 4.1e-16)."""
    JR, JC, B, N = 2, 3, NARROW_B, NARROW_N
    case = synthetic(B, N, JR, JC, "accuracy", seed=77 + JR)
    case["t"] = case["t"] + 3.0e8
    shared, own, perm = edge_points(case, np.random.RandomState(91))
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        bounds = plan.selection_bounds()
        assert bounds["dmax"] * bounds["tmax"] >= 1.0e9, bounds        # CLR_FAST_TRIG_LIMIT (csrc/clr_core.h)
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        osa = plan.one_step_ahead()
        mean, var = plan.forecast(own, return_var=True)
    finally:
        plan.close()
    check_innovations("filter, library trig", case, osa)
    check_forecast("filter, library trig", case, own, mean, var, bar_var=PHASE_ROUNDING)


# ---------------------------------------------------------------------------------------------------------------------
# 9. wide plans
# ---------------------------------------------------------------------------------------------------------------------

def wide_plan(case, JR, JC):
    B, N = case["t"].shape
    plan = batch.BatchedGP(B, N, JR, JC)
    plan.set_series(case["t"], case["diag"], case["y"])
    plan.set_coefficients(*coeffs_of(case))
    return plan


@pytest.mark.parametrize("JR,JC", [(4, 4), (1, 10), (0, 32)])
def test_one_step_ahead_on_wide_plans(JR, JC):
    """Widths 12, 21 and 64 at N = 2048: the forward sweep of the wide solve, D from the factor; the plan's y and two
    uploaded right-hand sides."""
    B, N = 3, 2048
    case = synthetic(B, N, JR, JC, "accuracy", seed=60 + JC)
    b2 = np.random.RandomState(2).randn(B, 2, N)
    plan = wide_plan(case, JR, JC)
    try:
        ll, ld, q, st = plan.log_likelihood(materialize=True)
        assert (st == 0).all()
        osa = plan.one_step_ahead()
        osa2 = plan.one_step_ahead(b2)
    finally:
        plan.close()
    tag = "one_step_ahead on a wide plan (width %d)" % (JR + 2 * JC)
    check_innovations(tag, case, osa, bar=WIDE_SOLVE)
    check_innovations(tag + ", two rhs", case, osa2, rhs=b2, bar=WIDE_SOLVE)
    within(tag + ": sum z^2 / D vs the plan's quadratic form (relative)", np.max(np.abs(np.sum(osa.innovation ** 2 / osa.variance, axis=1) - q) / np.abs(q)), 1e-10)


def test_wide_plans_refuse_what_they_do_not_cover():
    """N = 400 on a wide plan: ``one_step_ahead`` is refused like ``solve``.  ``forecast`` on a wide plan is refused with a
    message that names the routes to take, after which ``predict`` still answers."""
    JR, JC, B = 1, 10, 2
    short = synthetic(B, 400, JR, JC, "bench", seed=14)
    plan = wide_plan(short, JR, JC)
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        with pytest.raises(RuntimeError, match=r"unsupported configuration.*N >= 512"):
            plan.one_step_ahead()
    finally:
        plan.close()
    case = synthetic(B, 2048, JR, JC, "bench", seed=15)
    xs = np.linspace(case["t"].min(), case["t"].max() * 1.05, 7)
    plan = wide_plan(case, JR, JC)
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        with pytest.raises(RuntimeError, match=r"unsupported configuration.*clr_batch_predict / clr_batch_predict_var\b"):
            plan.forecast(xs, return_var=True)
        pred = plan.predict(xs)
    finally:
        plan.close()
    for p in range(B):
        want = oracle_solver(case, p).predict(case["y"][p], xs)
        within("wide plan after forecast's refusal: predict vs oracle, of the largest", np.max(np.abs(pred[p] - want)) / np.max(np.abs(want)), PREDICT, p)


# ---------------------------------------------------------------------------------------------------------------------
# 10. sharded
# ---------------------------------------------------------------------------------------------------------------------

def test_sharded_filter_equals_the_unsharded_plan():
    """B = 5 over 1 / 2 / 3 shards on the visible devices: every shard on its slice, no collective -- the same bits as the
    unsharded plan, for shared, per-problem unsorted points and three right-hand sides."""
    JR, JC, B, N = 2, 3, 5, 600
    case = synthetic(B, N, JR, JC, "bench", seed=34)
    rng = np.random.RandomState(6)
    lo, hi = case["t"].min(), case["t"].max()
    shared = np.sort(rng.uniform(lo - 0.05, hi + 0.05, 9))
    own = rng.uniform(lo - 0.05, hi + 0.05, (B, 9))          # (unsorted)
    b3 = rng.randn(B, 3, N)

    def run(q):
        a, b = q.one_step_ahead(), q.one_step_ahead(b3)
        return (a.innovation, a.variance, a.status, b.innovation, b.variance) + q.forecast(own, return_var=True) + \
               q.forecast(shared, return_var=True) + (q.forecast(own),)

    plan = narrow_plan(case, JR, JC, None, chunks=16, expect=None)
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        want = run(plan)
    finally:
        plan.close()
    ndev = batch.device_count()
    for S in (1, 2, 3):
        sp = narrow_plan(case, JR, JC, None, chunks=16, expect=None, cls=batch.ShardedBatchedGP, devices=[s % ndev for s in range(S)])
        try:
            assert (sp.materialize()[3] == 0).all()
            got = run(sp)
        finally:
            sp.close()
        for g, w in zip(got, want):
            assert np.array_equal(g, w), S
    check_forecast("sharded filter, the unsharded plan", case, own, want[5], want[6])


# ---------------------------------------------------------------------------------------------------------------------
# 11. refusals and statuses
# ---------------------------------------------------------------------------------------------------------------------

def test_filter_refusals_leave_the_outputs_untouched_and_the_plan_usable():
    """Without a materialising run both entries fail with ``clr_batch_solve``'s message and write nothing; ``b == NULL``
    with ``nrhs = 2`` and all-NULL outputs are CLR_INVALID_ARGUMENT; M = 0 returns OK."""
    JR, JC, B, N = 2, 3, 2, 700
    case = synthetic(B, N, JR, JC, "bench", seed=16)
    xs = np.ascontiguousarray(case["t"][0, ::50])
    M = len(xs)
    z, D, st = np.full((B, N), -1.0), np.full((B, N), -1.0), np.full(B, -7, dtype=np.int32)
    mean, var = np.full((B, M), -1.0), np.full((B, M), -1.0)
    lib = batch._load()
    lib.clr_batch_solve.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    scratch = np.empty((B, 2, N))
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        assert (plan.log_likelihood()[3] == 0).all()         # (an evaluation, not a materialising one)
        said = {}
        calls = {"solve": lambda: lib.clr_batch_solve(plan._h, 1, None, batch._ptr(z)),
                 "one_step_ahead": lambda: lib.clr_batch_one_step_ahead(plan._h, 1, None, batch._ptr(z), batch._ptr(D), st.ctypes.data_as(_ip)),
                 "forecast": lambda: lib.clr_batch_forecast(plan._h, M, batch._ptr(xs), 0, batch._ptr(mean), batch._ptr(var))}
        for name, call in calls.items():
            with pytest.raises(RuntimeError) as err:
                batch._check(call())
            said[name] = str(err.value)
        assert said["one_step_ahead"] == said["solve"] == said["forecast"] and "materialising" in said["solve"]
        assert (z == -1.0).all() and (D == -1.0).all() and (st == -7).all() and (mean == -1.0).all() and (var == -1.0).all()
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()      # ... and the plan stays usable
        with pytest.raises(RuntimeError, match="invalid argument"):
            batch._check(lib.clr_batch_one_step_ahead(plan._h, 2, None, batch._ptr(scratch), None, None))
        with pytest.raises(RuntimeError, match="invalid argument"):
            batch._check(lib.clr_batch_one_step_ahead(plan._h, 1, None, None, None, None))
        with pytest.raises(RuntimeError, match="invalid argument"):
            batch._check(lib.clr_batch_forecast(plan._h, M, batch._ptr(xs), 0, None, None))
        batch._check(lib.clr_batch_forecast(plan._h, 0, None, 0, batch._ptr(mean), batch._ptr(var)))
        assert (mean == -1.0).all() and (var == -1.0).all()
        batch._check(lib.clr_batch_one_step_ahead(plan._h, 1, None, None, None, st.ctypes.data_as(_ip)))      # (statuses alone)
        assert (st == 0).all()
        batch._check(lib.clr_batch_one_step_ahead(plan._h, 1, None, None, batch._ptr(D), None))               # (D alone)
        batch._check(lib.clr_batch_forecast(plan._h, M, batch._ptr(xs), 0, None, batch._ptr(var)))            # (var alone)
        osa = plan.one_step_ahead()
        got = plan.forecast(xs, return_var=True)
    finally:
        plan.close()
    assert np.array_equal(D, osa.variance) and np.array_equal(var, got[1])
    check_innovations("one_step_ahead after the refusals", case, osa)
    check_forecast("forecast after the refusals", case, xs, *got)


def test_filter_beside_a_refused_problem():
    """One problem in the middle is not positive definite (status 2): NaN rows and its status for that problem, the
    others untouched and correct; a NaN point gives NaN and sorts last."""
    JR, JC, B, N = 2, 3, 5, 700
    case = synthetic(B, N, JR, JC, "bench", seed=1000 + 3 * JR + JC)
    mid = B // 2
    case["a_real"][mid] *= -40.0
    shared, own, perm = edge_points(case, np.random.RandomState(2))
    xs = np.concatenate([shared[:3], [np.nan], shared[3:]])
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        st = plan.log_likelihood(materialize=True)[3]
        osa = plan.one_step_ahead()
        mean, var = plan.forecast(xs, return_var=True)
    finally:
        plan.close()
    s0 = ref.batch_log_likelihood(0.0, *coeffs_of(case), case["t"], case["diag"], case["y"])[3]
    assert np.array_equal(st, s0) and st[mid] == 2 and (np.delete(st, mid) == 0).all() and np.array_equal(osa.status, s0)
    assert np.isnan(osa.innovation[mid]).all() and np.isnan(osa.variance[mid]).all()
    assert np.isnan(mean[mid]).all() and np.isnan(var[mid]).all()
    assert np.isnan(mean[:, 3]).all() and np.isnan(var[:, 3]).all()
    keep = np.arange(len(xs)) != 3
    assert np.isfinite(np.delete(mean[:, keep], mid, axis=0)).all() and np.isfinite(np.delete(var[:, keep], mid, axis=0)).all()
    check_innovations("one_step_ahead beside a refused problem", case, osa, skip=(mid,))
    check_forecast("forecast beside a refused problem", case, shared, mean[:, keep], var[:, keep], skip=(mid,))
