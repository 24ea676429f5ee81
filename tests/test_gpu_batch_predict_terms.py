# -*- coding: utf-8 -*-
"""`-m gpu`: component separation on batched plans -- ``BatchedGP.predict_terms``, ``clr_batch_predict_terms`` -- at
every narrow kernel shape in both factor layouts, at the edges of the merge of points and samples, across tile sizes,
beside ``predict`` and the recurrence variance, under a constant and a linear mean, across reuse of the factor-only state,
past 65 535 problems, sharded, and where it refuses.

The oracle per problem, group and point: ``k_g*^T alpha`` and ``k_g(0) - sum k_g* o RefSolver.solve(k_g*)`` with
``alpha = RefSolver.solve(r)`` and ``k_g`` from ``oracle.dense.kernel_value`` on the coefficients with the amplitudes
outside the group zeroed.

Bars: the mean ``PREDICT = 1e-10`` of the largest |mean| over the groups of the problem; the variance 1e-10 k(0) of the
FULL kernel, the recurrence variance's bar (the error terms scale with S+ and Q, not with the group).  The masked
recurrences themselves are pinned in NumPy by tests/test_predict_terms_cpu.py.

Largest deviations seen (MI355X): all 24 shapes, both layouts, N = 130 and 1000 -- the mean 1.2e-13 of the largest |mean|,
the variance 9.5e-14 k(0); the edges of the merge, M = 1, all points before / beyond 4.3e-14 and 3.2e-14; under a
constant and a linear mean 1.1e-14 and 1.2e-14; B = 65537 2.5e-15 and 2.0e-14.  The all group against ``predict`` 1.5e-15
of the largest entry and against the recurrence variance 3.9e-16 k(0); the single terms' means against the all group's
4.2e-16; terms + (diag + jitter) alpha against the residual 3.0e-15.  Library trig at t ~ 3e8: the variance 1.2e-8 k(0)
(the phase rounding, as the recurrence variance's 1.0e-8), the mean 4.7e-11 of k(0) sum|alpha|; lean against the stored
layout 0.  Tiles, shared against per-problem points, unsorted input, 2 and 3 shards and every order of calls: the same
bits."""
import ctypes as C

import numpy as np
import pytest

from celerite_amd import batch
from oracle import dense, ref
from _cases import ALL_WIDTH_SHAPES, general_terms, synthetic, coeffs_of, within

pytestmark = pytest.mark.gpu

PREDICT = 1e-10
NOGEN = (np.empty(0), np.empty((0, 0)), np.empty((0, 0)))
# At t ~ 3e8 the phase d t rounded to double is off by up to half an ulp of 1.5e9 (1.2e-7 rad).  The kernels evaluate the
# features of a point at its ABSOLUTE phase d x and those of a sample at d t_n, so the phase difference between a point
# and a sample carries both roundings, up to 2.4e-7 rad; the oracle forms k_g* from the RELATIVE phase d (x - t_n), which
# carries neither.  Every entry of k_g* is then off by that order times k(0): the variance by that times k(0)
# (tests/test_gpu_batch_predict_var_recurrence.py: PHASE_ROUNDING, the same bar), the mean k_g*^T alpha by that times
# k(0) sum_n |alpha_n|.  A property of such inputs.
PHASE_ROUNDING = 1e-6


def k_zero(case, p):
    return float(np.sum(case["a_real"][p]) + np.sum(case["a_comp"][p]))


def group_sets(JR, JC):
    """(G, T) 0/1: the T single terms, one mixed group (the first and the last term), all, empty."""
    T = JR + JC
    g = np.zeros((T + 3, T), dtype=bool)
    g[:T] = np.eye(T, dtype=bool)
    g[T, [0, T - 1]] = True
    g[T + 1] = True
    return g


def points_of(pts, p):
    return pts[p] if pts.ndim == 2 else pts


def oracle_terms(case, p, x, groups, resid=None):
    """(mean[G, M], var[G, M], alpha[N]) of problem p at its points x."""
    ar, cr, ac, bc, cc, dc = coeffs_of(case, p)
    JR = len(ar)
    r = ref.RefSolver()
    r.compute(0.0, ar, cr, ac, bc, cc, dc, *NOGEN, case["t"][p], case["diag"][p])
    y = case["y"][p] if resid is None else resid[p]
    alpha = np.asarray(r.solve(y[:, None]))[:, 0]
    mean, var = np.empty((len(groups), len(x))), np.empty((len(groups), len(x)))
    for q, g in enumerate(groups):
        masked = (np.where(g[:JR], ar, 0.0), cr, np.where(g[JR:], ac, 0.0), np.where(g[JR:], bc, 0.0), cc, dc)
        kstar = dense.kernel_value(*masked, x[None, :] - case["t"][p][:, None])          # (N, M)
        mean[q] = kstar.T @ alpha
        var[q] = float(np.sum(masked[0]) + np.sum(masked[2])) - np.sum(kstar * r.solve(kstar), axis=0)
    return mean, var, alpha


def check_against_oracle(tag, case, pts, groups, mean, var, resid=None, bar=PREDICT, phase=False):
    B = case["t"].shape[0]
    G, M = len(groups), pts.shape[-1]
    worst_m = worst_v = 0.0
    for p in range(B):
        want_m, want_v, alpha = oracle_terms(case, p, points_of(pts, p), groups, resid)
        k0 = k_zero(case, p)
        if mean is not None:
            assert mean.shape == (B, G, M)
            scale = k0 * np.sum(np.abs(alpha)) if phase else np.max(np.abs(want_m))
            dev = np.max(np.abs(mean[p] - want_m)) / scale
            worst_m = max(worst_m, dev) if dev == dev else float("nan")
            within(tag + (": mean vs oracle, of k(0) sum|alpha|" if phase else ": mean vs oracle, of the largest |mean|"), dev, bar, p)
        if var is not None:
            assert var.shape == (B, G, M)
            dev = np.max(np.abs(var[p] - want_v)) / k0
            worst_v = max(worst_v, dev) if dev == dev else float("nan")
            within(tag + ": var vs oracle, of k(0)", dev, bar, p)
    print("%s: max |mean - oracle| / scale = %.3e   max |var - oracle| / k(0) = %.3e" % (tag, worst_m, worst_v))


def prediction_points(case, rng, M_random=24, M_own=20):
    """Shared points reaching 5 % past both ends with some exact data times and two duplicates, per-problem points, and
    an unsorted permutation of the shared ones."""
    B, N = case["t"].shape
    lo, hi = case["t"].min(), case["t"].max()
    pad = 0.05 * (hi - lo)
    rnd = rng.uniform(lo - pad, hi + pad, M_random)
    shared = np.sort(np.concatenate([rnd, rnd[:2], [lo - pad, hi + pad], case["t"][0, ::max(1, N // 9)]]))
    own = np.sort(rng.uniform(lo - pad, hi + pad, (B, M_own)), axis=1)
    perm = rng.permutation(len(shared))
    assert shared[0] < lo and shared[-1] > hi and np.any(np.diff(shared[perm]) < 0) and np.any(np.diff(shared) == 0)
    return shared, own, perm


NARROW_B = 4


def narrow_plan(case, JR, JC, layout, chunks=24, cls=batch.BatchedGP, **kw):
    B, N = case["t"].shape
    plan = cls(B, N, JR, JC, **kw)
    plan.set_chunks(chunks)
    if layout:
        plan.set_factor_layout(layout)
    plan.set_series(case["t"], case["diag"], case["y"])
    plan.set_coefficients(*coeffs_of(case))
    return plan


def materialise(plan):
    st = plan.materialize()[3] if isinstance(plan, batch.ShardedBatchedGP) else plan.log_likelihood(materialize=True)[3]
    assert (st == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 1. every narrow shape, both factor layouts
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["reference", "lean"])
@pytest.mark.parametrize("JR,JC", ALL_WIDTH_SHAPES)
def test_terms_at_every_narrow_shape(JR, JC, layout):
    """The kernels are compiled per (J_real, J_comp), factor layout and trig flavour (``bterms_*`` in
    csrc/clr_bterms_kernels.h): all 24 shapes, both layouts.  N = 130: two chunks of 72, the last one of 58; N = 1000: 21
    chunks of 48, the last one of 40.  The T single terms, a mixed pair, all and the empty group at shared sorted points
    (random, the plan's own sample times, before the first sample, beyond the last, duplicates), per-problem points, and
    an unsorted permutation of the shared ones, which must give the sorted result permuted, bit for bit."""
    groups = group_sets(JR, JC)
    for N, chunks, expect, family in ((130, 2, (2, 72), "accuracy"), (1000, 24, (21, 48), "bench")):
        case = synthetic(NARROW_B, N, JR, JC, family, seed=600 + 9 * JC + JR)
        shared, own, perm = prediction_points(case, np.random.RandomState(40 + JR + 7 * JC))
        plan = narrow_plan(case, JR, JC, layout, chunks=chunks)
        try:
            assert plan.chunks == expect and N % expect[1] != 0      # a ragged last chunk
            materialise(plan)
            mean, var = plan.predict_terms(shared, groups, return_var=True)
            mean_own, var_own = plan.predict_terms(own, groups, return_var=True)
            mean_perm, var_perm = plan.predict_terms(shared[perm], groups, return_var=True)
            mean_only = plan.predict_terms(shared, groups)
            singles = plan.predict_terms(shared)                       # groups=None: one group per term
        finally:
            plan.close()
        tag = "predict_terms (%s layout, N = %d)" % (layout, N)
        assert np.array_equal(mean_perm, mean[:, :, perm]) and np.array_equal(var_perm, var[:, :, perm]), tag
        assert np.array_equal(mean_only, mean) and np.array_equal(singles, mean[:, :JR + JC]), tag
        assert np.all(mean[:, -1] == 0.0) and np.all(var[:, -1] == 0.0), tag
        check_against_oracle(tag + ", shared points", case, shared, groups, mean, var)
        check_against_oracle(tag + ", per-problem points", case, own, groups, mean_own, var_own)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the edges of the merge of points and samples
# ---------------------------------------------------------------------------------------------------------------------

def test_terms_at_the_edges_of_the_merge():
    """(2, 3) lean, N = 700: 22 chunks of 32, the last one of 28.  Per problem, points exactly at t_0 and t_{N-1}, at the
    first and the last sample of an interior chunk (5: samples 160 and 191), at the midpoint of the gap between chunks 5
    and 6, just outside both ends, and a run of 5 inside one gap; then M = 1, all points before the series and all
    beyond it."""
    JR, JC, B, N, L = 2, 3, NARROW_B, 700, 32
    groups = group_sets(JR, JC)
    for family in ("bench", "accuracy"):
        case = synthetic(B, N, JR, JC, family, seed=77)
        t = case["t"]
        delta = 0.37 * np.min(np.diff(t, axis=1), axis=1)
        names = ["t_0 - delta", "t_0", "chunk 5 first", "chunk 5 last", "between chunks 5 and 6"] + ["run in gap 300|301"] * 5 + \
                ["t_N-1", "t_N-1 + delta"]
        pts = np.stack([np.concatenate([[t[p, 0] - delta[p], t[p, 0], t[p, 5 * L], t[p, 6 * L - 1], 0.5 * (t[p, 6 * L - 1] + t[p, 6 * L])],
                                        t[p, 300] + (t[p, 301] - t[p, 300]) * np.array([0.1, 0.3, 0.5, 0.7, 0.9]),
                                        [t[p, N - 1], t[p, N - 1] + delta[p]]]) for p in range(B)])
        assert pts.shape == (B, len(names)) and (np.diff(pts, axis=1) > 0).all()
        span = t.max() - t.min()
        before = t.min() - span * np.array([0.3, 0.2, 0.1])
        beyond = t.max() + span * np.array([0.1, 0.2, 0.3])
        one = np.array([0.5 * (t[0, 400] + t[0, 401])])
        plan = narrow_plan(case, JR, JC, "lean")
        try:
            assert plan.chunks == (22, 32)
            materialise(plan)
            got = plan.predict_terms(pts, groups, return_var=True)
            got_before = plan.predict_terms(before, groups, return_var=True)
            got_beyond = plan.predict_terms(beyond, groups, return_var=True)
            got_one = plan.predict_terms(one, groups, return_var=True)
        finally:
            plan.close()
        for p in range(B):
            want_m, want_v, _ = oracle_terms(case, p, pts[p], groups)
            for m, name in enumerate(names):
                within("predict_terms at the edges: %s, mean of the largest |mean|" % name,
                       np.max(np.abs(got[0][p, :, m] - want_m[:, m])) / np.max(np.abs(want_m)), PREDICT, (family, p))
                within("predict_terms at the edges: %s, var of k(0)" % name,
                       np.max(np.abs(got[1][p, :, m] - want_v[:, m])) / k_zero(case, p), PREDICT, (family, p))
        check_against_oracle("predict_terms, all points before the series (%s)" % family, case, before, groups, *got_before)
        check_against_oracle("predict_terms, all points beyond the series (%s)" % family, case, beyond, groups, *got_beyond)
        check_against_oracle("predict_terms, M = 1 (%s)" % family, case, one, groups, *got_one)


@pytest.mark.parametrize("JR,JC", [(2, 3), (1, 1)])
def test_terms_on_the_library_trig_kernels(JR, JC):
    """A series offset to t ~ 3e8: max|d| max|t| >= CLR_FAST_TRIG_LIMIT, so the mean replays and the lean variance replays
    take the library sincos and the points' features take it too.  Against the oracle under PHASE_ROUNDING (see there),
    and the lean layout's variances against the reference layout's (stored phi, u) within 1e-12 k(0)."""
    B, N = NARROW_B, 700
    groups = group_sets(JR, JC)
    case = synthetic(B, N, JR, JC, "accuracy", seed=77 + JR)
    case["t"] = case["t"] + 3.0e8
    shared, own, perm = prediction_points(case, np.random.RandomState(91))
    out = {}
    for layout in ("lean", "reference"):
        plan = narrow_plan(case, JR, JC, layout)
        try:
            bounds = plan.selection_bounds()
            assert bounds["dmax"] * bounds["tmax"] >= 1.0e9, bounds        # CLR_FAST_TRIG_LIMIT (csrc/clr_core.h)
            materialise(plan)
            out[layout] = plan.predict_terms(shared, groups, return_var=True)
        finally:
            plan.close()
        check_against_oracle("predict_terms, library trig (%s layout)" % layout, case, shared, groups, *out[layout],
                             bar=PHASE_ROUNDING, phase=True)
    for p in range(B):
        within("predict_terms, library trig: lean vs reference layout, var of k(0)",
               np.max(np.abs(out["lean"][1][p] - out["reference"][1][p])) / k_zero(case, p), 1e-12, p)


# ---------------------------------------------------------------------------------------------------------------------
# 3. tiles, shared against per-problem points, unsorted input
# ---------------------------------------------------------------------------------------------------------------------

def test_terms_do_not_depend_on_the_tile_or_on_how_the_points_are_given():
    """Tiles of 1, of 7 (M = 40: a ragged last tile) and the automatic tile give the same bits; so do shared ``(M,)``
    points and the same points as ``(B, M)``; unsorted input gives the sorted result permuted."""
    JR, JC, B, N, M = 2, 3, 3, 2048, 40
    groups = group_sets(JR, JC)
    case = synthetic(B, N, JR, JC, "accuracy", seed=24)
    rng = np.random.RandomState(3)
    xs = np.sort(rng.uniform(case["t"].min() - 10.0, case["t"].max() + 10.0, M))
    perm = rng.permutation(M)
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_factor_layout("lean")
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        materialise(plan)
        got = {}
        for tile in (1, 7, 0):
            plan.set_predict_tile(tile)
            got[tile] = plan.predict_terms(xs, groups, return_var=True)
            got[tile, "mean"] = plan.predict_terms(xs, groups)
        tiled = plan.predict_terms(np.tile(xs, (B, 1)), groups, return_var=True)
        plan.set_predict_tile(7)
        unsorted = plan.predict_terms(xs[perm], groups, return_var=True)
        own_unsorted = plan.predict_terms(np.stack([xs[np.roll(perm, p)] for p in range(B)]), groups, return_var=True)
    finally:
        plan.close()
    for tile in (1, 7):
        assert np.array_equal(got[tile][0], got[0][0]) and np.array_equal(got[tile][1], got[0][1]), tile
        assert np.array_equal(got[tile, "mean"], got[0][0]), tile
    assert np.array_equal(got[0, "mean"], got[0][0])
    for k in range(2):
        assert np.array_equal(tiled[k], got[0][k])
        assert np.array_equal(unsorted[k], got[0][k][:, :, perm])
        for p in range(B):
            assert np.array_equal(own_unsorted[k][p], got[0][k][p][:, np.roll(perm, p)])
    check_against_oracle("predict_terms across tiles (width %d)" % (JR + 2 * JC), case, xs, groups, *got[0])


# ---------------------------------------------------------------------------------------------------------------------
# 4. identities without the oracle
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC,layout", [(2, 3, "lean"), (4, 2, "reference"), (1, 0, "lean")])
def test_the_identities(JR, JC, layout):
    """The all group is ``predict(xs)`` (route against route, 2e-10 of the largest entry) and its ``method="recurrence"``
    variance (2e-10 k(0)); the empty group is exactly 0; the single terms' means add up to the all group's (1e-12 of the
    largest); at ``xs = t`` the terms' means plus ``(diag + jitter) o solve()`` give back the residual (1e-10 of its
    largest entry)."""
    B, N, T = NARROW_B, 700, JR + JC
    groups = group_sets(JR, JC)
    jitter = 0.01
    for family in ("bench", "accuracy"):
        case = synthetic(B, N, JR, JC, family, seed=90 + JR)
        shared, own, perm = prediction_points(case, np.random.RandomState(8))
        plan = narrow_plan(case, JR, JC, layout)
        try:
            plan.set_coefficients(*coeffs_of(case), jitter=jitter)
            materialise(plan)
            mean, var = plan.predict_terms(own, groups, return_var=True)
            pred, pvar = plan.predict(own, return_var=True, method="recurrence")
            at_t = plan.predict_terms(case["t"])
            alpha = plan.solve()
        finally:
            plan.close()
        assert np.all(mean[:, T + 2] == 0.0) and np.all(var[:, T + 2] == 0.0)
        for p in range(B):
            ctx = (JR, JC, family, p)
            within("predict_terms: all group vs predict, of the largest entry",
                   np.max(np.abs(mean[p, T + 1] - pred[p])) / np.max(np.abs(pred[p])), 2 * PREDICT, ctx)
            within("predict_terms: all group vs the recurrence variance, of k(0)",
                   np.max(np.abs(var[p, T + 1] - pvar[p])) / k_zero(case, p), 2 * PREDICT, ctx)
            within("predict_terms: sum of the single terms' means vs the all group, of the largest",
                   np.max(np.abs(mean[p, :T].sum(axis=0) - mean[p, T + 1])) / np.max(np.abs(mean[p, T + 1])), 1e-12, ctx)
            back = at_t[p].sum(axis=0) + (case["diag"][p] + jitter) * alpha[p]
            within("predict_terms at xs = t: terms + (diag + jitter) alpha vs the residual, of its largest entry",
                   np.max(np.abs(back - case["y"][p])) / np.max(np.abs(case["y"][p])), PREDICT, ctx)


# ---------------------------------------------------------------------------------------------------------------------
# 5. a mean in force: the residual is what is decomposed, and nothing is added
# ---------------------------------------------------------------------------------------------------------------------

def test_terms_decompose_the_residual_under_a_constant_and_a_linear_mean():
    JR, JC, B, N = 2, 3, NARROW_B, 700
    groups = group_sets(JR, JC)
    T = JR + JC
    case = synthetic(B, N, JR, JC, "accuracy", seed=31)
    shared, own, perm = prediction_points(case, np.random.RandomState(9))
    rng = np.random.RandomState(10)
    mu = rng.uniform(-2.0, 2.0, B)
    tn = (case["t"] - case["t"].min()) / (case["t"].max() - case["t"].min())
    Phi = np.stack([np.ones_like(tn), tn], axis=1)                       # (B, K = 2, N)
    w = rng.uniform(-1.0, 1.0, (B, 2))
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        plan.set_mean(mu)
        materialise(plan)
        const = plan.predict_terms(own, groups, return_var=True)
        const_pred = plan.predict(own)
        plan.set_mean(None)
        plan.set_mean_basis(Phi)
        plan.set_mean_weights(w)
        materialise(plan)
        linear = plan.predict_terms(own, groups, return_var=True)
    finally:
        plan.close()
    check_against_oracle("predict_terms under a constant mean", case, own, groups, *const, resid=case["y"] - mu[:, None])
    check_against_oracle("predict_terms under a linear mean", case, own, groups, *linear,
                         resid=case["y"] - np.einsum("bk,bkn->bn", w, Phi))
    for p in range(B):
        within("predict_terms under a constant mean: all group vs predict less the mean, of the largest entry",
               np.max(np.abs(const[0][p, T + 1] - (const_pred[p] - mu[p]))) / np.max(np.abs(const_pred[p] - mu[p])), 2 * PREDICT, p)
    assert np.array_equal(const[1], linear[1])                           # (the variances do not see the data)


# ---------------------------------------------------------------------------------------------------------------------
# 6. reuse and renewal of the factor-only state
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["lean", "reference"])
def test_terms_reuse_and_renew_the_factor_state(layout):
    """The start states of S and Q are shared with the recurrence variance and ``leave_one_out``: calls after either, after
    ``solve()`` and repeated calls return the bits of a fresh plan's first call; a mean-only call neither forms nor
    invalidates them (the recurrence variance and the leave-one-out diagonal after it are those of a plan that never made
    one); after new coefficients and a new materialising run the new factor's results."""
    JR, JC, B, N = 2, 3, NARROW_B, 700
    groups = group_sets(JR, JC)
    case = synthetic(B, N, JR, JC, "bench", seed=12)
    other = synthetic(B, N, JR, JC, "bench", seed=13)
    other["t"], other["diag"], other["y"] = case["t"], case["diag"], case["y"]
    shared, own, perm = prediction_points(case, np.random.RandomState(5))
    REC = dict(return_var=True, method="recurrence")
    plans = [narrow_plan(case, JR, JC, layout) for _ in range(4)]
    plan, after_loo, after_rec, plain = plans
    try:
        for q in plans:
            materialise(q)
        first = plan.predict_terms(own, groups, return_var=True)
        second = plan.predict_terms(own, groups, return_var=True)
        x = plan.solve()
        third = plan.predict_terms(own, groups, return_var=True)
        loo = after_loo.leave_one_out()
        late_loo = after_loo.predict_terms(own, groups, return_var=True)
        rec = after_rec.predict(own, **REC)[1]
        late_rec = after_rec.predict_terms(own, groups, return_var=True)
        # a mean-only call first, then the consumers of S and Q
        mean_only = plain.predict_terms(own, groups)
        rec_plain = plain.predict(own, **REC)[1]
        mean_again = plain.predict_terms(own, groups)
        loo_plain = plain.leave_one_out()
        rec_after = plan.predict(own, **REC)[1]
        loo_after = plan.leave_one_out()
        plan.set_coefficients(*coeffs_of(other))
        materialise(plan)
        renewed = plan.predict_terms(own, groups, return_var=True)
    finally:
        for q in plans:
            q.close()
    for got in (second, third, late_loo, late_rec):
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
    assert np.array_equal(mean_only, first[0]) and np.array_equal(mean_again, first[0])
    assert np.array_equal(rec_plain, rec) and np.array_equal(rec_after, rec)
    assert np.array_equal(loo_plain.kinv_diag, loo.kinv_diag) and np.array_equal(loo_after.kinv_diag, loo.kinv_diag)
    assert np.isfinite(x).all() and not np.array_equal(renewed[1], first[1])
    check_against_oracle("predict_terms (%s layout), first factor" % layout, case, own, groups, *first)
    check_against_oracle("predict_terms (%s layout), after a new materialising run" % layout, other, own, groups, *renewed)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the batch-size limit of a grid axis
# ---------------------------------------------------------------------------------------------------------------------

def test_terms_past_65535_problems():
    """B = 65537 problems of width 1 ((1, 0), N = 128, 4 chunks), 64 distinct ones tiled over the batch: every problem
    equals its twin in a plan of the 64, bit for bit, and the 64 meet the oracle."""
    JR, JC, N, BIG, DISTINCT = 1, 0, 128, 65537, 64
    small = synthetic(DISTINCT, N, JR, JC, "bench", seed=7)
    idx = np.arange(BIG) % DISTINCT
    big = {k: v[idx] for k, v in small.items()}
    groups = np.array([[True], [False]])
    xs = np.array([small["t"].min() - 1e-3, small["t"][0, 40], 0.5 * (small["t"][0, 63] + small["t"][0, 64]), small["t"].max() + 1e-3])
    res = []
    for case in (big, small):
        plan = narrow_plan(case, JR, JC, "reference", chunks=4)
        try:
            materialise(plan)
            res.append(plan.predict_terms(xs, groups, return_var=True))
        finally:
            plan.close()
    assert res[0][0].shape == (BIG, 2, len(xs))
    for k in range(2):
        assert np.array_equal(res[0][k], res[1][k][idx])
    check_against_oracle("predict_terms, B = 65537 (width 1): the 64 distinct problems", small, xs, groups, *res[1])


# ---------------------------------------------------------------------------------------------------------------------
# 8. sharded
# ---------------------------------------------------------------------------------------------------------------------

def test_sharded_terms_equal_the_unsharded_plan():
    """B = 5 over 2 and 3 shards on the visible devices: every shard on its slice, no collective -- the same bits as the
    unsharded plan, for shared and for unsorted per-problem points, with and without the variance."""
    JR, JC, B, N = 2, 3, 5, 600
    groups = group_sets(JR, JC)
    case = synthetic(B, N, JR, JC, "bench", seed=34)
    shared, own, perm = prediction_points(case, np.random.RandomState(6), M_random=9, M_own=9)
    own = own[:, np.random.RandomState(7).permutation(own.shape[1])]          # (unsorted)
    plan = narrow_plan(case, JR, JC, None, chunks=16)
    try:
        materialise(plan)
        want = plan.predict_terms(own, groups, return_var=True), plan.predict_terms(shared, groups, return_var=True)
        want_mean = plan.predict_terms(shared)
    finally:
        plan.close()
    ndev = batch.device_count()
    for S in (2, 3):
        sp = narrow_plan(case, JR, JC, None, chunks=16, cls=batch.ShardedBatchedGP, devices=[s % ndev for s in range(S)])
        try:
            materialise(sp)
            got = sp.predict_terms(own, groups, return_var=True), sp.predict_terms(shared, groups, return_var=True)
            got_mean = sp.predict_terms(shared)
        finally:
            sp.close()
        for g, w in zip(got, want):
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), S
        assert np.array_equal(got_mean, want_mean), S
    check_against_oracle("sharded predict_terms, the unsharded plan", case, own, groups, *want[0])


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals: none writes a number or leaves the plan unusable
# ---------------------------------------------------------------------------------------------------------------------

def c_call(plan, xs, groups, mean, var):
    lib = batch._load()
    g = np.ascontiguousarray(groups, dtype=np.uint8)
    return lib.clr_batch_predict_terms(plan._h, len(xs), batch._ptr(xs), 0, len(g), g.ctypes.data_as(C.c_void_p),
                                       batch._ptr(mean), batch._ptr(var))


def test_terms_refuse_a_wide_plan():
    """(1, 10), N = 2048: CLR_UNSUPPORTED with a message that names ``clr_batch_predict``, which still answers."""
    JR, JC, B, N = 1, 10, 2, 2048
    case = synthetic(B, N, JR, JC, "bench", seed=15)
    xs = np.ascontiguousarray(case["t"][0, ::400])
    mean, var = np.full((B, 1, len(xs)), -1.0), np.full((B, 1, len(xs)), -1.0)
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        materialise(plan)
        with pytest.raises(RuntimeError, match=r"unsupported configuration.*clr_batch_predict\b"):
            batch._check(c_call(plan, xs, np.ones((1, JR + JC)), mean, var))
        with pytest.raises(RuntimeError, match=r"unsupported configuration.*clr_batch_predict\b"):
            plan.predict_terms(xs)
        assert (mean == -1.0).all() and (var == -1.0).all()
        pred = plan.predict(xs)
    finally:
        plan.close()
    assert np.isfinite(pred).all()


def test_terms_refuse_an_unchunked_plan():
    """N = 100: one chunk.  CLR_UNSUPPORTED naming ``clr_batch_predict``, which refuses such a plan as well (its solve is
    chunked); the plan still evaluates."""
    JR, JC, B, N = 2, 3, 2, 100
    case = synthetic(B, N, JR, JC, "bench", seed=17)
    xs = np.ascontiguousarray(case["t"][0, ::20])
    G = np.ones((1, JR + JC))
    mean, var = np.full((B, 1, len(xs)), -1.0), np.full((B, 1, len(xs)), -1.0)
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        materialise(plan)
        with pytest.raises(RuntimeError, match=r"unsupported configuration.*clr_batch_predict\b"):
            batch._check(c_call(plan, xs, G, mean, var))
        assert (mean == -1.0).all() and (var == -1.0).all()
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            plan.predict(xs)
        ll = plan.log_likelihood(materialize=True)
    finally:
        plan.close()
    assert (ll[3] == 0).all() and np.isfinite(ll[0]).all()


def test_terms_without_a_materialising_run_a_bad_group_byte_and_general_terms():
    JR, JC, B, N = 2, 3, 2, 700
    groups = group_sets(JR, JC)
    case = synthetic(B, N, JR, JC, "bench", seed=16)
    xs = np.ascontiguousarray(case["t"][0, ::50])
    G = np.ones((1, JR + JC))
    mean, var = np.full((B, 1, len(xs)), -1.0), np.full((B, 1, len(xs)), -1.0)
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        assert (plan.log_likelihood()[3] == 0).all()         # (an evaluation, not a materialising one)
        with pytest.raises(RuntimeError, match="materialising"):
            batch._check(c_call(plan, xs, G, mean, var))
        materialise(plan)
        bad = G.copy()
        bad[0, 2] = 2
        with pytest.raises(RuntimeError, match=r"invalid argument.*0 or 1"):
            batch._check(c_call(plan, xs, bad, mean, var))
        assert (mean == -1.0).all() and (var == -1.0).all()
        got = plan.predict_terms(xs, groups, return_var=True)   # ... and the plan stays usable
    finally:
        plan.close()
    check_against_oracle("predict_terms after the refusals", case, xs, groups, *got)
    # a general-terms plan (A, U, V): refused by the width check
    A, U, V = general_terms(case["t"][0], np.random.RandomState(3).rand)
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        plan.set_general(A, U, V)
        with pytest.raises(RuntimeError, match=r"unsupported configuration.*celerite-only"):
            batch._check(c_call(plan, xs, G, mean, var))
        assert (mean == -1.0).all() and (var == -1.0).all()
    finally:
        plan.close()
