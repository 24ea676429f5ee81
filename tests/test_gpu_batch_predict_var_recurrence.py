# -*- coding: utf-8 -*-
"""`-m gpu`: the conditional variance of ``GP.predict`` on batched plans by recurrence --
``BatchedGP.predict(xs, return_var=True, method="recurrence")``, ``clr_batch_predict_var_recurrence`` -- at every narrow
kernel shape in both factor layouts, at the edges of the merge of points and samples, across tile sizes, beside the solve
route, across reuse of the factor-only state, sharded, and where it refuses.

The oracle value per problem and point is the reference's own formula (celerite.py:465-470) on the oracle's factor:
``k(0) - sum k* o RefSolver.solve(k*)`` with ``k*`` from a NumPy evaluation of the kernel (the helpers are those of
tests/test_gpu_batch_predict_var.py, copied).

Bar: ``max |var_dev - var_oracle| <= 1e-10 k(0)`` -- the project's PREDICT bar; the two routes against each other
2e-10 k(0), two PREDICT bars.  The identity itself is pinned in NumPy by tests/test_predict_var_recurrence_cpu.py
(5.4e-15 k(0) there)."""
import ctypes as C

import numpy as np
import pytest

from celerite_amd import batch
from oracle import ref
from _cases import ALL_WIDTH_SHAPES, synthetic, coeffs_of, within

pytestmark = pytest.mark.gpu

PREDICT = 1e-10
NOGEN = (np.empty(0), np.empty((0, 0)), np.empty((0, 0)))
TRUTH_POINTS = 6        # points of problem 0 attributed against binary128: each one refactors in binary128 (20 ms at width 8)
REC = dict(return_var=True, method="recurrence")
# At t ~ 3e8 the phase d t rounded to double is off by up to half an ulp of 1.5e9 (1.2e-7 rad).  The recurrence route
# evaluates the features of a point at its ABSOLUTE phase d x, as the factor does at d t_n (and as the reference's own
# predict does), so the phase difference between a point and a sample carries both roundings, up to 2.4e-7 rad; the oracle
# value forms k* from the RELATIVE phase d (x - t_n), which carries neither.  The two differ by that order times k(0):
# a property of such inputs, held to the bar tests/test_gpu_batch_predict_var.py keeps for them (PHASE_ROUNDING there).
PHASE_ROUNDING = 1e-6


def kernel_value(case, p, tau):
    """k_p(tau) by the six-coefficient formula (terms.py: RealTerm / ComplexTerm get_value)."""
    ar, cr, ac, bc, cc, dc = coeffs_of(case, p)
    tau = np.abs(np.asarray(tau, dtype=float))[..., None]
    return np.sum(ar * np.exp(-cr * tau), axis=-1) + np.sum(np.exp(-cc * tau) * (ac * np.cos(dc * tau) + bc * np.sin(dc * tau)), axis=-1)


def k_zero(case, p):
    return float(np.sum(case["a_real"][p]) + np.sum(case["a_comp"][p]))


def oracle_solver(case, p):
    r = ref.RefSolver()
    r.compute(0.0, *coeffs_of(case, p), *NOGEN, case["t"][p], case["diag"][p])
    return r


def oracle_var(case, p, pts):
    """(var[M], k*[N, M]) of problem p at its points."""
    kstar = kernel_value(case, p, pts[None, :] - case["t"][p][:, None])
    return k_zero(case, p) - np.sum(kstar * oracle_solver(case, p).solve(kstar), axis=0), kstar


def points_of(pts, p):
    return pts[p] if pts.ndim == 2 else pts


def check_against_oracle(tag, case, pts, var, truth=False, bar=PREDICT):
    """Every problem against the oracle under ``bar``; ``truth``: device and oracle of problem 0 against binary128 at
    TRUTH_POINTS of its points, side by side under the same bar."""
    B = case["t"].shape[0]
    assert var.shape == (B, pts.shape[-1])
    worst = 0.0
    for p in range(B):
        x = points_of(pts, p)
        want, kstar = oracle_var(case, p, x)
        k0 = k_zero(case, p)
        dev = np.max(np.abs(var[p] - want)) / k0
        worst = max(worst, dev) if dev == dev else float("nan")
        within(tag + ": var vs oracle, of k(0)", dev, bar, p)
        if truth and p == 0:
            idx = np.unique(np.linspace(0, len(x) - 1, TRUTH_POINTS + 2).astype(int)[1:-1])   # (inside the series)
            vq = np.array([k0 - kstar[:, m] @ ref.quad_factor_solve(0.0, *coeffs_of(case, 0), case["t"][0], case["diag"][0],
                                                                     kstar[:, m], want_factor=False)[2] for m in idx])
            within(tag + ": device var vs binary128, of k(0)", np.max(np.abs(var[0][idx] - vq)) / k0, PREDICT)
            within(tag + ": double oracle var vs binary128, of k(0)", np.max(np.abs(want[idx] - vq)) / k0, PREDICT)
    print("%s: max |var - oracle| / k(0) = %.3e" % (tag, worst))


def prediction_points(case, rng, M_random=30, M_own=30):
    """About 40 shared points reaching 5 % past both ends with some exact data times, per-problem points, and an
    unsorted permutation of the shared ones."""
    B = case["t"].shape[0]
    lo, hi = case["t"].min(), case["t"].max()
    pad = 0.05 * (hi - lo)
    shared = np.sort(np.concatenate([rng.uniform(lo - pad, hi + pad, M_random), [lo - pad, hi + pad], case["t"][0, ::97]]))
    own = np.sort(rng.uniform(lo - pad, hi + pad, (B, M_own)), axis=1)
    perm = rng.permutation(len(shared))
    assert shared[0] < lo and shared[-1] > hi and np.any(np.diff(shared[perm]) < 0)
    return shared, own, perm


NARROW_B, NARROW_N, NARROW_CHUNKS = 4, 700, (22, 32)    # set_chunks(24): chunks of 32 samples, the last one 28


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
def test_recurrence_at_every_narrow_shape(JR, JC, layout):
    """The kernels are compiled per (J_real, J_comp), factor layout and trig flavour (``bpvrec_*`` in
    csrc/clr_bpredvar_rec_kernels.h, instantiated through csrc/clr_batch_kernels.h): all 24 shapes, both layouts, both
    families, 22 chunks with a ragged last one of 28.  Shared sorted points, per-problem points, and an unsorted
    permutation of the shared ones, which must give the sorted result permuted, bit for bit."""
    B, N = NARROW_B, NARROW_N
    for family in ("bench", "accuracy"):
        case = synthetic(B, N, JR, JC, family, seed=500 + 9 * JC + JR)
        shared, own, perm = prediction_points(case, np.random.RandomState(40 + JR + 7 * JC))
        plan = narrow_plan(case, JR, JC, layout)
        try:
            assert plan.chunks == (22, 32) and N - 21 * 32 == 28
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            var = plan.predict(shared, **REC)[1]
            var_own = plan.predict(own, **REC)[1]
            var_perm = plan.predict(shared[perm], **REC)[1]
        finally:
            plan.close()
        tag = "predict_var by recurrence (%s layout, %s family)" % (layout, family)
        assert np.array_equal(var_perm, var[:, perm]), tag
        check_against_oracle(tag + ", shared points", case, shared, var, truth=family == "accuracy")
        check_against_oracle(tag + ", per-problem points", case, own, var_own)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the edges of the merge of points and samples
# ---------------------------------------------------------------------------------------------------------------------

def test_recurrence_at_the_edges_of_the_merge():
    """(2, 3) lean, 22 chunks of 32.  Per problem, points exactly at t_0 and t_{N-1}, at the first and the last sample of
    an interior chunk (5: samples 160 and 191), at the midpoint of the gap between chunks 5 and 6, just outside both
    ends, and a run of 5 inside one gap (300 | 301); chunks 1..4, 6..8 and 10..20 own no point at all."""
    JR, JC, B, N, L = 2, 3, NARROW_B, NARROW_N, 32
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
        for p in range(B):
            owner = np.clip((np.searchsorted(t[p], pts[p], side="right") - 1) // L, 0, None)
            assert sorted(set(owner)) == [0, 5, 9, 21]
        plan = narrow_plan(case, JR, JC, "lean")
        try:
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            var = plan.predict(pts, **REC)[1]
        finally:
            plan.close()
        for p in range(B):
            want = oracle_var(case, p, pts[p])[0]
            for m, name in enumerate(names):
                dev = abs(var[p, m] - want[m]) / k_zero(case, p)
                print("edges (%s family), problem %d, %-24s |var - oracle| / k(0) = %.3e" % (family, p, name, dev))
                within("predict_var by recurrence at the edges: %s, of k(0)" % name, dev, PREDICT, (family, p))


# ---------------------------------------------------------------------------------------------------------------------
# 3. tiles
# ---------------------------------------------------------------------------------------------------------------------

def test_recurrence_does_not_depend_on_the_tile():
    """Tiles of 1, of 7 (M = 40: a ragged last tile) and the automatic tile give the same bits; the mean is what
    ``predict(xs)`` returns, before and after."""
    JR, JC, B, N, M = 2, 3, 3, 2048, 40
    case = synthetic(B, N, JR, JC, "accuracy", seed=24)
    xs = np.sort(np.random.RandomState(3).uniform(case["t"].min() - 10.0, case["t"].max() + 10.0, M))
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_factor_layout("lean")
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        before = plan.predict(xs)
        got = {}
        for tile in (1, 7, 0):
            plan.set_predict_tile(tile)
            got[tile] = plan.predict(xs, **REC)
        after = plan.predict(xs, method="recurrence")      # (accepted and ignored for the mean)
    finally:
        plan.close()
    for tile in (1, 7, 0):
        assert np.array_equal(got[tile][0], before) and np.array_equal(got[tile][1], got[0][1]), tile
    assert np.array_equal(after, before)
    check_against_oracle("predict_var by recurrence across tiles (width %d)" % (JR + 2 * JC), case, xs, got[0][1], truth=True)


@pytest.mark.parametrize("JR,JC", [(2, 3), (1, 1)])
def test_recurrence_on_the_library_trig_kernels(JR, JC):
    """A series offset to t ~ 3e8: max|d| max|t| >= CLR_FAST_TRIG_LIMIT, so the lean plan regenerates phi, u with the
    library sincos (``bpredvar_rec_go<true, false>``) and the points' features take it too.  Against the oracle under
    PHASE_ROUNDING (see there: the absolute phase of a point at 3e8 is rounded, the oracle's relative one is not), and the
    lean layout against the reference layout of the same plan (stored phi, u) within 1e-12 k(0)."""
    B, N = NARROW_B, NARROW_N
    case = synthetic(B, N, JR, JC, "accuracy", seed=77 + JR)
    case["t"] = case["t"] + 3.0e8
    shared, own, perm = prediction_points(case, np.random.RandomState(91))
    out = {}
    for layout in ("lean", "reference"):
        plan = narrow_plan(case, JR, JC, layout)
        try:
            bounds = plan.selection_bounds()
            assert bounds["dmax"] * bounds["tmax"] >= 1.0e9, bounds        # CLR_FAST_TRIG_LIMIT (csrc/clr_core.h)
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            out[layout] = plan.predict(shared, **REC)[1]
        finally:
            plan.close()
        check_against_oracle("predict_var by recurrence, library trig (%s layout)" % layout, case, shared, out[layout], bar=PHASE_ROUNDING)
    for p in range(B):
        within("predict_var by recurrence, library trig: lean vs reference layout, of k(0)",
               np.max(np.abs(out["lean"][p] - out["reference"][p])) / k_zero(case, p), 1e-12, p)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the two routes side by side
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC,layout", [(2, 3, "lean"), (4, 2, "reference"), (1, 0, "lean")])
def test_the_two_routes_agree(JR, JC, layout):
    """``method="recurrence"`` against ``method="solve"`` on the same plan within two PREDICT bars of k(0);
    ``method="solve"`` is the call without ``method``, bit for bit (mean and variance)."""
    B, N = NARROW_B, NARROW_N
    for family in ("bench", "accuracy"):
        case = synthetic(B, N, JR, JC, family, seed=90 + JR)
        shared, own, perm = prediction_points(case, np.random.RandomState(8))
        plan = narrow_plan(case, JR, JC, layout)
        try:
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            plain = plan.predict(own, return_var=True)
            solve = plan.predict(own, return_var=True, method="solve")
            rec = plan.predict(own, **REC)
            plain_again = plan.predict(own, return_var=True)
        finally:
            plan.close()
        assert np.array_equal(solve[0], plain[0]) and np.array_equal(solve[1], plain[1])
        assert np.array_equal(plain_again[1], plain[1]) and np.array_equal(rec[0], plain[0])
        for p in range(B):
            dev = np.max(np.abs(rec[1][p] - solve[1][p])) / k_zero(case, p)
            print("two routes (%d, %d) %s, %s family, problem %d: max |recurrence - solve| / k(0) = %.3e" % (JR, JC, layout, family, p, dev))
            within("predict_var: recurrence vs solve route, of k(0)", dev, 2 * PREDICT, (JR, JC, family, p))


# ---------------------------------------------------------------------------------------------------------------------
# 5. reuse of the factor-only state
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["lean", "reference"])
def test_recurrence_reuses_and_renews_its_factor_state(layout):
    """The chunks' start states are kept between calls: a second call, and calls after a ``solve()`` and a
    ``leave_one_out()`` (which share the chunk maps and the backward start matrices), return the bits of the first; a
    ``leave_one_out()`` BEFORE the first call of a fresh plan changes nothing either.  After new coefficients and a new
    materialising run the route returns the new factor's variances."""
    JR, JC, B, N = 2, 3, NARROW_B, NARROW_N
    case = synthetic(B, N, JR, JC, "bench", seed=12)
    other = synthetic(B, N, JR, JC, "bench", seed=13)
    other["t"], other["diag"], other["y"] = case["t"], case["diag"], case["y"]
    shared, own, perm = prediction_points(case, np.random.RandomState(5))
    plan = narrow_plan(case, JR, JC, layout)
    fresh = narrow_plan(case, JR, JC, layout)
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        first = plan.predict(own, **REC)[1]
        second = plan.predict(own, **REC)[1]
        x = plan.solve()
        loo = plan.leave_one_out()
        third = plan.predict(own, **REC)[1]
        c_after = plan.inverse_diagonal()
        plan.set_coefficients(*coeffs_of(other))
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        renewed = plan.predict(own, **REC)[1]
        assert (fresh.log_likelihood(materialize=True)[3] == 0).all()
        loo_fresh = fresh.leave_one_out()
        late = fresh.predict(own, **REC)[1]
    finally:
        plan.close()
        fresh.close()
    assert np.array_equal(second, first) and np.array_equal(third, first) and np.array_equal(late, first)
    assert np.array_equal(loo_fresh.kinv_diag, loo.kinv_diag) and np.array_equal(c_after, loo.kinv_diag)
    assert np.isfinite(x).all() and not np.array_equal(renewed, first)
    check_against_oracle("predict_var by recurrence (%s layout), first factor" % layout, case, own, first)
    check_against_oracle("predict_var by recurrence (%s layout), after a new materialising run" % layout, other, own, renewed)


# ---------------------------------------------------------------------------------------------------------------------
# 6. sharded
# ---------------------------------------------------------------------------------------------------------------------

def test_sharded_recurrence_equals_the_unsharded_plan():
    """B = 5 over 1 / 2 / 3 shards on the visible devices: every shard on its slice of xs and var, no collective -- the
    same bits as the unsharded plan, for shared, per-problem and unsorted points."""
    JR, JC, B, N = 2, 3, 5, 600
    case = synthetic(B, N, JR, JC, "bench", seed=34)
    shared, own, perm = prediction_points(case, np.random.RandomState(6), M_random=9, M_own=9)
    own = own[:, np.random.RandomState(7).permutation(own.shape[1])]          # (unsorted)
    plan = narrow_plan(case, JR, JC, None, chunks=16, expect=None)
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        want = plan.predict(own, **REC), plan.predict(shared, **REC)
    finally:
        plan.close()
    ndev = batch.device_count()
    for S in (1, 2, 3):
        sp = narrow_plan(case, JR, JC, None, chunks=16, expect=None, cls=batch.ShardedBatchedGP, devices=[s % ndev for s in range(S)])
        try:
            assert (sp.materialize()[3] == 0).all()
            got = sp.predict(own, **REC), sp.predict(shared, **REC)
        finally:
            sp.close()
        for g, w in zip(got, want):
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), S
    check_against_oracle("sharded predict_var by recurrence, the unsharded plan", case, own, want[0][1])


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------

def test_recurrence_refuses_a_wide_plan():
    """(1, 10), N = 2048: CLR_UNSUPPORTED with a message that names the route to take; the solve route still answers."""
    JR, JC, B, N = 1, 10, 2, 2048
    case = synthetic(B, N, JR, JC, "bench", seed=15)
    xs = prediction_points(case, np.random.RandomState(5), M_random=6)[0]
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        with pytest.raises(RuntimeError, match=r"unsupported configuration.*clr_batch_predict_var\b"):
            plan.predict(xs, **REC)
        var = plan.predict(xs, return_var=True)[1]
    finally:
        plan.close()
    check_against_oracle("wide plan after the recurrence route's refusal: the solve route", case, xs, var)


def test_recurrence_without_a_materialising_run_fails_as_the_solve_route():
    JR, JC, B, N = 2, 3, 2, 700
    case = synthetic(B, N, JR, JC, "bench", seed=16)
    xs = np.ascontiguousarray(case["t"][0, ::50])
    var = np.full((B, len(xs)), -1.0)
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        assert (plan.log_likelihood()[3] == 0).all()         # (an evaluation, not a materialising one)
        lib = batch._load()
        said = {}
        for name in ("clr_batch_predict_var", "clr_batch_predict_var_recurrence"):
            fn = getattr(lib, name)
            fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_long, C.POINTER(C.c_double)]
            with pytest.raises(RuntimeError) as err:
                batch._check(fn(plan._h, len(xs), batch._ptr(xs), 0, batch._ptr(var)))
            said[name] = str(err.value)
        assert said["clr_batch_predict_var"] == said["clr_batch_predict_var_recurrence"] and "materialising" in said["clr_batch_predict_var"]
        assert (var == -1.0).all()
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()      # ... and the plan stays usable
        got = plan.predict(xs, **REC)[1]
    finally:
        plan.close()
    check_against_oracle("predict_var by recurrence after the refusal", case, xs, got)
