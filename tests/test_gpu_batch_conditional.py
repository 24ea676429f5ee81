# -*- coding: utf-8 -*-
"""`-m gpu`: the joint posterior at prediction points on batched plans -- ``BatchedGP.predict_cov`` (``clr_batch_predict_cov``)
and ``BatchedGP.sample_conditional`` (``clr_batch_sample_conditional``) -- at every narrow kernel shape in both factor
layouts, on the point sets at which the stitching of the transports can go wrong, under the pivot rule, across batch, tile
and sharding, across reuse of the factor-only state, and where they refuse.

The oracle per problem is ``kernel_value(x_i - x_j) - k*_i^T RefSolver.solve(k*_j)`` with ``k*`` from a NumPy evaluation of
the kernel (the helpers are those of tests/test_gpu_batch_predict_var_recurrence.py, copied).

Bars: ``max |cov - oracle| <= 1e-10 k(0)``, the project's PREDICT bar, of which the variance is the diagonal case; with
``size = M`` and the identity as normals the draws are ``A = L diag(d)^1/2`` and ``A A^T`` is held to the same bar against
``oracle + regularize I`` (the factorisation is backward stable: conditioning does not enter).  A draw from other normals
against ``A n``: both are the same linear recurrence, so they differ by its rounding alone -- held to the PREDICT bar in
units of sqrt k(0) per unit of normal, ``1e-10 sqrt(k(0)) sum |n|``.  The identities themselves are pinned in NumPy by
tests/test_conditional_cpu.py (3.5e-15 k(0) there)."""
import ctypes as C

import numpy as np
import pytest

from celerite_amd import batch
from oracle import ref
from _cases import ALL_WIDTH_SHAPES, synthetic, coeffs_of, within

pytestmark = pytest.mark.gpu

PREDICT = 1e-10
NOGEN = (np.empty(0), np.empty((0, 0)), np.empty((0, 0)))
REC = dict(return_var=True, method="recurrence")
NARROW_B, NARROW_N, NARROW_CHUNKS, L = 4, 700, (22, 32), 32    # set_chunks(24): chunks of 32 samples, the last one 28


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


def oracle_cov(case, p, pts):
    """cov[M, M] of problem p at its points."""
    kstar = kernel_value(case, p, pts[None, :] - case["t"][p][:, None])
    return kernel_value(case, p, pts[:, None] - pts[None, :]) - kstar.T @ oracle_solver(case, p).solve(kstar)


def points_of(pts, p):
    return pts[p] if pts.ndim == 2 else pts


def check_cov(tag, case, pts, cov, skip=()):
    B, M = case["t"].shape[0], pts.shape[-1]
    assert cov.shape == (B, M, M)
    want = {}
    for p in range(B):
        if p in skip:
            continue
        want[p] = oracle_cov(case, p, points_of(pts, p))
        assert np.array_equal(cov[p], cov[p].T), (tag, p)
        within(tag + ": cov vs oracle, of k(0)", np.max(np.abs(cov[p] - want[p])) / k_zero(case, p), PREDICT, p)
    return want


def check_factor(tag, case, want, A, reg=0.0):
    """A[B, M, M] = draws from the identity, transposed: A A^T against the oracle's cov + reg I."""
    for p, w in want.items():
        M = w.shape[0]
        within(tag + ": A A^T vs oracle cov + reg I, of k(0)", np.max(np.abs(A[p] @ A[p].T - w - reg * np.eye(M))) / k_zero(case, p), PREDICT, p)


def zero_mean_draws(plan, pts, normals, regularize=0.0, min_pivot=1e-10):
    """(draws[B, size, M], status[B]) of ``clr_batch_sample_conditional`` itself: no mean added."""
    pts, normals = np.ascontiguousarray(pts, dtype=float), np.ascontiguousarray(normals, dtype=float)
    B, size, M = normals.shape
    draws, st = np.empty((B, size, M)), np.empty(B, dtype=np.int32)
    batch._check(batch._load().clr_batch_sample_conditional(plan._h, M, batch._ptr(pts), 0 if pts.ndim == 1 else M, size, batch._ptr(normals),
                                                            float(regularize), float(min_pivot), batch._ptr(draws),
                                                            st.ctypes.data_as(C.POINTER(C.c_int))))
    return draws, st


def factor_of(plan, pts, **kw):
    """(A[B, M, M], status) with A = L diag(d)^1/2: the draws from the identity as normals, transposed."""
    M = pts.shape[-1]
    out, st = zero_mean_draws(plan, pts, np.broadcast_to(np.eye(M), (plan.B, M, M)), **kw)
    return np.transpose(out, (0, 2, 1)), st


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
def test_covariance_and_factor_at_every_narrow_shape(JR, JC, layout):
    """The kernels are compiled per (J_real, J_comp), factor layout and trig flavour (``bcond_*`` in
    csrc/clr_bcond_kernels.h, instantiated through csrc/clr_batch_kernels.h): all 24 shapes, both layouts, both families,
    22 chunks with a ragged last one.  Shared sorted points, per-problem points, and an unsorted permutation of the shared
    ones, which must give the sorted result permuted on both axes, bit for bit; the diagonal beside the recurrence
    variance; the factor at regularize = 0; a draw from Gaussian normals beside ``A n``."""
    B, N = NARROW_B, NARROW_N
    for family in ("bench", "accuracy"):
        case = synthetic(B, N, JR, JC, family, seed=500 + 9 * JC + JR)
        rng = np.random.RandomState(40 + JR + 7 * JC)
        shared, own, perm = prediction_points(case, rng)
        M = len(shared)
        n = rng.standard_normal((B, 2, M))
        plan = narrow_plan(case, JR, JC, layout)
        try:
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            cov = plan.predict_cov(shared)
            cov_own = plan.predict_cov(own)
            cov_perm = plan.predict_cov(shared[perm])
            mean, var = plan.predict(shared, **REC)
            A, st = factor_of(plan, shared)
            A_own, st_own = factor_of(plan, own)
            A_perm, st_perm = factor_of(plan, shared[perm])
            f = zero_mean_draws(plan, shared, n)[0]
        finally:
            plan.close()
        tag = "conditional (%s layout, %s family)" % (layout, family)
        assert (st == 0).all() and (st_own == 0).all() and (st_perm == 0).all(), tag
        assert np.array_equal(cov_perm, cov[:, perm][:, :, perm]), tag
        assert np.array_equal(A_perm, A[:, perm][:, :, perm]), tag
        want = check_cov(tag + ", shared points", case, shared, cov)
        want_own = check_cov(tag + ", per-problem points", case, own, cov_own)
        check_factor(tag + ", shared points", case, want, A)
        check_factor(tag + ", per-problem points", case, want_own, A_own)
        for p in range(B):
            k0 = k_zero(case, p)
            within(tag + ": diag(cov) vs the recurrence variance, of k(0)", np.max(np.abs(np.diagonal(cov[p]) - var[p])) / k0, PREDICT, p)
            assert np.array_equal(np.triu(A[p], 1), np.zeros((M, M))), (tag, p)
            within(tag + ": a draw vs A n, of sqrt k(0) sum |n|",
                   np.max(np.abs(f[p] - n[p] @ A[p].T) / np.sum(np.abs(n[p]), axis=1, keepdims=True)) / np.sqrt(k0), PREDICT, p)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the point sets at which the stitching can go wrong
# ---------------------------------------------------------------------------------------------------------------------

def edge_sets(t, rng):
    """Per-problem point sets [B, M] for a series in 22 chunks of 32 (the last one of 28)."""
    B, N = t.shape
    gap = lambda p, n, f: t[p, n] + f * (t[p, n + 1] - t[p, n])
    delta = 0.37 * np.min(np.diff(t, axis=1), axis=1)
    rows = lambda fn: np.stack([np.sort(np.asarray(fn(p), dtype=float)) for p in range(B)])
    sets = {}
    # ~40 points in chunks 0, 5, 9, 21 -- the others own none: outside both ends, exact data times (the first and the last
    # sample, the first and the last sample of chunk 5), three points in one gap, a run across the gap between chunks 5 | 6
    sets["about 40 points, most chunks own none"] = rows(lambda p: np.concatenate([
        [t[p, 0] - 3 * delta[p], t[p, 0] - delta[p], t[p, 0], t[p, 5 * L], t[p, 6 * L - 1], gap(p, 6 * L - 1, 0.5)],
        [gap(p, 300, f) for f in (0.2, 0.5, 0.8)], [gap(p, n, 0.4) for n in range(5 * L + 3, 5 * L + 27, 2)],
        [gap(p, n, 0.6) for n in range(9 * L + 1, 9 * L + 25, 3)], [gap(p, n, 0.5) for n in range(21 * L + 2, 21 * L + 20, 3)],
        [t[p, N - 1], t[p, N - 1] + delta[p], t[p, N - 1] + 4 * delta[p]]]))
    sets["one point per chunk"] = rows(lambda p: [gap(p, c * L + 5 + (c % 7), 0.3) for c in range(22)])
    sets["all points in the last chunk"] = rows(lambda p: np.concatenate([[gap(p, n, 0.5) for n in range(21 * L, N - 1, 4)], [t[p, N - 1], t[p, N - 1] + delta[p]]]))
    sets["one point"] = rows(lambda p: [gap(p, 333, 0.5)])
    sets["two points, a chunk boundary and empty chunks between"] = rows(lambda p: [gap(p, 3 * L + 30, 0.5), gap(p, 11 * L + 1, 0.5)])
    sets["two points in neighbouring chunks"] = rows(lambda p: [gap(p, 4 * L - 1, 0.5), t[p, 4 * L]])
    sets["points before the first sample only"] = rows(lambda p: t[p, 0] - delta[p] * np.array([5.0, 3.0, 1.0]))
    sets["points after the last sample only"] = rows(lambda p: t[p, N - 1] + delta[p] * np.array([0.0, 1.0, 2.5]))
    m40 = sets["about 40 points, most chunks own none"]
    assert 38 <= m40.shape[1] <= 45
    for p in range(B):
        owner = np.clip((np.searchsorted(t[p], m40[p], side="right") - 1) // L, 0, None)
        assert sorted(set(owner)) == [0, 5, 9, 21]
    return sets


@pytest.mark.parametrize("JR,JC,layout", [(2, 3, "lean"), (4, 2, "reference"), (1, 0, "lean")])
def test_conditional_on_the_edge_point_sets(JR, JC, layout):
    """Covariance against the oracle and ``A A^T`` against ``oracle + regularize I`` at ``regularize = 1e-8 k(0)`` (problem
    0's k(0): one value per call) on every edge set, both families."""
    B, N = NARROW_B, NARROW_N
    for family in ("bench", "accuracy"):
        case = synthetic(B, N, JR, JC, family, seed=77 + JR)
        reg = 1e-8 * k_zero(case, 0)
        sets = edge_sets(case["t"], np.random.RandomState(3))
        got = {}
        plan = narrow_plan(case, JR, JC, layout)
        try:
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            for name, pts in sets.items():
                got[name] = (plan.predict_cov(pts),) + factor_of(plan, pts, regularize=reg)
        finally:
            plan.close()
        for name, pts in sets.items():
            tag = "conditional on '%s' (%d, %d) %s, %s family" % (name, JR, JC, layout, family)
            cov, A, st = got[name]
            assert (st == 0).all(), tag
            want = check_cov(tag, case, pts, cov)
            check_factor(tag, case, want, A, reg)


# ---------------------------------------------------------------------------------------------------------------------
# 3. sample_conditional is predict plus the draws, under a constant and a linear mean
# ---------------------------------------------------------------------------------------------------------------------

def test_sample_conditional_adds_the_mean_of_predict():
    JR, JC, B, N = 2, 3, NARROW_B, NARROW_N
    case = synthetic(B, N, JR, JC, "accuracy", seed=21)
    rng = np.random.RandomState(9)
    shared, own, perm = prediction_points(case, rng, M_random=12, M_own=12)
    M = own.shape[1]
    n1, n3 = rng.standard_normal((B, M)), rng.standard_normal((B, 3, M))
    basis = np.stack([np.ones((B, N)), case["t"] - case["t"].mean()], axis=1)
    basis_at = np.stack([np.ones((B, M)), own - case["t"].mean()], axis=1)
    w = rng.standard_normal((B, 2))
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        raw1, raw3 = zero_mean_draws(plan, own, n1[:, None, :])[0][:, 0], zero_mean_draws(plan, own, n3)[0]
        mean0 = plan.predict(own)
        zero = plan.sample_conditional(own, normals=n1), plan.sample_conditional(own, size=3, normals=n3)
        seeded = plan.sample_conditional(own, size=3, random=np.random.RandomState(4))
        again = plan.sample_conditional(own, size=3, normals=np.random.RandomState(4).standard_normal((B, 3, M)))
        plan.set_mean(np.arange(1.0, B + 1.0))
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        const = plan.sample_conditional(own, size=3, normals=n3), plan.predict(own)
    finally:
        plan.close()
    assert zero[0].shape == (B, M) and zero[1].shape == (B, 3, M) and np.array_equal(seeded, again)
    assert np.array_equal(zero[0], mean0 + raw1) and np.array_equal(zero[1], mean0[:, None, :] + raw3)
    # (the factor does not depend on the mean: the zero-mean parts are the same bits)
    assert np.array_equal(const[0], const[1][:, None, :] + raw3) and not np.array_equal(const[1], mean0)
    lin = narrow_plan(case, JR, JC, "lean")
    try:
        lin.set_mean_basis(basis)
        lin.set_mean_weights(w)
        assert (lin.log_likelihood(materialize=True)[3] == 0).all()
        with pytest.raises(ValueError, match="mean_basis"):
            lin.sample_conditional(own, normals=n1)
        got = lin.sample_conditional(own, size=3, normals=n3, mean_basis=basis_at)
        mean = lin.predict(own, mean_basis=basis_at)
    finally:
        lin.close()
    assert np.array_equal(got, mean[:, None, :] + raw3)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the pivot rule
# ---------------------------------------------------------------------------------------------------------------------

def test_a_repeated_point_gives_two_equal_columns():
    """A point given twice (per problem, inside a gap): status 0, the second pivot is degenerate -- its row of A has no
    diagonal entry -- and the two columns of every draw are equal up to the rounding of ``r^T omega = 1``: 64 roundings of
    numbers of size k(0) over the first copy's pivot d, times z = sqrt(d) n (tests/test_conditional_cpu.py), d from the
    oracle's covariance."""
    JR, JC, B, N = 2, 3, NARROW_B, NARROW_N
    case = synthetic(B, N, JR, JC, "accuracy", seed=31)
    rng = np.random.RandomState(1)
    t = case["t"]
    twice = t[:, 417] + 0.3 * (t[:, 418] - t[:, 417])
    base = np.sort(rng.uniform(t.min(), t.max(), (B, 9)), axis=1)
    pts = np.sort(np.concatenate([base, twice[:, None], twice[:, None]], axis=1), axis=1)
    M = pts.shape[1]
    n = rng.standard_normal((B, 4, M))
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        A, st = factor_of(plan, pts)
        f = zero_mean_draws(plan, pts, n)[0]
        cov = plan.predict_cov(pts)
    finally:
        plan.close()
    assert (st == 0).all()
    want = check_cov("conditional with a repeated point", case, pts, cov)
    check_factor("conditional with a repeated point", case, want, A)
    for p in range(B):
        rep = int(np.flatnonzero(np.diff(pts[p]) == 0)[0]) + 1
        assert A[p][rep, rep] == 0.0 and (np.delete(np.diagonal(A[p]), rep) > 0).all(), p
        C = want[p]
        d = C[rep - 1, rep - 1] - C[rep - 1, :rep - 1] @ np.linalg.solve(C[:rep - 1, :rep - 1], C[:rep - 1, rep - 1])
        bar = 64 * np.finfo(float).eps * k_zero(case, p) / np.sqrt(d) * np.max(np.abs(n[p]))
        within("conditional: the two columns of a repeated point, of their bar", np.max(np.abs(f[p][:, rep] - f[p][:, rep - 1])) / bar, 1.0, p)


def test_conditional_beside_a_refused_problem():
    """One problem in the middle is not positive definite in the materialising run (status 2): NaN rows and its status for
    that problem, the others the bits of a plan whose problem in the middle is sound.  A negative regularize is refused
    as an argument."""
    JR, JC, B, N = 2, 3, 5, 700
    case = synthetic(B, N, JR, JC, "bench", seed=1000 + 3 * JR + JC)
    mid = B // 2
    good = {k: np.array(v) for k, v in case.items()}
    case["a_real"][mid] *= -40.0
    shared = prediction_points(case, np.random.RandomState(2), M_random=10)[0]
    M = len(shared)
    out = {}
    for name, c in (("bad", case), ("good", good)):
        plan = narrow_plan(c, JR, JC, "lean")
        try:
            st = plan.log_likelihood(materialize=True)[3]
            out[name] = (st, plan.predict_cov(shared)) + factor_of(plan, shared)
            if name == "good":
                with pytest.raises(RuntimeError, match="invalid argument.*regularize"):
                    lib = batch._load()
                    z, dr, s = np.zeros((B, 1, M)), np.zeros((B, 1, M)), np.zeros(B, dtype=np.int32)
                    batch._check(lib.clr_batch_sample_conditional(plan._h, M, batch._ptr(shared), 0, 1, batch._ptr(z), -1.0, 1e-10, batch._ptr(dr),
                                                                  s.ctypes.data_as(C.POINTER(C.c_int))))
        finally:
            plan.close()
    st, cov, A, fst = out["bad"]
    assert st[mid] == 2 and (np.delete(st, mid) == 0).all() and np.array_equal(fst, st)
    assert np.isnan(cov[mid]).all() and np.isnan(A[mid]).all()
    keep = np.arange(B) != mid
    assert np.array_equal(cov[keep], out["good"][1][keep]) and np.array_equal(A[keep], out["good"][2][keep])
    check_cov("conditional beside a refused problem", case, shared, cov, skip=(mid,))


def test_a_negative_pivot_refuses_the_problem_alone():
    """Zero observational variance on problem 1 and points on its exact data times: the posterior variance there is zero,
    the pivots are rounding noise of either sign.  With min_pivot = 1e-10 they are degenerate and every problem answers
    (status 0, A A^T within the bar); with min_pivot = 0 a negative one refuses that problem -- status 2, NaN rows -- or
    it answers, and the other problems' bits do not change either way."""
    JR, JC, B, N = 2, 3, NARROW_B, NARROW_N
    case = synthetic(B, N, JR, JC, "accuracy", seed=41)
    case["diag"][1] = 0.0
    pts = np.stack([np.sort(np.concatenate([case["t"][p, 100:420:40], [case["t"][p, 0] - 1.0]])) for p in range(B)])
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        cov = plan.predict_cov(pts)
        A, st = factor_of(plan, pts)
        A0, st0 = factor_of(plan, pts, min_pivot=0.0)
    finally:
        plan.close()
    assert (st == 0).all()
    want = check_cov("conditional on noiseless samples", case, pts, cov)
    check_factor("conditional on noiseless samples", case, want, A)
    assert np.count_nonzero(np.diagonal(A[1])) == 1          # (only the point before the series is free)
    keep = np.arange(B) != 1
    assert (st0[keep] == 0).all() and np.array_equal(A0[keep], A[keep]) and st0[1] in (0, 2)
    assert np.isnan(A0[1]).all() if st0[1] == 2 else np.isfinite(A0[1]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. independence of the batch, the tile and the sharding; reuse of the factor-only state
# ---------------------------------------------------------------------------------------------------------------------

def test_conditional_does_not_depend_on_batch_or_tile():
    """Problem 2 alone in a plan of its own, and tiles of 1, of 3 (B = 4: a ragged last tile) and the automatic one: the
    same bits, for unsorted per-problem points."""
    JR, JC, B, N = 2, 3, NARROW_B, NARROW_N
    case = synthetic(B, N, JR, JC, "accuracy", seed=24)
    rng = np.random.RandomState(3)
    own = prediction_points(case, rng, M_own=14)[1][:, rng.permutation(14)]
    n = rng.standard_normal((B, 3, 14))
    got = {}
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        for tile in (0, 1, 3):
            plan.set_conditional_tile(tile)
            got[tile] = plan.predict_cov(own), plan.sample_conditional(own, size=3, normals=n, regularize=1e-9)
    finally:
        plan.close()
    one = {k: v[2:3] for k, v in case.items()}
    solo = narrow_plan(one, JR, JC, "lean")
    try:
        assert (solo.log_likelihood(materialize=True)[3] == 0).all()
        alone = solo.predict_cov(own[2:3]), solo.sample_conditional(own[2:3], size=3, normals=n[2:3], regularize=1e-9)
    finally:
        solo.close()
    for tile in (1, 3):
        assert np.array_equal(got[tile][0], got[0][0]) and np.array_equal(got[tile][1], got[0][1]), tile
    assert np.array_equal(alone[0][0], got[0][0][2]) and np.array_equal(alone[1][0], got[0][1][2])
    check_cov("conditional across tiles", case, own, got[0][0])


def test_sharded_conditional_equals_the_unsharded_plan():
    """B = 5 over 1 / 2 / 3 shards on the visible devices: every shard on its slice, no collective -- the same bits as the
    unsharded plan, for shared and for unsorted per-problem points."""
    JR, JC, B, N = 2, 3, 5, 600
    case = synthetic(B, N, JR, JC, "bench", seed=34)
    rng = np.random.RandomState(6)
    shared, own, perm = prediction_points(case, rng, M_random=9, M_own=9)
    own = own[:, rng.permutation(own.shape[1])]
    n_own, n_sh = rng.standard_normal((B, 2, own.shape[1])), rng.standard_normal((B, len(shared)))

    def run(p):
        return (p.predict_cov(own), p.predict_cov(shared), p.sample_conditional(own, size=2, normals=n_own, return_status=True),
                p.sample_conditional(shared, normals=n_sh))

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
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3]), S
        assert np.array_equal(got[2][0], want[2][0]) and np.array_equal(got[2][1], want[2][1]), S
    check_cov("sharded conditional, the unsharded plan", case, own, want[0])


@pytest.mark.parametrize("layout", ["lean", "reference"])
def test_conditional_reuses_and_renews_the_factor_state(layout):
    """A call on a fresh factor, a second call, and calls after ``solve()``, ``leave_one_out()`` and
    ``predict(..., method="recurrence")`` (which form the chunk maps, Q and S) return the same bits, and so does a call on
    a fresh plan AFTER those -- a chunk that owns no point is the solve's chunk map where that is formed and the chunk's
    own product where not.  After new coefficients and a new materialising run the results follow the new factor."""
    JR, JC, B, N = 2, 3, NARROW_B, NARROW_N
    case = synthetic(B, N, JR, JC, "bench", seed=12)
    other = synthetic(B, N, JR, JC, "bench", seed=13)
    other["t"], other["diag"], other["y"] = case["t"], case["diag"], case["y"]
    rng = np.random.RandomState(5)
    own = prediction_points(case, rng, M_own=12)[1]
    n = rng.standard_normal((B, 2, 12))
    run = lambda p: (p.predict_cov(own), p.sample_conditional(own, size=2, normals=n, regularize=1e-9))
    plan = narrow_plan(case, JR, JC, layout)
    fresh = narrow_plan(case, JR, JC, layout)
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        first = run(plan)
        second = run(plan)
        plan.solve()
        plan.leave_one_out()
        var = plan.predict(own, **REC)[1]
        third = run(plan)
        plan.set_coefficients(*coeffs_of(other))
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        renewed = run(plan)
        assert (fresh.log_likelihood(materialize=True)[3] == 0).all()
        fresh.solve()
        fresh.leave_one_out()
        var_fresh = fresh.predict(own, **REC)[1]
        late = run(fresh)
    finally:
        plan.close()
        fresh.close()
    for got in (second, third, late):
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
    assert np.array_equal(var, var_fresh) and not np.array_equal(renewed[0], first[0])
    check_cov("conditional (%s layout), first factor" % layout, case, own, first[0])
    check_cov("conditional (%s layout), after a new materialising run" % layout, other, own, renewed[0])


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------

def test_conditional_refusals():
    """A wide plan (1, 10) at N = 2048, an unchunked plan (N = 100), a NaN point and size < 1 return their status and
    message; ``predict`` still answers afterwards where it answers at all."""
    lib = batch._load()
    ip = C.POINTER(C.c_int)
    for JR, JC, N, said in ((1, 10, 2048, r"unsupported configuration.*%s covers narrow plans \(widths 1\.\.8\)"),
                            (2, 3, 100, r"unsupported configuration.*%s needs a chunked plan \(N >= 128\)")):
        B = 2
        case = synthetic(B, N, JR, JC, "bench", seed=15)
        xs = prediction_points(case, np.random.RandomState(5), M_random=6)[0]
        plan = batch.BatchedGP(B, N, JR, JC)
        try:
            plan.set_series(case["t"], case["diag"], case["y"])
            plan.set_coefficients(*coeffs_of(case))
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            with pytest.raises(RuntimeError, match=said % "clr_batch_predict_cov"):
                plan.predict_cov(xs)
            with pytest.raises(RuntimeError, match=said % "clr_batch_sample_conditional"):
                plan.sample_conditional(xs)
            # (predict itself needs a chunked plan: the short one shows that it still evaluates)
            after = plan.predict(xs) if N >= 128 else plan.log_likelihood()[0]
        finally:
            plan.close()
        assert np.isfinite(after).all()
    JR, JC, B, N = 2, 3, 2, 700
    case = synthetic(B, N, JR, JC, "bench", seed=16)
    xs = np.ascontiguousarray(case["t"][0, ::50])
    M = len(xs)
    bad = xs.copy()
    bad[3] = np.nan
    cov, z, dr, st = np.full((B, M, M), -1.0), np.zeros((B, 1, M)), np.full((B, 1, M), -1.0), np.full(B, -7, dtype=np.int32)
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        with pytest.raises(RuntimeError, match="invalid argument.*clr_batch_predict_cov: a point is NaN"):
            plan.predict_cov(bad)
        with pytest.raises(RuntimeError, match="invalid argument.*clr_batch_sample_conditional: a point is NaN"):
            plan.sample_conditional(bad)
        with pytest.raises(RuntimeError, match="invalid argument.*size >= 1"):
            batch._check(lib.clr_batch_sample_conditional(plan._h, M, batch._ptr(xs), 0, 0, batch._ptr(z), 0.0, 1e-10, batch._ptr(dr), st.ctypes.data_as(ip)))
        with pytest.raises(RuntimeError, match="invalid argument.*min_pivot"):
            batch._check(lib.clr_batch_sample_conditional(plan._h, M, batch._ptr(xs), 0, 1, batch._ptr(z), 0.0, 1.0, batch._ptr(dr), st.ctypes.data_as(ip)))
        with pytest.raises(RuntimeError, match="invalid argument"):
            batch._check(lib.clr_batch_predict_cov(plan._h, M, batch._ptr(xs), 0, None))
        with pytest.raises(RuntimeError, match="invalid argument.*stride"):
            batch._check(lib.clr_batch_predict_cov(plan._h, M, batch._ptr(xs), 3, batch._ptr(cov)))
        batch._check(lib.clr_batch_predict_cov(plan._h, 0, None, 0, batch._ptr(cov)))
        assert (cov == -1.0).all() and (dr == -1.0).all() and (st == -7).all()
        mean = plan.predict(xs)
        got = plan.predict_cov(xs)
        ms = plan.solve_device_ms()
    finally:
        plan.close()
    assert np.isfinite(mean).all() and ms > 0.0
    check_cov("conditional after the refusals", case, xs, got)
