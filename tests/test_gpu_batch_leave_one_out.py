# -*- coding: utf-8 -*-
"""`-m gpu`: diag(K^-1), K^-1 r and the leave-one-out predictive distribution on batched plans --
``BatchedGP.inverse_diagonal`` / ``.leave_one_out``, ``clr_batch_leave_one_out`` -- at every narrow kernel shape in both
factor layouts, on the library-trig instantiations, in every bucket of the wide consumers, past 65535 problems, sharded,
with a mean in force and beside a refused problem, against the CPU oracle.

The oracle for ``c = diag(K^-1)`` is ``diag(RefSolver.solve(I))`` per problem, for ``alpha`` it is ``RefSolver.solve(r)``.

Bars: the project's solve bars (test_gpu_batch_consumers.py), since ``c_n`` is entry n of a solve --
``max_n |c_dev - c_oracle| <= 1e-10 max_n c_oracle`` on narrow plans, ``2e-11`` on wide ones; ``alpha`` the same against
its own largest entry.  The per-entry relative deviation of ``c`` (and so of ``variance = 1 / c``) is recorded under the
same bar times 250, the measured spread of one problem's entries.  ``residual = alpha / c``: per entry
``|d res_n| <= |d alpha_n| / c_n + |res_n| |d c_n| / c_n``; with the spread of 250 in ``c``, ``max |alpha| / c_n`` is at
most 250 times the largest residual, so both terms stay below 250 bar times the largest residual: the bar is 500 bar of
the largest entry.  On the CPU the double oracle sits <= 3.3e-13 relative from binary128, and the chunked recurrence in
NumPy on the oracle's factor <= 2.7e-15 from the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

from celerite_amd import batch
from oracle import ref
from _cases import ALL_WIDTH_SHAPES, CONSUMER_WIDE_SHAPES, NO_GENERAL, synthetic, coeffs_of, within

pytestmark = pytest.mark.gpu

NARROW, WIDE = 1e-10, 2e-11
SPREAD = 250.0
FAST_TRIG_LIMIT = 1.0e9        # CLR_FAST_TRIG_LIMIT (csrc/clr_core.h)
NARROW_B, NARROW_N, NARROW_CHUNKS = 4, 700, (22, 32)    # set_chunks(24): chunks of 32 samples, the last one 28


def oracle_solver(case, p):
    r = ref.RefSolver()
    try:
        r.compute(0.0, *coeffs_of(case, p), *NO_GENERAL, case["t"][p], case["diag"][p])
    except ref.RefLinAlgError:
        return None
    return r


def oracle_of(case, resid=None, skip=()):
    """(c[B, N], alpha[B, N]) of the oracle; ``resid``: the residual the solve sees (default: y)."""
    B, N = case["t"].shape
    resid = case["y"] if resid is None else resid
    c, a = np.full((B, N), np.nan), np.full((B, N), np.nan)
    for p in range(B):
        if p in skip:
            continue
        r = oracle_solver(case, p)
        c[p] = np.diag(r.solve(np.eye(N)))
        a[p] = np.asarray(r.solve(resid[p])).reshape(N)
    return c, a


@functools.lru_cache(maxsize=None)
def narrow_case(JR, JC, family):
    """One case and its oracle per shape and family, shared by both layouts (the arrays are not written to)."""
    case = synthetic(NARROW_B, NARROW_N, JR, JC, family, seed=700 + 9 * JC + JR)
    return case, oracle_of(case)


def check_c(tag, c, c0, bar, skip=()):
    for p in range(c0.shape[0]):
        if p in skip:
            continue
        within(tag + ": c vs oracle, of the largest entry", np.max(np.abs(c[p] - c0[p])) / np.max(c0[p]), bar, p)
        within(tag + ": c vs oracle, per entry", np.max(np.abs(c[p] - c0[p]) / c0[p]), SPREAD * bar, p)


def check_all(tag, loo, c0, a0, bar, skip=()):
    """Every field of a LeaveOneOut against the oracle's c and alpha."""
    check_c(tag, loo.kinv_diag, c0, bar, skip)
    res0, var0, lp0 = batch.leave_one_out_from(c0, a0)
    own = batch.leave_one_out_from(loo.kinv_diag, loo.alpha)
    for p in range(c0.shape[0]):
        if p in skip:
            continue
        within(tag + ": alpha vs oracle, of the largest entry", np.max(np.abs(loo.alpha[p] - a0[p])) / np.max(np.abs(a0[p])), bar, p)
        within(tag + ": variance vs oracle, per entry", np.max(np.abs(loo.variance[p] - var0[p]) / var0[p]), SPREAD * bar, p)
        within(tag + ": residual vs oracle, of the largest entry",
               np.max(np.abs(loo.residual[p] - res0[p])) / np.max(np.abs(res0[p])), 2.0 * SPREAD * bar, p)
        within(tag + ": logpdf vs leave_one_out_from(oracle)", abs(loo.logpdf[p] - lp0[p]) / abs(lp0[p]), 1e-10, p)
        within(tag + ": device logpdf vs leave_one_out_from(its own arrays)", abs(loo.logpdf[p] - own[2][p]) / abs(own[2][p]), 1e-13, p)
        assert np.array_equal(loo.residual[p], own[0][p]) and np.array_equal(loo.variance[p], own[1][p])


def check_truth(tag, case, c, c0, idx, bar):
    """Device and double oracle of problem 0 against binary128 (the solve of the unit vector), side by side."""
    N = case["t"].shape[1]
    cq = np.array([ref.quad_factor_solve(0.0, *coeffs_of(case, 0), case["t"][0], case["diag"][0], np.eye(N)[n], want_factor=False)[2][n]
                   for n in idx])
    scale = np.max(c0[0])
    within(tag + ": device c vs binary128, of the largest entry", np.max(np.abs(c[0][idx] - cq)) / scale, bar)
    within(tag + ": double oracle c vs binary128, of the largest entry", np.max(np.abs(c0[0][idx] - cq)) / scale, bar)


def narrow_plan(case, JR, JC, layout, chunks=24, expect=NARROW_CHUNKS):
    B, N = case["t"].shape
    plan = batch.BatchedGP(B, N, JR, JC)
    plan.set_chunks(chunks)
    if expect:
        assert plan.chunks == expect and N % expect[1] != 0      # a ragged last chunk
    plan.set_factor_layout(layout)
    plan.set_series(case["t"], case["diag"], case["y"])
    plan.set_coefficients(*coeffs_of(case))
    return plan


# ---------------------------------------------------------------------------------------------------------------------
# 1. narrow plans (widths 1..8) at every (J_real, J_comp) shape, both factor layouts
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["reference", "lean"])
@pytest.mark.parametrize("JR,JC", ALL_WIDTH_SHAPES)
def test_narrow_leave_one_out_at_every_shape(JR, JC, layout):
    """``binvdiag_*`` (csrc/clr_binvdiag_kernels.h) is compiled per (J_real, J_comp), factor layout and trig flavour: all
    24 shapes, both layouts, both families, 22 chunks of 32 with a ragged last one of 28.  On the accuracy family problem
    0 goes against binary128 at the chunk edges, in the ragged chunk and at both ends."""
    N = NARROW_N
    for family in ("bench", "accuracy"):
        case, (c0, a0) = narrow_case(JR, JC, family)
        plan = narrow_plan(case, JR, JC, layout)
        try:
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            loo = plan.leave_one_out()
        finally:
            plan.close()
        tag = "narrow leave_one_out (%s layout, %s family)" % (layout, family)
        assert (loo.status == 0).all()
        check_all(tag, loo, c0, a0, NARROW)
        if family == "accuracy":
            check_truth(tag, case, loo.kinv_diag, c0, [0, 31, 32, N // 3, 671, 672, N - 1], NARROW)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the same bits whatever ran before
# ---------------------------------------------------------------------------------------------------------------------

def test_inverse_diagonal_does_not_depend_on_what_ran_before():
    """The chunk maps are the batched solve's: formed here straight after the materialising run, by ``solve`` or by the
    predictive variance before the other calls -- the same kernel, so the same bits; alpha is ``solve()``'s."""
    JR, JC = 2, 3
    case = synthetic(NARROW_B, NARROW_N, JR, JC, "accuracy", seed=17)
    xs = np.linspace(case["t"].min(), case["t"].max(), 9)
    plan = narrow_plan(case, JR, JC, "lean")
    try:
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        first = plan.inverse_diagonal()
        x = plan.solve()
        after_solve = plan.inverse_diagonal()
        plan.predict(xs, return_var=True)
        after_var = plan.inverse_diagonal()
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        again = plan.inverse_diagonal()
        loo = plan.leave_one_out()
        x2 = plan.solve()
    finally:
        plan.close()
    assert np.array_equal(first, after_solve) and np.array_equal(first, after_var) and np.array_equal(first, again)
    assert np.array_equal(loo.kinv_diag, first) and np.array_equal(loo.alpha, x) and np.array_equal(x, x2)
    check_c("inverse_diagonal straight after the materialising run", first, oracle_of(case)[0], NARROW)


# ---------------------------------------------------------------------------------------------------------------------
# 3. a mean in force
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC", [(2, 3), (4, 4)])
def test_leave_one_out_with_a_mean_in_force(JR, JC):
    """A mean changes the residual, not K: kinv_diag keeps its bits, alpha and residual follow the new residual;
    ``arrays=False`` returns the same logpdf bits with ``None`` arrays."""
    narrow = JR + 2 * JC <= 8
    B, N = (NARROW_B, NARROW_N) if narrow else (3, 512)
    bar = NARROW if narrow else WIDE
    case = synthetic(B, N, JR, JC, "bench", seed=23 + JC)
    mu = np.linspace(-1.0, 2.0, B)
    Phi = np.stack([np.ones(N), np.linspace(-1.0, 1.0, N)])
    w = np.random.RandomState(4).uniform(-0.5, 0.5, (B, 2))
    plan = narrow_plan(case, JR, JC, "lean") if narrow else batch.BatchedGP(B, N, JR, JC)
    try:
        if not narrow:
            plan.set_series(case["t"], case["diag"], case["y"])
            plan.set_coefficients(*coeffs_of(case))
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        plain = plan.leave_one_out()
        plan.set_mean(mu)
        const = plan.leave_one_out()
        const_small = plan.leave_one_out(arrays=False)
        plan.set_mean(None)
        plan.set_mean_basis(Phi)
        plan.set_mean_weights(w)
        linear = plan.leave_one_out()
        linear_small = plan.leave_one_out(arrays=False)
    finally:
        plan.close()
    c0, a0 = oracle_of(case)
    tag = "leave_one_out with a mean (width %d)" % (JR + 2 * JC)
    check_all(tag + ", no mean", plain, c0, a0, bar)
    for name, got, small, resid in (("constant", const, const_small, case["y"] - mu[:, None]), ("linear", linear, linear_small, case["y"] - w @ Phi)):
        assert np.array_equal(got.kinv_diag, plain.kinv_diag), name
        assert not np.array_equal(got.alpha, plain.alpha), name
        check_all(tag + ", %s mean" % name, got, c0, oracle_of(case, resid)[1], bar)
        assert np.array_equal(small.logpdf, got.logpdf) and np.array_equal(small.status, got.status), name
        assert small.residual is None and small.variance is None and small.kinv_diag is None and small.alpha is None


# ---------------------------------------------------------------------------------------------------------------------
# 4. the library-trig instantiations
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC", [(2, 3), (1, 1)])
def test_narrow_leave_one_out_on_the_library_trig_kernels(JR, JC):
    """A series offset to t ~ 3e8: max|d| max|t| >= CLR_FAST_TRIG_LIMIT, so the lean plan regenerates phi, u with the
    library sincos (``binvdiag_go<true, false>``).  Against the oracle, and the lean layout against the reference layout
    of the same plan (stored phi, u: no trigonometry) within 1e-12 of the largest entry."""
    case = synthetic(NARROW_B, NARROW_N, JR, JC, "accuracy", seed=77 + JR)
    case["t"] = case["t"] + 3.0e8
    c0, a0 = oracle_of(case)
    out = {}
    for layout in ("lean", "reference"):
        plan = narrow_plan(case, JR, JC, layout)
        try:
            bounds = plan.selection_bounds()
            assert bounds["dmax"] * bounds["tmax"] >= FAST_TRIG_LIMIT, bounds
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            out[layout] = plan.leave_one_out()
        finally:
            plan.close()
        check_all("narrow leave_one_out, library trig (%s layout)" % layout, out[layout], c0, a0, NARROW)
    for p in range(NARROW_B):
        within("narrow leave_one_out, library trig: lean vs reference layout, of the largest entry",
               np.max(np.abs(out["lean"].kinv_diag[p] - out["reference"].kinv_diag[p])) / np.max(c0[p]), 1e-12, p)


# ---------------------------------------------------------------------------------------------------------------------
# 5. wide plans (widths 9..64)
# ---------------------------------------------------------------------------------------------------------------------

def wide_loo(case, JR, JC):
    B, N = case["t"].shape
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        st = plan.log_likelihood(materialize=True)[3]
        return st, plan.leave_one_out()
    finally:
        plan.close()


@pytest.mark.parametrize("JR,JC", CONSUMER_WIDE_SHAPES)
def test_wide_leave_one_out_at_every_consumer_shape(JR, JC):
    B, N = 3, 512
    case = synthetic(B, N, JR, JC, "bench", seed=1000 + N % 97 + 3 * JR + JC)
    st, loo = wide_loo(case, JR, JC)
    assert (st == 0).all() and (loo.status == 0).all()
    check_all("wide leave_one_out (width %d, N = %d)" % (JR + 2 * JC, N), loo, *oracle_of(case), WIDE)


@pytest.mark.parametrize("JR,JC", [(1, 15), (0, 32)])
def test_wide_leave_one_out_on_a_longer_series_against_binary128(JR, JC):
    """N = 2047 (no multiple of the kernel's tile of 16 samples), accuracy family; problem 0 against binary128 at both
    ends and in the middle."""
    B, N = 3, 2047
    case = synthetic(B, N, JR, JC, "accuracy", seed=1000 + N % 97 + 3 * JR + JC)
    st, loo = wide_loo(case, JR, JC)
    assert (st == 0).all() and (loo.status == 0).all()
    c0, a0 = oracle_of(case)
    tag = "wide leave_one_out (width %d, N = %d)" % (JR + 2 * JC, N)
    check_all(tag, loo, c0, a0, WIDE)
    check_truth(tag, case, loo.kinv_diag, c0, [0, N // 2, N - 1], WIDE)


@pytest.mark.parametrize("JR,JC", CONSUMER_WIDE_SHAPES)
def test_wide_leave_one_out_refuses_a_series_shorter_than_512(JR, JC):
    """N = 511: CLR_UNSUPPORTED, never numbers, and the plan stays usable."""
    B, N = 2, 511
    case = synthetic(B, N, JR, JC, "bench", seed=5 + JC)
    z = np.random.RandomState(3).randn(B, N)
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        lib = batch._load()
        c = np.full((B, N), -7.0)
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            batch._check(lib.clr_batch_leave_one_out(plan._h, batch._ptr(c), None, None, None))
        assert (c == -7.0).all()
        got_L = plan.dot_L(z)
    finally:
        plan.close()
    for p in range(B):
        want = oracle_solver(case, p).dot_L(z[p])[:, 0]
        within("wide plan at N = 511 after the refusal: dot_L vs oracle, of the largest entry",
               np.max(np.abs(got_L[p] - want)) / np.max(np.abs(want)), 1e-12, p)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the batch axis past 65535 problems
# ---------------------------------------------------------------------------------------------------------------------

def test_narrow_leave_one_out_past_65535_problems():
    """B = 65537 problems of width 1 ((1, 0), N = 128, 4 chunks), 64 distinct ones tiled over the batch: every problem
    equals its twin in a plan of the 64, bit for bit, and the 64 meet the oracle."""
    JR, JC, N, BIG, DISTINCT = 1, 0, 128, 65537, 64
    small = synthetic(DISTINCT, N, JR, JC, "bench", seed=7)
    idx = np.arange(BIG) % DISTINCT
    big = {k: v[idx] for k, v in small.items()}
    res = []
    for case in (big, small):
        plan = narrow_plan(case, JR, JC, "reference", chunks=4, expect=None)
        try:
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            res.append(plan.leave_one_out())
        finally:
            plan.close()
    assert res[0].kinv_diag.shape == (BIG, N)
    for field in ("kinv_diag", "alpha", "logpdf", "status"):
        assert np.array_equal(getattr(res[0], field), getattr(res[1], field)[idx]), field
    check_all("B = 65537, narrow plan (width 1): the 64 distinct problems", res[1], *oracle_of(small), NARROW)


# ---------------------------------------------------------------------------------------------------------------------
# 7. sharded
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC,N", [(2, 3, 600), (4, 4, 512)])
def test_sharded_leave_one_out_equals_the_unsharded_plan(JR, JC, N):
    """1 / 2 / 3 shards on the visible devices: every shard on its slice of each output, no collective -- the bits of the
    unsharded plan in all outputs."""
    B = 7
    narrow = JR + 2 * JC <= 8
    case = synthetic(B, N, JR, JC, "bench", seed=31 + JC)
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        if narrow:
            plan.set_chunks(16)
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        want, want_c, want_small = plan.leave_one_out(), plan.inverse_diagonal(), plan.leave_one_out(arrays=False)
    finally:
        plan.close()
    ndev = batch.device_count()
    for S in (1, 2, 3):
        sp = batch.ShardedBatchedGP(B, N, JR, JC, devices=[s % ndev for s in range(S)])
        try:
            if narrow:
                sp.set_chunks(16)
            sp.set_series(case["t"], case["diag"], case["y"])
            sp.set_coefficients(*coeffs_of(case))
            assert (sp.materialize()[3] == 0).all()
            got, got_c, got_small = sp.leave_one_out(), sp.inverse_diagonal(), sp.leave_one_out(arrays=False)
        finally:
            sp.close()
        for field in batch.LeaveOneOut._fields:
            assert np.array_equal(getattr(got, field), getattr(want, field)), (S, field)
        assert np.array_equal(got_c, want_c) and np.array_equal(got_c, want.kinv_diag), S
        assert np.array_equal(got_small.logpdf, want_small.logpdf) and np.array_equal(got_small.logpdf, want.logpdf), S
    check_all("sharded leave_one_out (width %d), the unsharded plan" % (JR + 2 * JC), want, *oracle_of(case), NARROW if narrow else WIDE)


# ---------------------------------------------------------------------------------------------------------------------
# 8. a batch with a refused problem
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC,N", [(2, 3, 700), (4, 4, 512)])
def test_leave_one_out_beside_a_refused_problem(JR, JC, N):
    """One problem in the middle is not positive definite (status 2): the statuses equal the oracle's, its row is NaN in
    every output and the other problems meet the bar."""
    B = 5
    narrow = JR + 2 * JC <= 8
    case = synthetic(B, N, JR, JC, "bench", seed=1000 + N % 97 + 3 * JR + JC)
    mid = B // 2
    case["a_real"][mid] *= -40.0
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        if narrow:
            plan.set_chunks(24)
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        st = plan.log_likelihood(materialize=True)[3]
        loo = plan.leave_one_out()
        small = plan.leave_one_out(arrays=False)
    finally:
        plan.close()
    s0 = ref.batch_log_likelihood(0.0, *coeffs_of(case), case["t"], case["diag"], case["y"])[3]
    assert np.array_equal(st, s0) and st[mid] == 2 and (np.delete(st, mid) == 0).all()
    assert np.array_equal(loo.status, s0) and np.array_equal(small.status, s0)
    for field in ("residual", "variance", "kinv_diag", "alpha"):
        assert np.isnan(getattr(loo, field)[mid]).all(), field
    assert np.isnan(loo.logpdf[mid]) and np.isnan(small.logpdf[mid])
    assert np.array_equal(np.delete(small.logpdf, mid), np.delete(loo.logpdf, mid))
    c0, a0 = oracle_of(case, skip=(mid,))
    check_all("leave_one_out beside a refused problem (width %d)" % (JR + 2 * JC), loo, c0, a0, NARROW if narrow else WIDE, skip=(mid,))


# ---------------------------------------------------------------------------------------------------------------------
# 9. argument errors
# ---------------------------------------------------------------------------------------------------------------------

def test_leave_one_out_argument_errors_leave_the_plan_usable():
    """All outputs NULL, or no materialising run yet: an error status and no numbers; the plan evaluates normally
    afterwards."""
    JR, JC = 2, 3
    case = synthetic(NARROW_B, NARROW_N, JR, JC, "bench", seed=3)
    lib = batch._load()
    plan = narrow_plan(case, JR, JC, "reference")
    try:
        with pytest.raises(RuntimeError):
            plan.inverse_diagonal()                     # no materialising run has been made
        with pytest.raises(RuntimeError):
            plan.leave_one_out(arrays=False)
        assert lib.clr_batch_leave_one_out(plan._h, None, None, None, None) != 0
        ll, _, _, st = plan.log_likelihood(materialize=True)
        assert (st == 0).all()
        with pytest.raises(RuntimeError, match="invalid argument"):
            batch._check(lib.clr_batch_leave_one_out(plan._h, None, None, None, None))
        c = plan.inverse_diagonal()
        ll2 = plan.log_likelihood()[0]
    finally:
        plan.close()
    ll0 = ref.batch_log_likelihood(0.0, *coeffs_of(case), case["t"], case["diag"], case["y"])[0]
    assert np.max(np.abs(ll - ll0) / np.abs(ll0)) < 1e-10 and np.max(np.abs(ll2 - ll0) / np.abs(ll0)) < 1e-10
    check_c("inverse_diagonal after the argument errors", c, oracle_of(case)[0], NARROW)
