# -*- coding: utf-8 -*-
"""`-m gpu`: the conditional variance of ``GP.predict`` on batched plans -- ``BatchedGP.predict(xs, return_var=True)``,
``clr_batch_predict_var`` -- at every narrow kernel shape in both factor layouts, in every bucket of the wide sweep,
across tile sizes, past 65535 problems and sharded, against the CPU oracle.

The oracle value per problem and point is the reference's own formula (celerite.py:465-470) on the oracle's factor:
``k(0) - sum k* o RefSolver.solve(k*)`` with ``k*`` from a NumPy evaluation of the kernel.

Bar: ``max |var_dev - var_oracle| <= 1e-10 k(0)`` -- the project's PREDICT bar (1e-10 of the largest entry); k(0)
bounds the variance, and is the scale because on the bench family the variance at and between data points falls to
about 6e-4 of k(0).  Measured on the CPU, the double oracle is <= 7e-15 k(0) from a binary128 evaluation (N = 700;
(2,3), (1,0), (0,4), (1,15); both families), four orders inside the bar.  Device and oracle are also recorded against
binary128 (``ref.quad_factor_solve`` on ``k*``) side by side on problem 0 of the accuracy-family cases."""
import numpy as np
import pytest

from celerite_amd import batch
from oracle import ref
from _cases import ALL_WIDTH_SHAPES, CONSUMER_WIDE_SHAPES, synthetic, coeffs_of, within

pytestmark = pytest.mark.gpu

PREDICT = 1e-10
NOGEN = (np.empty(0), np.empty((0, 0)), np.empty((0, 0)))
FAST_TRIG_LIMIT = 1.0e9        # CLR_FAST_TRIG_LIMIT (csrc/clr_core.h)
# At t ~ 3e8 the phase d t rounded to double is off by up to half an ulp of 1.5e9 (1.2e-7 rad) from the phase binary128
# carries: device and double oracle share that rounding (the same fl(d t)) -- a relative error of up to 2.4e-7 in the
# entries of K between two samples, so of that order times k(0) in the quadratic form.  There the two binary128 records
# are held to 1e-6 (the bar test_gpu_batch_consumers.py keeps for the same inputs); device vs oracle stays 1e-10.
PHASE_ROUNDING = 1e-6
TRUTH_POINTS = {False: 0, True: 6, "wide": 2}   # points of problem 0 attributed against binary128: each one refactors in
                                                # binary128 (20 ms at width 8, N = 700; 2 s at width 64, N = 2048)


def kernel_value(case, p, tau):
    """k_p(tau) by the six-coefficient formula (terms.py: RealTerm / ComplexTerm get_value)."""
    ar, cr, ac, bc, cc, dc = coeffs_of(case, p)
    tau = np.abs(np.asarray(tau, dtype=float))[..., None]
    return np.sum(ar * np.exp(-cr * tau), axis=-1) + np.sum(np.exp(-cc * tau) * (ac * np.cos(dc * tau) + bc * np.sin(dc * tau)), axis=-1)


def k_zero(case, p):
    return float(np.sum(case["a_real"][p]) + np.sum(case["a_comp"][p]))


def oracle_solver(case, p):
    r = ref.RefSolver()
    try:
        r.compute(0.0, *coeffs_of(case, p), *NOGEN, case["t"][p], case["diag"][p])
    except ref.RefLinAlgError:
        return None
    return r


def oracle_var(case, p, pts, r=None):
    """(var[M], k*[N, M]) of problem p at its points."""
    r = r or oracle_solver(case, p)
    kstar = kernel_value(case, p, pts[None, :] - case["t"][p][:, None])
    return k_zero(case, p) - np.sum(kstar * r.solve(kstar), axis=0), kstar


def points_of(pts, p):
    return pts[p] if pts.ndim == 2 else pts


def check_against_oracle(tag, case, pts, var, truth=False, skip=(), truth_bar=PREDICT):
    """Every problem but ``skip`` against the oracle under the bar; ``truth``: device and oracle of problem 0 against
    binary128 at TRUTH_POINTS[truth] of its points, side by side under ``truth_bar``."""
    B = case["t"].shape[0]
    assert var.shape == (B, pts.shape[-1])
    for p in range(B):
        if p in skip:
            continue
        x = points_of(pts, p)
        want, kstar = oracle_var(case, p, x)
        k0 = k_zero(case, p)
        dev = np.max(np.abs(var[p] - want)) / k0
        print("%s: problem %d, max |var - oracle| / k(0) = %.3e" % (tag, p, dev))
        within(tag + ": var vs oracle, of k(0)", dev, PREDICT, p)
        if truth and p == 0:
            idx = np.unique(np.linspace(0, len(x) - 1, TRUTH_POINTS[truth] + 2).astype(int)[1:-1])   # (inside the series)
            vq = np.array([k0 - kstar[:, m] @ ref.quad_factor_solve(0.0, *coeffs_of(case, 0), case["t"][0], case["diag"][0],
                                                                     kstar[:, m], want_factor=False)[2] for m in idx])
            within(tag + ": device var vs binary128, of k(0)", np.max(np.abs(var[0][idx] - vq)) / k0, truth_bar)
            within(tag + ": double oracle var vs binary128, of k(0)", np.max(np.abs(want[idx] - vq)) / k0, truth_bar)


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


# ---------------------------------------------------------------------------------------------------------------------
# 1. narrow plans (widths 1..8) at every (J_real, J_comp) shape, both factor layouts
# ---------------------------------------------------------------------------------------------------------------------

NARROW_B, NARROW_N, NARROW_CHUNKS = 4, 700, (22, 32)    # set_chunks(24): chunks of 32 samples, the last one 28


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


@pytest.mark.parametrize("layout", ["reference", "lean"])
@pytest.mark.parametrize("JR,JC", ALL_WIDTH_SHAPES)
def test_narrow_predict_var_at_every_shape(JR, JC, layout):
    """The narrow kernels are compiled per (J_real, J_comp), factor layout and trig flavour
    (``bpredvar_*`` in csrc/clr_bpredvar_kernels.h, instantiated through csrc/clr_batch_kernels.h): all 24 shapes, both
    layouts, both families, 22 chunks with a ragged last one.  Shared, per-problem and unsorted points; a mean in force
    does not enter the variance."""
    B, N = NARROW_B, NARROW_N
    for family in ("bench", "accuracy"):
        case = synthetic(B, N, JR, JC, family, seed=500 + 9 * JC + JR)
        shared, own, perm = prediction_points(case, np.random.RandomState(40 + JR + 7 * JC))
        plan = narrow_plan(case, JR, JC, layout)
        try:
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            mu, var = plan.predict(shared, return_var=True)
            var_own = plan.predict(own, return_var=True)[1]
            var_perm = plan.predict(shared[perm], return_var=True)[1]
            plan.set_mean(np.linspace(-1.0, 2.0, B))
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            mu_m, var_m = plan.predict(shared, return_var=True)
        finally:
            plan.close()
        tag = "narrow predict_var (%s layout, %s family)" % (layout, family)
        assert np.array_equal(var_perm, var[:, perm]), tag
        assert np.array_equal(var_m, var) and not np.array_equal(mu_m, mu), tag
        check_against_oracle(tag + ", shared points", case, shared, var, truth=family == "accuracy")
        check_against_oracle(tag + ", per-problem points", case, own, var_own)


# ---------------------------------------------------------------------------------------------------------------------
# 2. tiles
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC,layout", [(2, 3, "lean"), (1, 10, None)])
def test_predict_var_does_not_depend_on_the_tile(JR, JC, layout):
    """Tiles of 1, of 7 (M = 40: a ragged last tile) and the automatic tile give the same bits; the mean is what
    ``predict(xs)`` returns, before and after."""
    B, N, M = 3, 2048, 40
    case = synthetic(B, N, JR, JC, "accuracy", seed=21 + JC)
    rng = np.random.RandomState(3)
    xs = np.sort(rng.uniform(case["t"].min() - 10.0, case["t"].max() + 10.0, M))
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        if layout:
            plan.set_factor_layout(layout)
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        before = plan.predict(xs)
        got = {}
        for tile in (1, 7, 0):
            plan.set_predict_tile(tile)
            got[tile] = plan.predict(xs, return_var=True)
        after = plan.predict(xs)
    finally:
        plan.close()
    for tile in (1, 7, 0):
        assert np.array_equal(got[tile][0], before) and np.array_equal(got[tile][1], got[0][1]), tile
    assert np.array_equal(after, before)
    check_against_oracle("predict_var across tiles (width %d)" % (JR + 2 * JC), case, xs, got[0][1], truth=True if layout else "wide")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the library-trig instantiations
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC", [(2, 3), (1, 1)])
def test_narrow_predict_var_on_the_library_trig_kernels(JR, JC):
    """A series offset to t ~ 3e8: max|d| max|t| >= CLR_FAST_TRIG_LIMIT, so the lean plan regenerates phi, u with the
    library sincos (``bpredvar_go<true, false>``) and the cross-covariances take it too.  Against the oracle, and the
    lean layout against the reference layout of the same plan (stored phi, u: no trigonometry) within 1e-12 k(0).
    Device and oracle of problem 0 are recorded against binary128 side by side under PHASE_ROUNDING: the rounding of
    the phase d t at t ~ 3e8 is a property of the inputs that both share."""
    B, N = NARROW_B, NARROW_N
    case = synthetic(B, N, JR, JC, "accuracy", seed=77 + JR)
    case["t"] = case["t"] + 3.0e8
    shared, own, perm = prediction_points(case, np.random.RandomState(91))
    out = {}
    for layout in ("lean", "reference"):
        plan = narrow_plan(case, JR, JC, layout)
        try:
            bounds = plan.selection_bounds()
            assert bounds["dmax"] * bounds["tmax"] >= FAST_TRIG_LIMIT, bounds
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            out[layout] = plan.predict(shared, return_var=True)[1]
        finally:
            plan.close()
        check_against_oracle("narrow predict_var, library trig (%s layout)" % layout, case, shared, out[layout],
                             truth=True, truth_bar=PHASE_ROUNDING)
    for p in range(B):
        within("narrow predict_var, library trig: lean vs reference layout, of k(0)",
               np.max(np.abs(out["lean"][p] - out["reference"][p])) / k_zero(case, p), 1e-12, p)


# ---------------------------------------------------------------------------------------------------------------------
# 4. wide plans (widths 9..64) in every bucket of launch_wsweep_scan
# ---------------------------------------------------------------------------------------------------------------------

def wide_var(case, JR, JC, xs):
    B, N = case["t"].shape
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        st = plan.log_likelihood(materialize=True)[3]
        return st, plan.predict(xs, return_var=True)[1]
    finally:
        plan.close()


@pytest.mark.parametrize("N,family", [(512, "bench"), (2048, "accuracy")])
@pytest.mark.parametrize("JR,JC", CONSUMER_WIDE_SHAPES)
def test_wide_predict_var_in_every_sweep_bucket(JR, JC, N, family):
    B, M = 3, 25
    case = synthetic(B, N, JR, JC, family, seed=1000 + N % 97 + 3 * JR + JC)
    lo, hi = case["t"].min(), case["t"].max()
    xs = np.sort(np.random.RandomState(5 + JC).uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), M))
    st, var = wide_var(case, JR, JC, xs)
    assert (st == 0).all()
    check_against_oracle("wide predict_var (width %d, N = %d)" % (JR + 2 * JC, N), case, xs, var,
                         truth="wide" if family == "accuracy" else False)


@pytest.mark.parametrize("JR,JC", CONSUMER_WIDE_SHAPES)
def test_wide_predict_var_refuses_a_series_shorter_than_512(JR, JC):
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
        import ctypes as C
        lib.clr_batch_predict_var.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_long, C.POINTER(C.c_double)]
        xs = np.ascontiguousarray(case["t"][0, ::7])
        var = np.empty((B, len(xs)))
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            batch._check(lib.clr_batch_predict_var(plan._h, len(xs), batch._ptr(xs), 0, batch._ptr(var)))
        got_L = plan.dot_L(z)
    finally:
        plan.close()
    for p in range(B):
        want = oracle_solver(case, p).dot_L(z[p])[:, 0]
        within("wide plan at N = 511 after the refusal: dot_L vs oracle, of the largest entry",
               np.max(np.abs(got_L[p] - want)) / np.max(np.abs(want)), 1e-12, p)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the batch axis past 65535 problems
# ---------------------------------------------------------------------------------------------------------------------

def test_narrow_predict_var_past_65535_problems():
    """B = 65537 problems of width 1 ((1, 0), N = 128, 4 chunks), 64 distinct ones tiled over the batch, M = 2: every
    problem equals its twin in a plan of the 64, bit for bit, and the 64 meet the oracle.  The wide path at that size
    needs about 8 GB (the reference layout's factor of 65537 x 512 x 9 doubles, three times) and is not run here."""
    JR, JC, N, BIG, DISTINCT = 1, 0, 128, 65537, 64
    small = synthetic(DISTINCT, N, JR, JC, "bench", seed=7)
    idx = np.arange(BIG) % DISTINCT
    big = {k: v[idx] for k, v in small.items()}
    xs = np.array([0.31, 1.02])
    res = []
    for case in (big, small):
        plan = narrow_plan(case, JR, JC, "reference", chunks=4, expect=None)
        try:
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            res.append(plan.predict(xs, return_var=True)[1])
        finally:
            plan.close()
    assert res[0].shape == (BIG, 2) and np.array_equal(res[0], res[1][idx])
    check_against_oracle("B = 65537, narrow plan (width 1): the 64 distinct problems", small, xs, res[1])


# ---------------------------------------------------------------------------------------------------------------------
# 6. sharded
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC,N", [(2, 3, 600), (4, 4, 512)])
def test_sharded_predict_var_equals_the_unsharded_plan(JR, JC, N):
    """1 / 2 / 3 shards on one device: every shard on its slice of xs and var, no collective -- the same bits as the
    unsharded plan, shared and per-problem points."""
    B = 7
    narrow = JR + 2 * JC <= 8
    case = synthetic(B, N, JR, JC, "bench", seed=31 + JC)
    rng = np.random.RandomState(6)
    own = np.sort(rng.uniform(-0.05, 1.05, (B, 9)), axis=1)
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        if narrow:
            plan.set_chunks(16)
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        want = plan.predict(own, return_var=True), plan.predict(own[0], return_var=True)
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
            got = sp.predict(own, return_var=True), sp.predict(own[0], return_var=True)
        finally:
            sp.close()
        for g, w in zip(got, want):
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), S
    check_against_oracle("sharded predict_var (width %d), the unsharded plan" % (JR + 2 * JC), case, own, want[0][1])


# ---------------------------------------------------------------------------------------------------------------------
# 7. a batch with a refused problem
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC,N", [(2, 3, 700), (4, 4, 512)])
def test_predict_var_beside_a_refused_problem(JR, JC, N):
    """One problem in the middle is not positive definite (status 2): the statuses equal the oracle's and the other
    problems meet the bar."""
    B, M = 5, 12
    case = synthetic(B, N, JR, JC, "bench", seed=1000 + N % 97 + 3 * JR + JC)
    mid = B // 2
    case["a_real"][mid] *= -40.0
    xs = np.sort(np.random.RandomState(2).uniform(-0.05, 1.05, M))
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        if JR + 2 * JC <= 8:
            plan.set_chunks(24)
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        st = plan.log_likelihood(materialize=True)[3]
        var = plan.predict(xs, return_var=True)[1]
    finally:
        plan.close()
    s0 = ref.batch_log_likelihood(0.0, *coeffs_of(case), case["t"], case["diag"], case["y"])[3]
    assert np.array_equal(st, s0) and st[mid] == 2 and (np.delete(st, mid) == 0).all()
    check_against_oracle("predict_var beside a refused problem (width %d)" % (JR + 2 * JC), case, xs, var, skip=(mid,))
