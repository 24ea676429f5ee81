# -*- coding: utf-8 -*-
"""`-m gpu`: the batched consumers of a plan -- ``clr_batch_solve``, ``clr_batch_dot_L`` (and ``BatchedGP.sample`` on
it), ``clr_batch_dot`` and ``clr_batch_predict`` -- at every narrow kernel shape, in every instantiation bucket of the
wide sweeps and past 65535 problems, against the CPU oracle (``oracle.ref.RefSolver``) problem by problem.

Bars (those of the consumer tests in test_gpu_batch.py): narrow solve 1e-10 and wide solve 2e-11 of the largest entry,
``dot_L`` and ``dot`` 1e-12 of the largest entry, ``predict`` 1e-10 of the largest entry; statuses equal the oracle's.
Solves of the accuracy family are also attributed against the reference recurrence carried in binary128
(``ref.quad_factor_solve``): device and double oracle, each against that truth, side by side."""
import os

import numpy as np
import pytest

from celerite_amd import batch
from oracle import ref
from _cases import ALL_WIDTH_SHAPES, CONSUMER_WIDE_SHAPES, synthetic, coeffs_of, within, edge_points

pytestmark = pytest.mark.gpu

NARROW_SOLVE, WIDE_SOLVE, DOT, PREDICT = 1e-10, 2e-11, 1e-12, 1e-10
NOGEN = (np.empty(0), np.empty((0, 0)), np.empty((0, 0)))
FAST_TRIG_LIMIT = 1.0e9        # CLR_FAST_TRIG_LIMIT (csrc/clr_core.h): above it the kernels take the library sincos
# At t ~ 3e8 the phase d t rounded to double is off by up to half an ulp of 1.5e9 (1.2e-7 rad) from the phase binary128
# carries: device and double oracle share that rounding (the same fl(d t)) and sit about 1e-8 of the largest entry from
# the binary128 solve, side by side.  The device-vs-oracle bar stays 1e-10.
PHASE_ROUNDING = 1e-6
# dot_L of a long dense wide series (N = 20000, bench family) rests on a factor whose own rounding reaches 6e-12 of W
# and 1e-11 of D in the double oracle (against binary128).  At width 33 the device's dot_L is 1.4e-12 of the largest
# entry from the oracle's, and the binary128 record puts that on the oracle: 7.7e-13 from dot_L on the binary128 factor,
# the device 1.8e-13.  There the device-vs-oracle bar is 5e-12, and both are recorded against dot_L on the binary128
# factor, side by side.
WIDE_DOT_L_LONG = 5e-12


def of_largest(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def oracle_solver(case, p, jitter=0.0):
    """The oracle's factor of problem ``p``; None where the reference throws (not positive definite)."""
    r = ref.RefSolver()
    try:
        r.compute(jitter, *coeffs_of(case, p), *NOGEN, case["t"][p], case["diag"][p])
    except ref.RefLinAlgError:
        return None
    return r


def prediction_points(case, rng, M_shared=300, M_own=200, M_shuffled=150):
    """Points shared by all problems, points per problem and unsorted points -- all reaching past the series on both
    sides.  Unsorted points only on the dense bench family: the reference's walk over unsorted points multiplies by
    exp(c (x_prev - x)), which overflows on the sparse accuracy family's spans (the oracle returns NaN there)."""
    B = case["t"].shape[0]
    lo, hi = case["t"].min(), case["t"].max()
    pad = 0.05 * (hi - lo)
    shared = np.sort(np.concatenate([rng.uniform(lo - pad, hi + pad, M_shared), [lo - pad, hi + pad], case["t"][0, ::97]]))
    own = np.sort(np.concatenate([rng.uniform(lo - pad, hi + pad, (B, M_own)),
                                  np.tile([lo - 2 * pad, hi + 2 * pad], (B, 1))], axis=1), axis=1)
    shuffled = rng.permutation(shared)[:M_shuffled]
    assert shared[0] < lo and shared[-1] > hi and (own[:, 0] < lo).all() and (own[:, -1] > hi).all()
    assert np.any(np.diff(shuffled) < 0)
    if hi - lo > 10.0:
        return {"shared": shared, "own": own}
    return {"shared": shared, "own": own, "shuffled": shuffled}


def run_consumers(plan, case, rhs, points, jitter):
    """Every consumer of ``plan`` after one materialising run (the factor's consumers first, ``dot`` last: it needs the
    per-problem ``jitter`` in force)."""
    out = {}
    out["ll"] = plan.log_likelihood(materialize=True)
    out["solve y"] = plan.solve()
    out["solve 1"] = plan.solve(rhs["b1"])
    out["solve 3"] = plan.solve(rhs["b3"])
    out["dot_L 1"] = plan.dot_L(rhs["z1"])
    out["dot_L 3"] = plan.dot_L(rhs["z3"])
    out["sample"] = plan.sample(size=2, mean=case["y"], random=np.random.RandomState(5))
    for key, pts in points.items():
        out["predict " + key] = plan.predict(pts)
    plan.set_coefficients(*coeffs_of(case), jitter=jitter)
    out["dot 3"] = plan.dot(rhs["z3"])
    plan.set_coefficients(*coeffs_of(case))
    return out


def dot_L_on(phi, u, W, D, z):
    """``dot_L`` (cholesky.h:421-427, oracle/celerite_ref.c: ref_dot_L) on a given factor, carried in long double;
    ``z``: (N, nrhs)."""
    ld = np.longdouble
    phi, u, W, sD, z = phi.astype(ld), u.astype(ld), W.astype(ld), np.sqrt(D.astype(ld)), z.astype(ld)
    y = np.empty(z.shape, ld)
    f = np.zeros((W.shape[0], z.shape[1]), ld)
    tmp = z[0] * sD[0]
    y[0] = tmp
    for n in range(1, len(D)):
        f = phi[:, n - 1, None] * (f + W[:, n - 1, None] * tmp)
        tmp = sD[n] * z[n]
        y[n] = tmp + u[:, n - 1] @ f
    return y.astype(np.float64)


def check_against_oracle(tag, case, rhs, points, jitter, out, solve_bar, truth_bar=None, dot_L_bar=DOT):
    """Problem by problem against the oracle; statuses exactly.  ``truth_bar``: also record the device's solve(y) and
    the double oracle's, each against the binary128 recurrence, side by side.  ``dot_L_bar`` above 1e-12: also record
    problem 0's dot_L, device and double oracle, against dot_L on the binary128 factor.  Returns the problems the oracle
    refuses."""
    B, N = case["t"].shape
    ll, ld, q, st = out["ll"]
    s0 = ref.batch_log_likelihood(0.0, *coeffs_of(case), case["t"], case["diag"], case["y"])[3]
    assert np.array_equal(st, s0), (tag, st, s0)
    again = out["sample"] - case["y"][:, None, :]
    refused = []
    for p in range(B):
        r = oracle_solver(case, p)
        if r is None:
            assert st[p] == 2
            refused.append(p)
        else:
            assert st[p] == 0
            want_y = r.solve(case["y"][p])[:, 0]
            within(tag + ": solve(y) vs oracle solve, of the largest entry", of_largest(out["solve y"][p], want_y), solve_bar, p)
            within(tag + ": solve, one rhs, vs oracle solve, of the largest entry",
                   of_largest(out["solve 1"][p], r.solve(rhs["b1"][p])[:, 0]), solve_bar, p)
            within(tag + ": solve, three rhs, vs oracle solve, of the largest entry",
                   of_largest(out["solve 3"][p].T, r.solve(rhs["b3"][p].T)), solve_bar, p)
            want_L3 = r.dot_L(rhs["z3"][p].T)
            normals = np.random.RandomState(5).standard_normal((B, 2, N))[p].T
            within(tag + ": dot_L, one rhs, vs oracle dot_L, of the largest entry",
                   of_largest(out["dot_L 1"][p], r.dot_L(rhs["z1"][p])[:, 0]), dot_L_bar, p)
            within(tag + ": dot_L, three rhs, vs oracle dot_L, of the largest entry", of_largest(out["dot_L 3"][p].T, want_L3), dot_L_bar, p)
            within(tag + ": sample - mean vs oracle dot_L of the same normals, of the largest entry",
                   of_largest(again[p].T, r.dot_L(normals)), dot_L_bar, p)
            if dot_L_bar > DOT and p == 0:
                Wq, Dq = ref.quad_factor_solve(0.0, *coeffs_of(case, p), case["t"][p], case["diag"][p], case["y"][p])[:2]
                _, _, _, _, phi, u, _, _ = r.state()
                z5 = np.column_stack([rhs["z3"][p].T, normals])          # (the three right-hand sides and sample's normals)
                truth = dot_L_on(phi, u, Wq, Dq, z5)
                within(tag + ": device dot_L vs dot_L on the binary128 factor, of the largest entry",
                       of_largest(np.column_stack([out["dot_L 3"][p].T, again[p].T]), truth), dot_L_bar, p)
                within(tag + ": double oracle dot_L vs dot_L on the binary128 factor, of the largest entry",
                       of_largest(r.dot_L(z5), truth), dot_L_bar, p)
            for key, pts in points.items():
                pts_p = pts[p] if pts.ndim == 2 else pts
                within(tag + ": predict (%s points) vs oracle predict, of the largest" % key,
                       of_largest(out["predict " + key][p], r.predict(case["y"][p], pts_p)), PREDICT, p)
            if truth_bar is not None:
                xq = ref.quad_factor_solve(0.0, *coeffs_of(case, p), case["t"][p], case["diag"][p], case["y"][p],
                                           want_factor=False)[2]
                within(tag + ": device solve(y) vs binary128 truth, of the largest entry", of_largest(out["solve y"][p], xq), truth_bar, p)
                within(tag + ": double oracle solve(y) vs binary128 truth, of the largest entry", of_largest(want_y, xq), truth_bar, p)
        want_dot = ref.RefSolver().dot(jitter[p], *coeffs_of(case, p), *NOGEN, case["t"][p], rhs["z3"][p].T)
        within(tag + ": dot (a jitter per problem), three rhs, vs oracle dot, of the largest entry",
               of_largest(out["dot 3"][p].T, want_dot), DOT, p)
    return refused


def make_rhs(B, N, seed):
    rng = np.random.RandomState(seed)
    return rng, {"b1": rng.randn(B, N), "b3": rng.randn(B, 3, N), "z1": rng.randn(B, N), "z3": rng.randn(B, 3, N)}


# ---------------------------------------------------------------------------------------------------------------------
# 1. narrow consumers (widths 1..8) at every (J_real, J_comp) shape, both factor layouts
# ---------------------------------------------------------------------------------------------------------------------

NARROW_B, NARROW_N, NARROW_CHUNKS = 4, 700, (22, 32)    # set_chunks(24): chunks of 32 samples, the last one 28


def narrow_plan(case, JR, JC, layout):
    B, N = case["t"].shape
    plan = batch.BatchedGP(B, N, JR, JC)
    plan.set_chunks(24)
    assert plan.chunks == NARROW_CHUNKS and N % NARROW_CHUNKS[1] != 0      # a ragged last chunk, not an even split
    plan.set_factor_layout(layout)
    plan.set_series(case["t"], case["diag"], case["y"])
    plan.set_coefficients(*coeffs_of(case))
    return plan


@pytest.mark.parametrize("layout", ["reference", "lean"])
@pytest.mark.parametrize("JR,JC", ALL_WIDTH_SHAPES)
def test_narrow_consumers_at_every_shape(JR, JC, layout):
    """The narrow consumers are compiled per (J_real, J_comp), factor layout and trig flavour
    (``bsolve_*``, ``bdotl_*``, ``bdot_*`` in csrc/clr_batch_kernels.h): every one of the 24 shapes of widths 1..8 in
    both layouts, on both synthetic families, 22 chunks with a ragged last one.  ``solve`` with the plan's y, one and three
    uploaded right-hand sides; ``dot_L`` with one and three; ``sample``; ``dot`` with a jitter per problem; ``predict`` at
    shared, per-problem and unsorted points reaching past both ends of the series.  The accuracy family's solves are
    attributed against binary128."""
    B, N = NARROW_B, NARROW_N
    for family in ("bench", "accuracy"):
        case = synthetic(B, N, JR, JC, family, seed=500 + 9 * JC + JR)
        rng, rhs = make_rhs(B, N, 40 + JR + 7 * JC)
        points = prediction_points(case, rng)
        jitter = rng.uniform(0.0, 0.5, B)
        plan = narrow_plan(case, JR, JC, layout)
        try:
            out = run_consumers(plan, case, rhs, points, jitter)
        finally:
            plan.close()
        refused = check_against_oracle("narrow consumers (%s layout, %s family)" % (layout, family), case, rhs, points,
                                       jitter, out, NARROW_SOLVE,
                                       truth_bar=NARROW_SOLVE if family == "accuracy" else None)
        assert not refused


@pytest.mark.parametrize("JR,JC", [(2, 3), (1, 1)])
def test_narrow_consumers_on_the_library_trig_kernels(JR, JC):
    """A dense series offset to t ~ 3e8: max|d| max|t| >= CLR_FAST_TRIG_LIMIT, so the plan runs the library-sincos
    instantiations -- ``bsolve_go<true, false>`` and ``bdotl_go<true, false>`` on the lean factor, ``bdot`` with
    ``FAST = false`` -- which no other consumer test reaches.  Against the oracle, and the lean factor's consumers
    against the reference layout's of the same plan (stored phi, u: no trigonometry)."""
    B, N = NARROW_B, NARROW_N
    case = synthetic(B, N, JR, JC, "accuracy", seed=77 + JR)
    case["t"] = case["t"] + 3.0e8
    assert (np.diff(case["t"], axis=1) >= 0).all()
    rng, rhs = make_rhs(B, N, 91)
    points = prediction_points(case, rng)
    jitter = rng.uniform(0.0, 0.5, B)
    outs = {}
    for layout in ("lean", "reference"):
        plan = narrow_plan(case, JR, JC, layout)
        try:
            bounds = plan.selection_bounds()
            assert bounds["dmax"] * bounds["tmax"] >= FAST_TRIG_LIMIT, bounds
            outs[layout] = run_consumers(plan, case, rhs, points, jitter)
        finally:
            plan.close()
        check_against_oracle("narrow consumers, library trig (%s layout)" % layout, case, rhs, points, jitter, outs[layout],
                             NARROW_SOLVE, truth_bar=PHASE_ROUNDING)
    for key in outs["lean"]:
        if key == "ll":
            for a, b in zip(outs["lean"][key], outs["reference"][key]):
                assert np.array_equal(a, b)
        else:
            within("narrow consumers, library trig: lean vs reference layout of the same plan, of the largest entry",
                   of_largest(outs["lean"][key], outs["reference"][key]), DOT, key)


# the entries that claim a plan's cached factor state (the chunk maps, the start states of S, the start matrices Q), each
# as the FIRST call after a materialising run; `x`, `phi`: per-problem unsorted points and the mean's basis there
FIRST_CALLS = {
    "solve": lambda plan, x, phi: plan.solve(),
    "predict var (solve route)": lambda plan, x, phi: plan.predict(x, return_var=True, mean_basis=phi),
    "predict var (recurrence)": lambda plan, x, phi: plan.predict(x, return_var=True, mean_basis=phi, method="recurrence"),
    "inverse_diagonal": lambda plan, x, phi: plan.inverse_diagonal(),
    "one_step_ahead": lambda plan, x, phi: plan.one_step_ahead(),
    "forecast var": lambda plan, x, phi: plan.forecast(x, return_var=True, mean_basis=phi),
    "predict_terms var": lambda plan, x, phi: plan.predict_terms(x, return_var=True),
    "fit_mean_weights": lambda plan, x, phi: plan.fit_mean_weights(),
}
# ... and what runs after it on the same plan, in this order
FOLLOWERS = [
    ("solve", FIRST_CALLS["solve"]),
    ("predict var (recurrence)", FIRST_CALLS["predict var (recurrence)"]),
    ("forecast var", FIRST_CALLS["forecast var"]),
    ("leave_one_out", lambda plan, x, phi: plan.leave_one_out()),
    ("predict_terms var", FIRST_CALLS["predict_terms var"]),
]
_CALL_ORDER = {}


def call_order_case(layout):
    """The case, its points and -- computed once per layout -- what a fresh plan returns for each follower alone."""
    if layout not in _CALL_ORDER:
        JR, JC = 2, 3
        case = synthetic(NARROW_B, NARROW_N, JR, JC, "bench", seed=613)
        rng = np.random.RandomState(29)
        own = edge_points(case, rng, own=12)[1]
        own = own[:, rng.permutation(own.shape[1])]          # before t_0, at samples and past t_{N-1}, unsorted
        assert np.any(np.diff(own, axis=1) < 0) and (own.min(axis=1) < case["t"][:, 0]).all()
        assert (own.max(axis=1) > case["t"][:, -1]).all() and all(case["t"][p, 0] in own[p] for p in range(NARROW_B))
        phi = np.ones((1, own.shape[1]))
        alone = {}
        for name, call in FOLLOWERS:
            plan = call_order_plan(case, layout)
            try:
                alone[name] = arrays_of(call(plan, own, phi))
            finally:
                plan.close()
        _CALL_ORDER[layout] = (case, own, phi, alone)
    return _CALL_ORDER[layout]


def call_order_plan(case, layout):
    """A materialised plan under a one-column basis with weights zero: the residual is y exactly, and the fit can run."""
    plan = narrow_plan(case, 2, 3, layout)
    plan.set_mean_basis(np.ones((1, NARROW_N)))
    st = plan.log_likelihood(materialize=True)[3]
    assert (st == 0).all(), st
    return plan


def arrays_of(out):
    return [out] if isinstance(out, np.ndarray) else [np.asarray(a) for a in out]


@pytest.mark.parametrize("first", sorted(FIRST_CALLS))
@pytest.mark.parametrize("layout", ["reference", "lean"])
def test_cached_factor_state_whoever_claims_it_first(layout, first):
    """The chunk maps, the forward start states of S and the backward start matrices Q depend on the factor only and are
    shared by eight entries: whichever runs first after a materialising run forms what it needs, and the others must find
    exactly what they would have formed themselves.  Every claimant in turn is the first call; then ``solve``, the
    recurrence variance, ``forecast`` with its variance, ``leave_one_out`` and ``predict_terms`` with its variance run on
    the same plan, and each equals, bit for bit, what a fresh plan returns for that call alone.  22 chunks with a ragged
    last one (a stale start state shows there), widths (2, 3), a dozen unsorted points per problem."""
    case, own, phi, alone = call_order_case(layout)
    plan = call_order_plan(case, layout)
    try:
        FIRST_CALLS[first](plan, own, phi)
        for name, call in FOLLOWERS:
            got = arrays_of(call(plan, own, phi))
            assert len(got) == len(alone[name])
            for k, (a, b) in enumerate(zip(got, alone[name])):
                assert np.array_equal(a, b), (first, name, k, float(np.max(np.abs(a - b))))
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. wide consumers (widths 9..64) in every summarize / prefix bucket of launch_wsweep_scan
# ---------------------------------------------------------------------------------------------------------------------

# N -> (B, family): 512 the shortest series the wide batched solve takes (a problem in the middle not positive definite);
# 2047 / 2048 dot_L and dot on the sequential kernel / the chunked scan (attributed against binary128); 20000 with
# B <= 16: 2048 / B >= 128 chunks per problem, the two-level prefix at widths <= 32 (wsweep_run_len)
WIDE_LENGTHS = {512: (5, "bench"), 2047: (3, "accuracy"), 2048: (3, "accuracy"), 20000: (4, "bench")}


@pytest.mark.parametrize("N", sorted(WIDE_LENGTHS))
@pytest.mark.parametrize("JR,JC", CONSUMER_WIDE_SHAPES)
def test_wide_consumers_in_every_sweep_bucket(JR, JC, N):
    """The wide consumers run the object API's sweeps with a problem axis (``SweepParams::batch``, ``stride_ws``,
    ``stride_W`` ...): ``solve`` / ``predict`` the affine scans of ``launch_wsweep_scan``, ``dot_L`` ``wdotl`` or the
    sequential kernel, ``dot`` the object API's kernels problem by problem.  One shape per summarize / prefix
    instantiation (widths 12 ... 64), at the lengths where the kernels change."""
    B, family = WIDE_LENGTHS[N]
    case = synthetic(B, N, JR, JC, family, seed=1000 + N % 97 + 3 * JR + JC)
    mid = B // 2
    if N == 512:
        (case["a_real"] if JR else case["a_comp"])[mid] *= -40.0      # not positive definite: status 2, neighbours intact
    rng, rhs = make_rhs(B, N, 5 + JC)
    points = prediction_points(case, rng)
    jitter = rng.uniform(0.0, 0.5, B)
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        out = run_consumers(plan, case, rhs, points, jitter)
    finally:
        plan.close()
    refused = check_against_oracle("wide consumers (width %d)" % (JR + 2 * JC), case, rhs, points, jitter, out, WIDE_SOLVE,
                                   truth_bar=WIDE_SOLVE if N == 2048 else None,
                                   dot_L_bar=WIDE_DOT_L_LONG if N == 20000 else DOT)
    assert refused == ([mid] if N == 512 else [])


@pytest.mark.parametrize("JR,JC", CONSUMER_WIDE_SHAPES)
def test_wide_solve_and_predict_refuse_a_series_shorter_than_512(JR, JC):
    """At N = 511 the wide batched solve (and predict, built on it) has no kernel: CLR_UNSUPPORTED, never numbers.
    ``dot_L`` and ``dot`` still apply (the sequential kernels) and match the oracle."""
    B, N = 2, 511
    case = synthetic(B, N, JR, JC, "bench", seed=5 + JC)
    rng = np.random.RandomState(3)
    z = rng.randn(B, N)
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        for call in (lambda: plan.solve(), lambda: plan.solve(z), lambda: plan.predict(case["t"][0, ::7])):
            with pytest.raises(RuntimeError, match="unsupported configuration"):
                call()
        got_L, got_K = plan.dot_L(z), plan.dot(z)
    finally:
        plan.close()
    for p in range(B):
        r = oracle_solver(case, p)
        within("wide consumers at N = 511: dot_L vs oracle dot_L, of the largest entry", of_largest(got_L[p], r.dot_L(z[p])[:, 0]), DOT, p)
        within("wide consumers at N = 511: dot vs oracle dot, of the largest entry",
               of_largest(got_K[p], r.dot(0.0, *coeffs_of(case, p), *NOGEN, case["t"][p], z[p])[:, 0]), DOT, p)


@pytest.mark.parametrize("JR,JC", [(4, 4), (1, 22)])
def test_wide_consumers_on_a_batch_of_1024(JR, JC):
    """B = 1024 problems at N = 512: the batched solve's chunks per problem clamp to 2 (2048 / B), the workspace and
    output strides span the whole batch.  Every problem against the oracle."""
    B, N = 1024, 512
    case = synthetic(B, N, JR, JC, "bench", seed=61 + JC)
    rng = np.random.RandomState(8)
    z = rng.randn(B, N)
    xs = np.sort(rng.uniform(case["t"].min() - 0.05, case["t"].max() + 0.05, 120))
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        ll, ld, q, st = plan.log_likelihood(materialize=True)
        x, Lz, pred, Kz = plan.solve(), plan.dot_L(z), plan.predict(xs), plan.dot(z)
    finally:
        plan.close()
    s0 = ref.batch_log_likelihood(0.0, *coeffs_of(case), case["t"], case["diag"], case["y"])[3]
    assert np.array_equal(st, s0) and (st == 0).all()
    worst = {"solve": 0.0, "dot_L": 0.0, "predict": 0.0, "dot": 0.0}
    for p in range(B):
        r = oracle_solver(case, p)
        worst["solve"] = max(worst["solve"], of_largest(x[p], r.solve(case["y"][p])[:, 0]))
        worst["dot_L"] = max(worst["dot_L"], of_largest(Lz[p], r.dot_L(z[p])[:, 0]))
        worst["predict"] = max(worst["predict"], of_largest(pred[p], r.predict(case["y"][p], xs)))
        worst["dot"] = max(worst["dot"], of_largest(Kz[p], r.dot(0.0, *coeffs_of(case, p), *NOGEN, case["t"][p], z[p])[:, 0]))
    tag = "wide consumers, B = 1024 (width %d): " % (JR + 2 * JC)
    within(tag + "solve(y) vs oracle, of the largest entry", worst["solve"], WIDE_SOLVE)
    within(tag + "dot_L vs oracle, of the largest entry", worst["dot_L"], DOT)
    within(tag + "predict vs oracle, of the largest", worst["predict"], PREDICT)
    within(tag + "dot vs oracle, of the largest entry", worst["dot"], DOT)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the batch axis past 65535 problems
# ---------------------------------------------------------------------------------------------------------------------

BIG_B, DISTINCT = 65537, 64


def tiled(case, B):
    """``case`` of DISTINCT problems repeated over a batch of B: problem p is problem p % DISTINCT."""
    idx = np.arange(B) % DISTINCT
    return {k: v[idx] for k, v in case.items()}


def big_and_twin(JR, JC, N, nchunk, family, seed, ops):
    """Runs ``ops(plan)`` on a plan of 65537 tiled problems and on the plan of the DISTINCT problems themselves."""
    small = synthetic(DISTINCT, N, JR, JC, family, seed=seed)
    big = tiled(small, BIG_B)
    res = []
    for case in (big, small):
        B = case["t"].shape[0]
        plan = batch.BatchedGP(B, N, JR, JC)
        try:
            if nchunk:
                plan.set_chunks(nchunk)
            plan.set_series(case["t"], case["diag"], case["y"])
            plan.set_coefficients(*coeffs_of(case))
            res.append(ops(plan, B))
        finally:
            plan.close()
        del case
    return small, big, res[0], res[1]


def compare_every_problem(tag, big_out, twin_out, bars, bitwise):
    """Every one of the 65537 problems against its twin in the plan of the distinct problems."""
    idx = np.arange(BIG_B) % DISTINCT
    for key, bar in bars.items():
        g, w = big_out[key], twin_out[key][idx]
        assert g.shape[0] == BIG_B and np.isfinite(g).all(), (tag, key)
        axes = tuple(range(1, g.ndim))
        scale = np.max(np.abs(w), axis=axes) if axes else np.abs(w)
        dev = np.max(np.abs(g - w), axis=axes) / scale if axes else np.abs(g - w) / scale
        within(tag + ": %s of all 65537 problems vs the plan of the 64 distinct ones" % key, np.max(dev), bar, int(np.argmax(dev)))
        if key in bitwise:
            assert np.array_equal(g, w), (tag, key, np.flatnonzero(np.any(g != w, axis=axes) if axes else g != w)[:10])


def check_log_likelihoods(tag, big, got):
    """The evaluation's and the materialising run's log-likelihoods of all 65537 problems against the oracle directly,
    and both moved into ``got`` under their own keys for the twin comparison."""
    l0, d0, q0, s0 = ref.batch_log_likelihood(0.0, *coeffs_of(big), big["t"], big["diag"], big["y"],
                                              nthreads=min(32, os.cpu_count() or 1))
    assert (s0 == 0).all()
    for run, key in (("evaluation", "ll0"), ("materialising run", "ll")):
        ll, ld, q, st = got[key]
        assert np.array_equal(st, s0), (tag, run)
        within(tag + ", %s: log det of all 65537 problems vs oracle (relative)" % run, np.max(np.abs(ld - d0) / np.abs(d0)), 1e-10)
        within(tag + ", %s: quadratic form of all 65537 problems vs oracle (relative)" % run, np.max(np.abs(q - q0) / np.abs(q0)), 1e-10)
        within(tag + ", %s: log-likelihood of all 65537 problems vs oracle (relative)" % run, np.max(np.abs(ll - l0) / np.abs(l0)), 1e-10)


def split_results(out):
    for key in ("ll0", "ll"):
        for name, v in zip(("loglike", "logdet", "quad"), out[key][:3]):
            out["%s (%s)" % (name, "evaluation" if key == "ll0" else "materialising run")] = v


LL_BARS = {"%s (%s)" % (n, r): 1e-10 for n in ("loglike", "logdet", "quad") for r in ("evaluation", "materialising run")}


def test_narrow_plan_past_65535_problems():
    """B = 65537 problems of width 3 ((1, 1), N = 256, 4 chunks): every launch that puts the problem on grid.y / grid.z
    -- summarize, replay, the narrow consumers, the gradient's reductions and adjoint walk -- must reach every problem.
    64 distinct problems are tiled over the batch; each of the 65537 is compared with its twin in a plan of the 64 (bit
    for bit where the chunking pins the arithmetic), the 64 with the oracle, all 65537 log-likelihoods with the oracle
    directly.  Needs about 2 GB of device memory."""
    JR, JC, N = 1, 1, 256
    rng = np.random.RandomState(12)
    z_small = rng.randn(DISTINCT, N)
    xs = np.sort(rng.uniform(-0.05, 1.05, 50))

    def ops(plan, B):
        z = z_small[np.arange(B) % DISTINCT]
        out = {}
        out["ll0"] = plan.log_likelihood()
        out["ll"] = plan.log_likelihood(materialize=True)
        out["solve"] = plan.solve()
        out["dot_L"] = plan.dot_L(z)
        out["dot"] = plan.dot(z)
        out["predict"] = plan.predict(xs)
        out["grad value"], out["grad"], gst = plan.grad_log_likelihood()
        assert (gst == 0).all()
        return out

    small, big, got, twin = big_and_twin(JR, JC, N, 4, "bench", 7, ops)
    tag = "B = 65537, narrow plan (width 3)"
    check_log_likelihoods(tag, big, got)
    split_results(got)
    split_results(twin)
    compare_every_problem(tag, got, twin, dict(LL_BARS, solve=NARROW_SOLVE, dot_L=DOT, dot=DOT, predict=PREDICT,
                                               **{"grad value": 1e-10, "grad": 1e-10}),
                          bitwise=[k for k in LL_BARS if "materialising" in k] + ["solve", "dot_L", "dot", "predict"])
    from oracle import grad as ograd
    for p in range(DISTINCT):
        r = oracle_solver(small, p)
        within(tag + ": the 64 distinct problems, solve vs oracle, of the largest entry", of_largest(twin["solve"][p], r.solve(small["y"][p])[:, 0]), NARROW_SOLVE, p)
        within(tag + ": the 64 distinct problems, dot_L vs oracle, of the largest entry", of_largest(twin["dot_L"][p], r.dot_L(z_small[p])[:, 0]), DOT, p)
        within(tag + ": the 64 distinct problems, dot vs oracle, of the largest entry",
               of_largest(twin["dot"][p], r.dot(0.0, *coeffs_of(small, p), *NOGEN, small["t"][p], z_small[p])[:, 0]), DOT, p)
        within(tag + ": the 64 distinct problems, predict vs oracle, of the largest", of_largest(twin["predict"][p], r.predict(small["y"][p], xs)), PREDICT, p)
        if p in (0, DISTINCT - 1):
            v0, g0 = ograd.grad_log_likelihood(0.0, *coeffs_of(small, p), *NOGEN, small["t"][p], small["y"][p], small["diag"][p])
            within(tag + ": the 64 distinct problems, gradient partials vs oracle (of the largest partial)",
                   of_largest(twin["grad"][p], g0), 1e-10, p)


def test_wide_plan_past_65535_problems():
    """B = 65537 problems of width 9 ((9, 0), N = 512): the wide evaluation and materialising run, the batched solve
    (the wide sweeps with the problem on grid.z), ``dot_L`` and ``predict`` must reach every problem.  64 distinct
    problems tiled over the batch; each of the 65537 against its twin in a plan of the 64, the 64 against the oracle, all
    65537 log-likelihoods against the oracle directly.  Needs about 8 GB of device memory (the reference layout's phi,
    u and W of 65537 x 512 x 9 doubles each)."""
    JR, JC, N = 9, 0, 512
    rng = np.random.RandomState(13)
    z_small = rng.randn(DISTINCT, N)
    xs = np.sort(rng.uniform(-0.05, 1.05, 50))

    def ops(plan, B):
        z = z_small[np.arange(B) % DISTINCT]
        out = {}
        out["ll0"] = plan.log_likelihood()
        out["ll"] = plan.log_likelihood(materialize=True)
        out["solve"] = plan.solve()
        out["dot_L"] = plan.dot_L(z)
        out["predict"] = plan.predict(xs)
        return out

    small, big, got, twin = big_and_twin(JR, JC, N, 0, "bench", 8, ops)
    tag = "B = 65537, wide plan (width 9)"
    check_log_likelihoods(tag, big, got)
    split_results(got)
    split_results(twin)
    compare_every_problem(tag, got, twin, dict(LL_BARS, solve=WIDE_SOLVE, dot_L=DOT, predict=PREDICT), bitwise=())
    for p in range(DISTINCT):
        r = oracle_solver(small, p)
        within(tag + ": the 64 distinct problems, solve vs oracle, of the largest entry", of_largest(twin["solve"][p], r.solve(small["y"][p])[:, 0]), WIDE_SOLVE, p)
        within(tag + ": the 64 distinct problems, dot_L vs oracle, of the largest entry", of_largest(twin["dot_L"][p], r.dot_L(z_small[p])[:, 0]), DOT, p)
        within(tag + ": the 64 distinct problems, predict vs oracle, of the largest", of_largest(twin["predict"][p], r.predict(small["y"][p], xs)), PREDICT, p)
