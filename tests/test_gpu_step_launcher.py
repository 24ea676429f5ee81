# -*- coding: utf-8 -*-
"""`-m gpu`: an evaluation launched by ``clr_batch_enqueue`` and one launched inside ``clr_batch_run_timed`` are the
same evaluation -- on every route a plan can take (csrc/api_batch.hip: launch_step).  For each route: a fresh plan's
``log_likelihood()`` against a second fresh plan's ``run_timed(2, ...)`` + ``results()``, with and without the relayout
inside the step, all four arrays bit for bit; then a second coefficient draw on the timed plan against a fresh plan at
that draw (a stale ``*_pending`` flag or a copy that was not rebuilt shows there).  No oracle: equality only.  And the
per-kernel events of ``set_profiling`` / ``profile()``, which the benchmark reads."""
import numpy as np
import pytest

from celerite_amd import batch
from _cases import synthetic, coeffs_of

pytestmark = pytest.mark.gpu
NAMES = ("loglike", "logdet", "quad", "status")


def _second_draw(case, seed=1):
    rng = np.random.RandomState(seed)
    return tuple(c * (1.0 + 0.02 * rng.rand(*c.shape)) for c in coeffs_of(case))


def _plan(case, setup=None, coeffs=None, general=None, mean=None, jitter=0.0):
    """A fresh plan: settings, series, general terms, a mean set AFTER the series, coefficients."""
    B, N = case["y"].shape
    plan = batch.BatchedGP(B, N, case["a_real"].shape[1], case["a_comp"].shape[1])
    try:
        if setup:
            setup(plan)
        plan.set_series(case["t"], case["diag"], case["y"])
        if general:
            plan.set_general(*general)
        if mean is not None:
            plan.set_mean(mean)
        plan.set_coefficients(*(coeffs_of(case) if coeffs is None else coeffs), jitter=jitter)
    except Exception:
        plan.close()
        raise
    return plan


def _same(want, got, ctx):
    for name, a, b in zip(NAMES, want, got):
        assert np.array_equal(a, b), (ctx, name, a, b)


def _same_factor(a, b, B, ctx):
    for p in (0, B - 1):
        for name, x, y in zip(("phi", "u", "W", "D"), a.factor(p), b.factor(p)):
            assert np.array_equal(x, y), (ctx, p, name)


def _check_route(case, setup=None, route=None, info=None, materialize=False, **kw):
    """``route(plan)``: asserts on a plan before it evaluates that it takes the route meant; ``info(plan)``: what the
    plan reports about its last fetched evaluation (warm statistics, re-planned problems), equal on both plans."""
    B = case["y"].shape[0]
    a = _plan(case, setup, **kw)
    b = _plan(case, setup, **kw)
    try:
        if route:
            route(a)
            route(b)
        want = a.log_likelihood(materialize)
        want_info = info(a) if info else None
        for relayout in (False, True):
            b.run_timed(2, materialize=materialize, relayout_each_step=relayout)
            _same(want, b.results(), ("run_timed", relayout))
            if info:
                assert info(b) == want_info, (relayout, info(b), want_info)
            if materialize:
                _same_factor(a, b, B, ("run_timed", relayout))
        # a second draw on the plan the timed steps ran on, against a fresh plan at that draw
        c2 = _second_draw(case)
        jitter = kw.get("jitter", 0.0)
        b.set_coefficients(*c2, jitter=jitter)
        got2 = b.log_likelihood(materialize)
        f = _plan(case, setup, **dict(kw, coeffs=c2))
        try:
            _same(f.log_likelihood(materialize), got2, "second draw")
            if info:
                assert info(b) == info(f), (info(b), info(f))
            if materialize:
                _same_factor(f, b, B, "second draw")
        finally:
            f.close()
    finally:
        a.close()
        b.close()
    return want


def _narrow_scan(nchunk, summarize=None, kernel="single wave"):
    def setup(plan):
        plan.set_chunks(nchunk)
        plan.set_small_mode(0)
        plan.set_warm_start(0)
        if summarize is not None:
            plan.set_summarize_mode(summarize)

    def route(plan):
        # (a chunk count is rounded to chunks of whole tile rows: 64 asked for may be 63)
        assert (plan.chunks[0] > 1) == (nchunk > 1) and plan.summarize_kernel() == kernel, (plan.chunks, plan.summarize_kernel())
        assert not plan.small_mode_active() and plan.warm_start()["active"] == 0

    return dict(setup=setup, route=route)


@pytest.mark.parametrize("nchunk", [24, 1])
def test_narrow_scan_single_wave_summarize(nchunk):
    """Width 4 through summarize -> prefix -> correct -> replay -> sequential -> finalize, chunked and as one chunk."""
    _check_route(synthetic(6, 5000, 2, 1, "bench", seed=1), **_narrow_scan(nchunk))


@pytest.mark.parametrize("mode,kernel", [(1, "role split"), (2, "role split, lazy decay")])
def test_role_split_summarize(mode, kernel):
    """Width 8 on the role-split summarize, which reads the chunk-interleaved copy (test_role_split_summarize_kernels'
    dense shape: the relayout inside or in front of the timed steps)."""
    JR, JC, N = 2, 3, 6000
    case = synthetic(5, N, JR, JC, "bench", seed=JR + 7 * JC + N)
    case["t"] = case["t"] * 0.2
    _check_route(case, **_narrow_scan(64, summarize=mode, kernel=kernel))


def _slow_decay_batch():
    """test_warm_start_mixed_batch_and_indefinite_neighbours' batch without the indefinite problem: two problems whose
    slowest term does not forget over any warm-up."""
    case = synthetic(10, 16000, 2, 2, "accuracy", seed=5)
    case["c_real"][3, 0] = 1e-4
    case["c_real"][6, 1] = 3e-4
    return case


@pytest.mark.parametrize("which", ["some fall back", "all fall back"])
def test_warm_path_and_its_fallback_scan(which):
    """The warm-started recurrence, the problems it leaves pending settled by the scan behind it when the results are
    fetched: a forced warm-up of 128 steps that two problems of the batch do not converge over, and
    test_warm_start_boundary_check_sends_unconverged_problems_to_the_scan's two-step warm-up that nothing converges over."""
    if which == "some fall back":
        case, K = _slow_decay_batch(), 128
    else:
        case, K = synthetic(9, 12000, 2, 3, "accuracy", seed=77), 2
    B = case["y"].shape[0]

    def route(plan):
        assert plan.warm_start()["active"] == 1

    seen = []

    def info(plan):
        w = plan.warm_start()
        seen.append(w["fallbacks"])
        return w

    _check_route(case, setup=lambda plan: plan.set_warm_start(1, K), route=route, info=info)
    assert (0 < seen[0] < B) if which == "some fall back" else (seen[0] == B), seen


def test_one_launch_path():
    """test_short_narrow_problems_in_one_launch's shape: short narrow problems in one launch, a near-singular one left
    pending and settled by the scan pipeline."""
    JR, JC, N = 2, 1, 10000
    case = synthetic(5, N, JR, JC, "bench", seed=3 * JR + 5 * JC + N)
    case["diag"] = np.array(case["diag"], copy=True)
    case["diag"][3] = 1e-14

    def setup(plan):
        plan.set_small_mode(1)
        plan.set_warm_start(0)

    def route(plan):
        assert plan.small_mode_active()

    _check_route(case, setup=setup, route=route)


@pytest.mark.parametrize("JR,JC,N,nchunk", [(2, 7, 3000, 5), (10, 11, 3000, 5), (8, 20, 6000, 5), (0, 24, 6000, 1)])
def test_wide_plans(JR, JC, N, nchunk):
    """Widths 9..32 and 33..64 (test_wide_scan_over_chunks, ..._at_widths_33_to_64): the wide flow, chunked and as one sweep."""
    def route(plan):
        assert plan.chunks[0] == nchunk, plan.chunks

    _check_route(synthetic(3, N, JR, JC, "bench", seed=JR + 3 * JC), setup=lambda plan: plan.set_chunks(nchunk), route=route)


@pytest.mark.parametrize("JR,JC,JG,N,sequential", [(0, 4, 2, 1500, False), (0, 4, 2, 1500, True), (2, 1, 3, 700, False)])
def test_general_terms(JR, JC, JG, N, sequential):
    """General terms on the wide kernels (chunked at N = 1500, one chunk at 700) and on the any-width sequential kernel
    (test_general_terms_in_the_batch's shapes)."""
    B = 5
    rng = np.random.RandomState(JR + 10 * JC + JG)
    case = synthetic(B, N, JR, JC, "accuracy", seed=3 + JG)
    U = np.stack([np.vander((t - t.mean()) / (t.max() - t.min()), JG).T for t in case["t"]])
    V = U * rng.rand(B, JG)[:, :, None]
    A = np.sum(U * V, axis=1) + 1e-8
    _check_route(case, setup=(lambda plan: plan.set_general_route(1)) if sequential else None, general=(A, U, V), jitter=0.01)


def test_widths_65_to_128():
    _check_route(synthetic(3, 700, 1, 40, "bench", seed=81))


@pytest.mark.parametrize("layout", ["reference", "lean"])
def test_materialising_narrow_plan(layout):
    """A materialising run (replay modes 2 and 3, the chunk heads): results and the factor of the first and last problem."""
    def setup(plan):
        plan.set_chunks(24)
        plan.set_factor_layout(layout)

    _check_route(synthetic(5, 3000, 2, 3, "bench", seed=90 + 2 + 9), setup=setup, materialize=True)


def test_materialising_wide_plan():
    _check_route(synthetic(3, 3000, 1, 5, "bench", seed=9), setup=lambda plan: plan.set_chunks(6), materialize=True)


def _gamma_bound(case, setup, k):
    """The bound on gamma_max that sends exactly the k problems with the largest conditioning record to route 1
    (test_gpu_batch.py: _send_to_route1), read off a plan of its own."""
    plan = _plan(case, setup)
    try:
        plan.log_likelihood()
        gamma = np.sort(plan.conditioning()[0])[::-1]
    finally:
        plan.close()
    assert gamma[k - 1] > gamma[k]
    return 0.5 * (gamma[k - 1] + gamma[k])


def _check_deferred(case, chunks, k):
    def base(plan):
        if chunks:
            plan.set_chunks(chunks)

    bound = _gamma_bound(case, base, k)

    def setup(plan):
        base(plan)
        plan.set_certificate(max_gamma=bound)

    seen = []

    def info(plan):
        r = plan.rescue()
        seen.append(r["last"])
        # (the side plan's chunking while one is in use: a plan keeps its last side plan when nothing is pending)
        return r["last"], r["chunks"] if r["last"] else None, int((plan.exact_levels() == 1).sum())

    _check_route(case, setup=setup, info=info)
    # first the fresh plan's evaluation (k problems re-planned as a side plan), then the timed plan's: without and --
    # once an evaluation has re-planned -- with the side plan settled inside every step
    assert seen[0] == k and seen[1] == k and seen[2] == k, seen


def test_deferred_level1_problems_on_a_narrow_plan():
    """test_route1_replanning_on_a_narrow_plan_and_its_fallbacks' shape: level-1 problems left pending by the evaluation
    and re-planned with short chunks when the results are fetched -- or, in a timed step of a plan that has re-planned
    before, inside the step."""
    _check_deferred(synthetic(24, 40000, 2, 3, "bench", seed=515), 32, 2)


def test_deferred_level1_problems_on_a_wide_plan():
    """test_route1_problems_are_replanned_with_short_chunks' B = 128 shape (width 32, N = 1e5)."""
    from bench import make_inputs
    B, N, JC = 128, 100000, 16
    coeffs, t, diag, y = make_inputs(B, N, 0, JC, seed=B, d_spread=True)
    case = dict(zip(("a_real", "c_real", "a_comp", "b_comp", "c_comp", "d_comp"), coeffs), t=t, diag=diag, y=y)
    _check_deferred(case, 0, 4)


@pytest.mark.parametrize("JR,JC,setup_kw", [(6, 1, dict(nchunk=64, kernel="role split, lazy decay")), (2, 1, dict(nchunk=24))])
def test_mean_set_after_the_series(JR, JC, setup_kw):
    """A per-problem mean set after the series: the residual replaces y, and of the chunk-interleaved copy only y's part
    is rebuilt (relayout_y_pending) -- by ``enqueue`` and by the timed steps alike, also when the mean changes between
    two evaluations of the same plan."""
    B, N = 5, 6000
    case = synthetic(B, N, JR, JC, "bench", seed=17)
    case["t"] = case["t"] * 0.2
    rng = np.random.RandomState(3)
    mu = [rng.randn(B) for _ in range(3)]
    route = _narrow_scan(**setup_kw)
    _check_route(case, mean=mu[0], **route)
    b = _plan(case, route["setup"], mean=mu[0])
    try:
        b.log_likelihood()
        for m, relayout in ((mu[1], False), (mu[2], True)):   # only the mean changes: the copy of y alone is stale
            b.set_mean(m)
            b.run_timed(1, relayout_each_step=relayout)
            f = _plan(case, route["setup"], mean=m)
            try:
                _same(f.log_likelihood(), b.results(), ("new mean, timed", relayout))
                b.set_mean(mu[0])
                f.set_mean(mu[0])
                _same(f.log_likelihood(), b.log_likelihood(), ("mean back, enqueue", relayout))
            finally:
                f.close()
    finally:
        b.close()


def _profiled(plan, on, steps=3):
    plan.set_profiling(on)
    for _ in range(steps):
        plan.enqueue()
    plan.synchronize()
    return plan.profile()


@pytest.mark.parametrize("which", ["narrow scan", "one launch", "wide"])
def test_profile_of_enqueued_evaluations(which):
    """``set_profiling`` / ``profile()`` (clr_batch_get_profile): one record per enqueued evaluation, every slot a
    non-negative time, a positive sum; mode 2 on a narrow plan brackets the summarize kernel only."""
    if which == "wide":
        plan = _plan(synthetic(3, 3000, 2, 7, "bench", seed=23), lambda p: p.set_chunks(5))
    elif which == "one launch":
        plan = _plan(synthetic(5, 10000, 2, 1, "bench", seed=1), lambda p: (p.set_small_mode(1), p.set_warm_start(0)))
    else:
        plan = _plan(synthetic(6, 5000, 2, 1, "bench", seed=1), _narrow_scan(24)["setup"])
    try:
        ms, steps = _profiled(plan, True)
        assert steps == 3 and set(ms) == set(plan.KERNEL_NAMES), (steps, ms)
        assert all(v >= 0.0 for v in ms.values()) and sum(ms.values()) > 0.0, ms
        if which != "wide":
            ms, steps = _profiled(plan, 2)
            assert steps == 3 and ms["summarize"] > 0.0, (steps, ms)
            assert all(v == 0.0 for k, v in ms.items() if k != "summarize"), ms
    finally:
        plan.close()
