# -*- coding: utf-8 -*-
"""`-m gpu`: a plan that has evaluated, had ONE input or setting changed and evaluates again gives what a plan built
directly at the new state gives -- ``loglike, logdet, quad, status`` bit for bit, on materialising runs the factor of the
first and the last problem too.  Every route keeps something derived from the series (a chunk-interleaved copy, the
warm path's spans, a factor) and every change leaves some of it stale (csrc/api_internal.h: series_replaced,
residual_replaced, chunking_replaced, scan_reader_changed): a copy that was not rebuilt, or was taken for rebuilt, shows
here.  No oracle: equality only.

Reshaped so that a reused plan carries no history a fresh one lacks:
  * the warm path runs with a forced warm-up (``set_warm_start(1, K)``): the automatic mode adapts the warm-up lengths
    to the fallbacks of earlier evaluations (warm_boost / warm_clean), which a fresh plan has not seen;
  * a series with a shared ``y`` replaces the per-problem one a plan is created with before anything is evaluated
    (test_gpu_step_launcher's ``_plan`` reads the batch's shape off a per-problem ``y``), on both plans alike."""
import numpy as np
import pytest

from _cases import synthetic, coeffs_of
from test_gpu_step_launcher import _narrow_scan, _plan, _same, _same_factor

pytestmark = pytest.mark.gpu


def _at(setup, case, shared_y=None, mean=None, extra=None, coeffs=None):
    """A plan at a state, nothing evaluated yet: the route's settings, then ``extra``'s; the series; the mean."""
    def settings(plan):
        setup(plan)
        if extra:
            extra(plan)

    plan = _plan(case, settings, coeffs=coeffs)
    try:
        if shared_y is not None:
            plan.set_series(case["t"], case["diag"], shared_y)
        if mean is not None:
            plan.set_mean(mean)
    except Exception:
        plan.close()
        raise
    return plan


def _width4(N=5000):
    return synthetic(5, N, 2, 1, "bench", seed=1)


def _dense(JR, JC, seed):
    """test_role_split_summarize's series: dense enough for the lazy-decay kernels at these coefficients."""
    case = synthetic(5, 6000, JR, JC, "bench", seed=seed)
    case["t"] = case["t"] * 0.2
    return case


def _interleaved(nchunk):
    r = _narrow_scan(nchunk)
    return dict(r, setup=lambda plan: (r["setup"](plan), plan.set_layout("interleaved")))


def _warm():
    """Forced warm-up of 128 steps; one problem's slowest term does not forget over it and falls back to the scan."""
    case = synthetic(5, 6000, 2, 2, "accuracy", seed=5)
    case["c_real"][3, 0] = 1e-4

    def route(plan):
        assert plan.warm_start()["active"] == 1

    return dict(case=case, setup=lambda plan: plan.set_warm_start(1, 128), route=route, chunks=12)


def _one_launch(layout=None):
    """test_one_launch_path's batch, shorter: a near-singular problem is left pending and settled by the scan."""
    case = _width4(4000)
    case["diag"] = np.array(case["diag"], copy=True)
    case["diag"][3] = 1e-14

    def setup(plan):
        plan.set_small_mode(1)
        plan.set_warm_start(0)
        if layout:
            plan.set_chunks(24)
            plan.set_layout(layout)

    def route(plan):
        assert plan.small_mode_active()

    return dict(case=case, setup=setup, route=route, chunks=8)


def _wide():
    def route(plan):
        assert plan.chunks[0] == 5, plan.chunks

    return dict(case=synthetic(3, 3000, 2, 7, "bench", seed=23), setup=lambda plan: plan.set_chunks(5), route=route, chunks=3)


# route -> the batch, the settings that select it, a check that a plan takes it, and what the changes of a setting
# change it to (chunks, layout, summarize: another chunk count, layout and summarize mode than the route's own)
ROUTES = {
    "narrow, staged": lambda: dict(case=_width4(), chunks=16, layout="interleaved", **_narrow_scan(24)),
    "narrow, interleaved": lambda: dict(case=_width4(), chunks=16, layout="staged", **_interleaved(24)),
    "role split": lambda: dict(case=_dense(2, 3, 8023), chunks=48, summarize=2, **_narrow_scan(64, summarize=1, kernel="role split")),
    "warm": _warm,
    "one launch": _one_launch,
    "wide": _wide,
}
MATERIALISING = ("narrow, interleaved", "role split", "wide")  # (the warm and the one-launch path never materialise)


def _change(name, r, rng):
    """``(state 1, the change on a plan at state 1, state 2)``; a state is ``_at``'s keyword arguments."""
    case = r["case"]
    B, N = case["y"].shape
    if name == "new series":
        new = dict(case, t=case["t"] * 0.97, diag=case["diag"] * 1.1, y=case["y"] + 0.1 * rng.randn(B, N))
        return dict(case=case), lambda p: p.set_series(new["t"], new["diag"], new["y"]), dict(case=new)
    if name == "shared y to per-problem y":
        return (dict(case=case, shared_y=case["y"][0]), lambda p: p.set_series(case["t"], case["diag"], case["y"]),
                dict(case=case))
    if name == "new scalar mean":
        return dict(case=case, mean=0.3), lambda p: p.set_mean(-0.7), dict(case=case, mean=-0.7)
    if name == "per-problem mean on a shared y":   # (the residual's stride changes: 0 -> N)
        mu = rng.randn(B)
        return (dict(case=case, shared_y=case["y"][0]), lambda p: p.set_mean(mu),
                dict(case=case, shared_y=case["y"][0], mean=mu))
    if name == "mean removed":
        return dict(case=case, mean=rng.randn(B)), lambda p: p.set_mean(None), dict(case=case)
    if name == "set_chunks":
        n = r["chunks"]
        return dict(case=case), lambda p: p.set_chunks(n), dict(case=case, extra=lambda p: p.set_chunks(n))
    if name == "set_layout":
        lay = r.get("layout", "interleaved")
        return dict(case=case), lambda p: p.set_layout(lay), dict(case=case, extra=lambda p: p.set_layout(lay))
    if name == "set_summarize_mode":
        m = r.get("summarize", 0)
        return dict(case=case), lambda p: p.set_summarize_mode(m), dict(case=case, extra=lambda p: p.set_summarize_mode(m))
    raise ValueError(name)


CHANGES = ("new series", "shared y to per-problem y", "new scalar mean", "per-problem mean on a shared y", "mean removed",
           "set_chunks", "set_layout", "set_summarize_mode")


def _check_reuse(setup, route, state1, change, state2, materialize=False, kernels=None):
    """``kernels``: the summarize kernel the reused plan reports at state 1 and at state 2."""
    a = _at(setup, **state1)
    b = None
    try:
        if route:
            route(a)
        if kernels:
            assert a.summarize_kernel() == kernels[0], a.summarize_kernel()
        a.log_likelihood(materialize)
        change(a)
        if kernels:
            assert a.summarize_kernel() == kernels[1], a.summarize_kernel()
        got = a.log_likelihood(materialize)
        b = _at(setup, **state2)
        _same(b.log_likelihood(materialize), got, "reused against fresh")
        if materialize:
            _same_factor(b, a, a.B, "reused against fresh")
    finally:
        a.close()
        if b is not None:
            b.close()


@pytest.mark.parametrize("change", CHANGES)
@pytest.mark.parametrize("route", list(ROUTES) + [r + ", materialising" for r in MATERIALISING])
def test_reused_plan_equals_fresh_plan(route, change):
    name, _, mat = route.partition(", materialising")
    r = ROUTES[name]()
    state1, apply, state2 = _change(change, r, np.random.RandomState(11))
    _check_reuse(r["setup"], r["route"], state1, apply, state2, materialize=bool(mat))


@pytest.mark.parametrize("first", ["dense", "not dense"])
def test_coefficient_draw_switches_the_summarize_kernel(first):
    """Width 8 with one complex term, summarize mode automatic: the role split runs only where the draw's decay rates
    make the series dense (lazy_eligible), so a new draw switches the kernel -- and with it whether the scan reads its
    chunk-interleaved copy at all -- with the series unchanged.  Both directions."""
    case = _dense(6, 1, 17)
    fast = dict(case, c_comp=case["c_comp"] * 4.0)   # c_max dx_max: 3.4e-3 -> 1.4e-2, across the bound 2^-7
    draws = {"dense": (coeffs_of(case), "role split, lazy decay"), "not dense": (coeffs_of(fast), "single wave")}
    (c1, k1), (c2, k2) = [draws[d] for d in (("dense", "not dense") if first == "dense" else ("not dense", "dense"))]
    r = _narrow_scan(64)
    _check_reuse(r["setup"], None, dict(case=case, coeffs=c1), lambda p: p.set_coefficients(*c2),
                 dict(case=case, coeffs=c2), kernels=(k1, k2))


def test_scan_after_timed_steps_on_the_one_launch_path():
    """Timed steps with the relayout inside them, on the one-launch path of a plan whose layout is interleaved, rebuild
    the one-launch path's copy of the series and not the scan's; a forced-exact evaluation of the same plan afterwards
    reads the scan's copy, which must be built for it then."""
    r = _one_launch("interleaved")
    exact = lambda p: (p.set_small_mode(0), p.set_exact(True))
    a = _at(r["setup"], r["case"])
    b = None
    try:
        r["route"](a)
        a.run_timed(2, relayout_each_step=True)
        exact(a)
        got = a.log_likelihood()
        b = _at(r["setup"], r["case"], extra=exact)
        _same(b.log_likelihood(), got, "forced-exact scan after timed one-launch steps")
    finally:
        a.close()
        if b is not None:
            b.close()
