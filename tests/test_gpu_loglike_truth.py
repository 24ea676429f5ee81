# -*- coding: utf-8 -*-
"""Every log-likelihood route of the narrow plan (widths 1..8) against the binary128 recurrence
(oracle.ref.quad_factor_solve), log det and quadratic form each, with the double oracle measured beside it on the same
problem: the yardstick is the double oracle's own distance from the truth (tests/_loglike_truth.py), never the
device's, and no absolute tolerance appears apart from the sqrt(N) 2^-53 floor and the suite's REL = 1e-10 as a cap.

Each test names a route and asserts through the plan's own introspection (summarize_kernel, split_variant,
small_mode_active, warm_start, exact_levels, rescue, selection_bounds, prefix_plan, lengths) that it ran.  The
reference side of every case -- judged counts, finite truths, the yardsticks -- is held by
tests/test_loglike_truth_cpu.py without a device.

Bars: 30 x Y on every route and quantity, except the quadratic form of the problems the scan pipeline's summarize kernels
and the one-launch kernel settle from scanned chunk start states (levels 0 and 1) outside the adversarial family: 120 x Y
(QUAD_FACTOR_CHUNKED in tests/_loglike_truth.py, with the attribution -- the composition of the chunk elements on series
that do not forget -- and the measurement, 74 x Y, beside it), on the dense families that do not
forget alone (the squeezed synthetic bench family, F0, F1, F5: quad_factor_of).

Measured on an MI355X (per route and family the case with the worst e_dev / bar; the end-of-session table lists every
line with the level the problems took):
  route                                                                 family      quantity          e_dev    e_ref      bar ratio
  exact replay                                                          G           log det         1.6e-13  1.6e-13  4.9e-12  0.03
  exact replay                                                          G           quadratic form  3.6e-12  3.6e-12  1.0e-10  0.04
  exact replay                                                          adversarial log det         2.3e-14  1.9e-14  5.8e-13  0.04
  exact replay                                                          adversarial quadratic form  3.9e-14  1.0e-14  3.0e-13  0.13
  exact replay                                                          synthetic   log det         7.0e-15  3.4e-15  2.1e-13  0.03
  exact replay                                                          synthetic   quadratic form  6.4e-14  6.5e-16  1.8e-13  0.35
  materialising run, lean factor                                        synthetic   log det         7.0e-15  3.4e-15  2.1e-13  0.03
  materialising run, lean factor                                        synthetic   quadratic form  2.3e-14  3.5e-15  2.1e-13  0.11
  materialising run, reference factor                                   synthetic   log det         7.0e-15  3.4e-15  2.1e-13  0.03
  materialising run, reference factor                                   synthetic   quadratic form  2.3e-14  3.5e-15  2.1e-13  0.11
  one launch                                                            F           log det         1.6e-13  3.8e-15  2.1e-13  0.77
  one launch                                                            F           quadratic form  3.6e-13  4.4e-16  8.5e-13  0.42
  one launch                                                            adversarial log det         1.2e-13  1.6e-14  4.9e-13  0.24
  one launch                                                            adversarial quadratic form  8.2e-14  4.6e-15  1.5e-13  0.55
  one launch                                                            synthetic   log det         9.7e-14  5.4e-15  1.8e-13  0.54
  one launch                                                            synthetic   quadratic form  1.2e-12  2.1e-14  2.5e-12  0.47
  route 1, inline replay                                                route 1     log det         8.6e-15  1.0e-14  3.4e-13  0.03
  route 1, inline replay                                                route 1     quadratic form  1.4e-14  4.3e-15  2.6e-13  0.06
  route 1, side plan                                                    route 1     log det         1.2e-14  7.2e-15  3.4e-13  0.03
  route 1, side plan                                                    route 1     quadratic form  7.5e-14  3.6e-16  2.6e-13  0.29
  scan behind the warm start                                            warm        log det         5.7e-16  2.9e-15  3.7e-13  0.00
  scan behind the warm start                                            warm        quadratic form  7.3e-15  9.9e-15  3.7e-13  0.02
  scan pipeline (role split)                                            F           log det         3.8e-14  7.5e-15  2.3e-13  0.17
  scan pipeline (role split)                                            F           quadratic form  3.3e-13  4.8e-15  8.5e-13  0.38
  scan pipeline (role split)                                            G           log det         1.6e-13  1.6e-13  4.9e-12  0.03
  scan pipeline (role split)                                            G           quadratic form  3.6e-12  3.6e-12  1.0e-10  0.04
  scan pipeline (role split)                                            adversarial log det         1.4e-14  8.3e-15  2.5e-13  0.06
  scan pipeline (role split)                                            adversarial quadratic form  6.1e-14  4.5e-15  3.6e-13  0.17
  scan pipeline (role split)                                            synthetic   log det         3.9e-14  2.2e-14  6.8e-13  0.06
  scan pipeline (role split)                                            synthetic   quadratic form  4.3e-13  7.9e-16  8.1e-13  0.53
  scan pipeline (role split), c dx at 1.05 of the limit                 lazy edge   log det         1.0e-14  9.2e-15  2.8e-13  0.04
  scan pipeline (role split), c dx at 1.05 of the limit                 lazy edge   quadratic form  8.7e-15  8.3e-16  2.1e-13  0.04
  scan pipeline (role split), d dx at 1.05 of the limit                 lazy edge   log det         9.7e-15  9.8e-15  2.9e-13  0.03
  scan pipeline (role split), d dx at 1.05 of the limit                 lazy edge   quadratic form  4.7e-14  3.0e-15  2.1e-13  0.22
  scan pipeline (role split, lazy decay)                                F           log det         2.4e-14  3.8e-15  2.1e-13  0.11
  scan pipeline (role split, lazy decay)                                F           quadratic form  2.1e-12  5.2e-14  6.3e-12  0.33
  scan pipeline (role split, lazy decay)                                route 1     log det         8.8e-15  1.1e-14  3.4e-13  0.03
  scan pipeline (role split, lazy decay)                                route 1     quadratic form  1.4e-14  4.3e-15  2.6e-13  0.06
  scan pipeline (role split, lazy decay), c dx at 0.95 of the limit     lazy edge   log det         1.5e-14  7.7e-15  2.5e-13  0.06
  scan pipeline (role split, lazy decay), c dx at 0.95 of the limit     lazy edge   quadratic form  1.3e-14  1.1e-15  2.1e-13  0.06
  scan pipeline (role split, lazy decay), d dx at 0.95 of the limit     lazy edge   log det         8.5e-15  3.9e-15  2.1e-13  0.04
  scan pipeline (role split, lazy decay), d dx at 0.95 of the limit     lazy edge   quadratic form  3.4e-14  6.7e-15  2.1e-13  0.16
  scan pipeline (role split, lazy decay), every c dx at the lazy limit  lazy edge   log det         6.8e-15  6.6e-15  2.3e-13  0.03
  scan pipeline (role split, lazy decay), every c dx at the lazy limit  lazy edge   quadratic form  3.3e-15  2.6e-15  2.1e-13  0.01
  scan pipeline (role split, lazy decay), every d dx at the lazy limit  lazy edge   log det         9.0e-15  3.6e-16  8.8e-14  0.10
  scan pipeline (role split, lazy decay), every d dx at the lazy limit  lazy edge   quadratic form  2.3e-15  0.0e+00  8.8e-14  0.03
  scan pipeline (role split, lazy decay, automatic)                     synthetic   log det         1.3e-14  8.0e-15  2.6e-13  0.05
  scan pipeline (role split, lazy decay, automatic)                     synthetic   quadratic form  4.0e-13  5.0e-15  1.0e-12  0.39
  scan pipeline (role split, lazy decay, b_comp = 0)                    synthetic   log det         2.9e-14  5.4e-15  2.1e-13  0.14
  scan pipeline (role split, lazy decay, b_comp = 0)                    synthetic   quadratic form  3.5e-13  6.5e-15  7.7e-13  0.45
  scan pipeline (role split, lazy decay, general)                       synthetic   log det         2.5e-14  5.8e-15  1.8e-13  0.14
  scan pipeline (role split, lazy decay, general)                       synthetic   quadratic form  4.8e-13  4.5e-15  8.1e-13  0.59
  scan pipeline (single wave)                                           F           log det         3.6e-14  3.0e-15  2.1e-13  0.17
  scan pipeline (single wave)                                           F           quadratic form  1.7e-13  1.8e-14  5.5e-13  0.32
  scan pipeline (single wave)                                           G           log det         1.6e-13  1.6e-13  4.9e-12  0.03
  scan pipeline (single wave)                                           G           quadratic form  3.6e-12  3.6e-12  1.0e-10  0.04
  scan pipeline (single wave)                                           adversarial log det         1.4e-13  4.9e-15  1.5e-13  0.96
  scan pipeline (single wave)                                           adversarial quadratic form  2.5e-13  3.3e-15  6.5e-13  0.39
  scan pipeline (single wave)                                           synthetic   log det         2.0e-14  5.4e-15  1.8e-13  0.11
  scan pipeline (single wave)                                           synthetic   quadratic form  1.0e-12  1.4e-14  1.7e-12  0.61
  scan pipeline (single wave), exp gaps                                 exp         log det         8.8e-15  5.4e-15  2.6e-13  0.03
  scan pipeline (single wave), exp gaps                                 exp         quadratic form  8.3e-15  3.1e-15  2.1e-13  0.04
  scan pipeline (single wave), exp small                                exp         log det         5.7e-15  5.0e-15  2.1e-13  0.03
  scan pipeline (single wave), exp small                                exp         quadratic form  6.5e-16  2.1e-15  2.1e-13  0.00
  scan pipeline (single wave), exp tiny                                 exp         log det         9.5e-15  8.3e-15  3.0e-13  0.03
  scan pipeline (single wave), exp tiny                                 exp         quadratic form  6.6e-15  1.7e-15  2.1e-13  0.03
  scan pipeline (single wave), per-problem lengths                      ragged      log det         9.2e-15  8.3e-15  2.7e-13  0.03
  scan pipeline (single wave), per-problem lengths                      ragged      quadratic form  4.4e-14  3.3e-16  7.7e-14  0.57
  scan pipeline (single wave), prefix multilevel                        synthetic   log det         6.4e-15  4.0e-15  2.6e-13  0.03
  scan pipeline (single wave), prefix multilevel                        synthetic   quadratic form  1.3e-13  2.0e-15  7.3e-13  0.18
  scan pipeline (single wave), prefix single                            synthetic   log det         8.5e-15  9.2e-15  2.8e-13  0.03
  scan pipeline (single wave), prefix single                            synthetic   quadratic form  7.8e-14  2.6e-15  7.3e-13  0.11
  scan pipeline (single wave), prefix walk                              synthetic   log det         9.8e-15  9.2e-15  2.8e-13  0.04
  scan pipeline (single wave), prefix walk                              synthetic   quadratic form  5.5e-14  2.6e-15  7.3e-13  0.07
  scan pipeline, inline replay                                          adversarial log det         2.1e-14  1.8e-14  5.3e-13  0.04
  scan pipeline, inline replay                                          adversarial quadratic form  1.1e-14  2.8e-15  1.5e-13  0.07
  scan pipeline, side plan                                              adversarial log det         2.1e-14  1.8e-14  5.3e-13  0.04
  scan pipeline, side plan                                              adversarial quadratic form  1.1e-14  2.8e-15  1.5e-13  0.07
  scan pipeline, side plan asked for, no route-1 problem                adversarial log det         2.5e-14  2.2e-14  6.7e-13  0.04
  scan pipeline, side plan asked for, no route-1 problem                adversarial quadratic form  1.1e-13  7.4e-14  2.2e-12  0.05
  warm start                                                            warm        log det         5.7e-16  2.9e-15  3.7e-13  0.00
  warm start                                                            warm        quadratic form  7.3e-15  9.9e-15  3.7e-13  0.02
  library trig at t ~ 3e8 (log-likelihood)                              accuracy    loglike         1.1e-16  6.7e-16  2.1e-13  0.00
"""
import contextlib

import numpy as np
import pytest

from celerite_amd import batch
from _cases import ALL_WIDTH_SHAPES, GRAD_FAMILIES, coeffs_of, within
from _loglike_truth import (EVERY_STEP_D_CHUNKS, EXP_SMALL_LIMIT, EXP_TINY_LIMIT, F_FAMILIES, F_SHAPES, F_SMALL_SHAPES, FACTOR, LARGE_T_JITTER,
                            LAZY_C_LIMIT, LAZY_D_LIMIT, REL, SIZES, SIZE_FAMILIES, SMALL_SHAPES,
                            SPLIT_SHAPES, STRUCT_N, case_of, host_bounds, judge, large_t_case, large_t_reference,
                            quad_factor_of, ragged_lengths, reference)

pytestmark = pytest.mark.gpu

KERNELS = {0: "single wave", 1: "role split", 2: "role split, lazy decay"}
STRUCT_CHUNKS = 37
ADV_CHUNKS = 50


@contextlib.contextmanager
def _plan(key, nchunk=0, small=0, warm=(0, 0), layout=None, prefix=None, lengths=None):
    """A plan on case ``key`` with the fast paths in front of the scan pipeline switched as asked (both off unless the
    route is about them)."""
    case = case_of(key)
    B, N = case["t"].shape
    plan = batch.BatchedGP(B, N, case["a_real"].shape[1], case["a_comp"].shape[1])
    try:
        if nchunk:
            plan.set_chunks(nchunk)
        if layout is not None:
            plan.set_layout(layout)
        if prefix is not None:
            plan.set_prefix_mode(prefix)
        plan.set_small_mode(small)
        plan.set_warm_start(*warm)
        plan.set_series(case["t"], case["diag"], case["y"], lengths=lengths)
        plan.set_coefficients(*coeffs_of(case))
        yield plan
    finally:
        plan.close()


def _scan_runs(plan):
    """Neither fast path is in front of the scan pipeline."""
    return plan.warm_start()["active"] == 0 and not plan.small_mode_active()


def _expect_lazy(key):
    """csrc/api_internal.h, lazy_eligible, from the inputs."""
    case = case_of(key)
    cmax, dmax, dxmax = host_bounds(case)
    return cmax * dxmax < LAZY_C_LIMIT and dmax * dxmax < LAZY_D_LIMIT and dmax * np.abs(case["t"]).max() < 2.0 ** 20


def _scan(route, key, nchunk, mode, ctx=None, **kw):
    """One evaluation through the scan pipeline with summarize mode ``mode``; the kernel that must run is named by the
    mode (mode 2 on a series outside the lazy regime: the plain role split)."""
    with _plan(key, nchunk, **kw) as plan:
        plan.set_summarize_mode(mode)
        kernel = KERNELS[mode] if mode < 2 or _expect_lazy(key) else KERNELS[1]
        assert plan.summarize_kernel() == kernel and _scan_runs(plan), (key, mode, plan.summarize_kernel())
        out = plan.log_likelihood()
        judge("%s (%s)" % (route, kernel), key, out, (nchunk, ctx), levels=plan.exact_levels(), quad_factor=quad_factor_of(key))
        return kernel


# ---- 1. the scan pipeline with the single-wave summarize ------------------------------------------------------------------
@pytest.mark.parametrize("JR,JC", ALL_WIDTH_SHAPES)
def test_scan_pipeline_single_wave_every_shape(JR, JC):
    """All 24 shapes at the four sizes, the automatic prefix mode and layout, both synthetic families at every size."""
    for N, nchunk in SIZES:
        for fam in SIZE_FAMILIES[N]:
            _scan("scan pipeline", ("syn", fam, JR, JC, N), nchunk, 0)


@pytest.mark.parametrize("layout", ["staged", "interleaved", "rowmajor"])
@pytest.mark.parametrize("prefix", ["single", "walk", "multilevel"])
def test_scan_pipeline_single_wave_prefix_modes_and_layouts(prefix, layout):
    """The plan reports the multi-level prefix through ``prefix_plan`` (levels >= 1); it has no getter that tells "single"
    from "walk" (both report no level) and none for the series layout: for those the setter's success is all that is
    asserted, and the case stands for "this setting gives right numbers", not for "this kernel ran"."""
    for JR, JC in ((2, 3), (1, 0), (0, 2)):
        for N, nchunk in SIZES:
            key = ("syn", "bench" if nchunk in (64, 100) else "accuracy", JR, JC, N)
            with _plan(key, nchunk, layout=layout, prefix=prefix) as plan:
                plan.set_summarize_mode(0)
                if prefix == "multilevel":   # (left to itself the plan has no level at 37 chunks: it walks them)
                    plan.set_prefix_plan(*((2, 3) if nchunk > 64 else (1, 4)))
                assert plan.summarize_kernel() == KERNELS[0] and _scan_runs(plan)
                assert (plan.prefix_plan[0] >= 1) == (prefix == "multilevel"), plan.prefix_plan
                out = plan.log_likelihood()
                judge("scan pipeline (single wave), prefix %s" % prefix, key, out, (nchunk, layout), levels=plan.exact_levels(),
                      quad_factor=quad_factor_of(key))


@pytest.mark.parametrize("JR,JC", ALL_WIDTH_SHAPES)
def test_scan_pipeline_single_wave_on_the_adversarial_family(JR, JC):
    _scan("scan pipeline", ("adv", JR, JC), ADV_CHUNKS, 0)


# ---- 2. role split, plain and lazy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("JR,JC", SPLIT_SHAPES)
def test_role_split_plain_and_lazy(JR, JC):
    for N, nchunk in SIZES:
        for fam in SIZE_FAMILIES[N]:
            key = ("syn", fam, JR, JC, N)
            _scan("scan pipeline", key, nchunk, 1)
            if fam != "bench":
                continue
            for k, b_zero in ((key, False), (("syn b=0", JR, JC, N), True)):
                if JC == 0 and b_zero:
                    continue
                with _plan(k, nchunk) as plan:
                    plan.set_summarize_mode(2)
                    assert plan.summarize_kernel() == KERNELS[2] and _scan_runs(plan), k
                    assert plan.split_variant()["b_zero"] == (b_zero and JC > 0), k
                    assert np.any(case_of(k)["b_comp"] > 0) != b_zero or JC == 0
                    out = plan.log_likelihood()
                    judge("scan pipeline (%s, %s)" % (KERNELS[2], "b_comp = 0" if b_zero else "general"), k, out, nchunk,
                          levels=plan.exact_levels(), quad_factor=quad_factor_of(k))
    # the automatic mode on a dense series at widths 7 and 8: the lazy kernel
    key = ("syn", "bench", JR, JC, 6000)
    with _plan(key, 64) as plan:
        plan.set_summarize_mode(-1)
        assert plan.summarize_kernel() == KERNELS[2] and _scan_runs(plan)
        judge("scan pipeline (%s, automatic)" % KERNELS[2], key, plan.log_likelihood(), 64, levels=plan.exact_levels(),
              quad_factor=quad_factor_of(key))


@pytest.mark.parametrize("JR,JC", SPLIT_SHAPES)
def test_role_split_on_the_adversarial_family(JR, JC):
    for mode in (1, 2):
        _scan("scan pipeline", ("adv", JR, JC), ADV_CHUNKS, mode)


# ---- structured families on routes 1 and 2 --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GRAD_FAMILIES))
def test_gradient_families_on_the_scan_pipeline_and_the_replay(name):
    """G1 .. G5 at shape (2, 3): the three summarize kernels and the forced exact replay."""
    key = ("G", name)
    for mode in (0, 1, 2):
        _scan("scan pipeline", key, STRUCT_CHUNKS, mode)
    with _plan(key, STRUCT_CHUNKS) as plan:
        plan.set_exact(True)
        out = plan.log_likelihood()
        levels = plan.exact_levels()
        assert (levels != 0).all() and _scan_runs(plan)
        judge("exact replay", key, out, STRUCT_CHUNKS, levels=levels)


@pytest.mark.parametrize("JR,JC", F_SHAPES)
@pytest.mark.parametrize("name", sorted(F_FAMILIES))
def test_output_check_families_on_the_scan_pipeline(name, JR, JC):
    """F0 .. F5 generated at narrow shapes (uniform cadence and the near-identical ladder: systematic rounding)."""
    for mode in (0, 1, 2):
        _scan("scan pipeline", ("F", name, JR, JC), STRUCT_CHUNKS, mode)


# ---- 3. the edges of the lazy regime -----------------------------------------------------------------------------------
@pytest.mark.parametrize("JR,JC", [(2, 3), (0, 4)])
@pytest.mark.parametrize("which", ["c", "d"])
def test_edges_of_the_lazy_regime(which, JR, JC):
    """cmax dxmax at 0.95 x 2^-7 (the longest step the 64-step renormalisation window carries), dmax dxmax at 0.95 x 2^-5
    (the largest rotation of the short Taylor series): the lazy kernel; at 1.05 x: not chosen, and what runs is judged."""
    for frac, kernel in ((0.95, KERNELS[2]), (1.05, KERNELS[1])):
        key = ("lazy edge", which, frac, JR, JC)
        with _plan(key, STRUCT_CHUNKS) as plan:
            plan.set_summarize_mode(-1)
            sb = plan.selection_bounds()
            at = sb["cmax"] * sb["dxmax"] / LAZY_C_LIMIT if which == "c" else sb["dmax"] * sb["dxmax"] / LAZY_D_LIMIT
            assert abs(at - frac) < 1e-6, (key, sb)
            assert plan.summarize_kernel() == kernel and _scan_runs(plan), (key, plan.summarize_kernel())
            judge("scan pipeline (%s), %s dx at %.2f of the lazy limit" % (kernel, which, frac), key, plan.log_likelihood(),
                  sb, levels=plan.exact_levels())


@pytest.mark.parametrize("JR,JC", [(2, 3), (0, 4)])
@pytest.mark.parametrize("which", ["c", "d"])
def test_every_step_at_the_edge_of_the_lazy_regime(which, JR, JC):
    """EVERY step at 0.9 .. 0.999 of the limit: in each 64-step window the decay factored out of the state comes down to
    ~e^-0.47 ("c"), every rotation between two anchors is the largest the short Taylor series takes and their
    truncations add up over the window ("d", N = 700 in 4 chunks) -- what a series with one long step cannot show."""
    key = ("lazy edge, every step", which, JR, JC)
    with _plan(key, STRUCT_CHUNKS if which == "c" else EVERY_STEP_D_CHUNKS) as plan:
        plan.set_summarize_mode(-1)
        sb = plan.selection_bounds()
        at = sb["cmax"] * sb["dxmax"] / LAZY_C_LIMIT if which == "c" else sb["dmax"] * sb["dxmax"] / LAZY_D_LIMIT
        assert 0.99 < at < 1.0, (key, sb)
        assert plan.summarize_kernel() == KERNELS[2] and _scan_runs(plan), (key, plan.summarize_kernel())
        judge("scan pipeline (%s), every %s dx at the lazy limit" % (KERNELS[2], which), key, plan.log_likelihood(), sb,
              levels=plan.exact_levels())


# ---- 4. the decay-factor regimes of features_phi_distinct --------------------------------------------------------------
@pytest.mark.parametrize("JR,JC", [(3, 0), (1, 2)])
@pytest.mark.parametrize("which", ["tiny", "small", "gaps"])
def test_decay_factor_regimes_of_the_single_wave_kernel(which, JR, JC):
    key = ("exp", which, JR, JC)
    with _plan(key, STRUCT_CHUNKS) as plan:
        plan.set_summarize_mode(0)
        sb = plan.selection_bounds()
        x = sb["cmax"] * sb["dxmax"]
        lo, hi = {"tiny": (0.89 * EXP_TINY_LIMIT, EXP_TINY_LIMIT), "small": (0.89 * EXP_SMALL_LIMIT, EXP_SMALL_LIMIT),
                  "gaps": (EXP_SMALL_LIMIT, 2 * EXP_SMALL_LIMIT)}[which]
        assert lo < x < hi, (key, sb)
        assert plan.summarize_kernel() == KERNELS[0] and _scan_runs(plan)
        judge("scan pipeline (single wave), decay factors: %s" % which, key, plan.log_likelihood(), sb,
              levels=plan.exact_levels())


# ---- 5. one launch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("JR,JC", SMALL_SHAPES)
def test_one_launch_route(JR, JC):
    """small_batch_kernel at its lower limit N = 512, 700, 4099 and (two shapes) its upper limit 32768; just outside
    (511, 32769) the mode is not active."""
    sizes = [(512, ("bench", "accuracy")), (700, ("bench", "accuracy")), (4099, ("bench", "accuracy"))]
    if (JR, JC) in ((4, 0), (0, 2)):
        sizes.append((32768, ("bench", "accuracy")))
    for N, fams in sizes:
        for fam in fams:
            key = ("syn", fam, JR, JC, N)
            with _plan(key, small=1) as plan:
                assert plan.small_mode_active() and plan.warm_start()["active"] == 0, key
                out = plan.log_likelihood()
                judge("one launch", key, out, N, levels=plan.exact_levels(), quad_factor=quad_factor_of(key))
    for N in (511, 32769):
        plan = batch.BatchedGP(2, N, JR, JC)
        try:
            plan.set_small_mode(1)
            plan.set_warm_start(0)
            t = np.sort(np.random.RandomState(N).rand(2, N), axis=1)
            plan.set_series(t, np.full((2, N), 0.02), np.sin(t))
            plan.set_coefficients(*coeffs_of(case_of(("syn", "bench", JR, JC, 512)), slice(0, 2)))
            assert not plan.small_mode_active(), N
        finally:
            plan.close()


@pytest.mark.parametrize("JR,JC", SMALL_SHAPES)
def test_one_launch_route_on_the_adversarial_family(JR, JC):
    key = ("adv", JR, JC)
    with _plan(key, small=1) as plan:
        assert plan.small_mode_active() and plan.warm_start()["active"] == 0
        out = plan.log_likelihood()
        judge("one launch", key, out, levels=plan.exact_levels())


@pytest.mark.parametrize("JR,JC", F_SMALL_SHAPES)
@pytest.mark.parametrize("name", sorted(F_FAMILIES))
def test_output_check_families_on_the_one_launch_route(name, JR, JC):
    key = ("F", name, JR, JC)
    with _plan(key, small=1) as plan:
        assert plan.small_mode_active() and plan.warm_start()["active"] == 0
        judge("one launch", key, plan.log_likelihood(), levels=plan.exact_levels(), quad_factor=quad_factor_of(key))


# ---- 6. warm start ---------------------------------------------------------------------------------------------------
def test_warm_start_route():
    """The accuracy family forgets its past: a forced warm-up of 128 steps settles every problem; one of 2 steps settles
    none (the boundary check sends them to the scan behind it); in the mixed batch the two problems with a slow decay and
    the indefinite one take the scan, the others the warm-started recurrence -- each half against its own route."""
    key = ("warm", "all")
    B = len(reference(key).s0)
    for K, settled in ((128, B), (2, 0)):
        with _plan(key, warm=(1, K)) as plan:
            assert plan.warm_start()["active"] == 1 and not plan.small_mode_active()
            out = plan.log_likelihood()
            info = plan.warm_start()
            assert info["settled"] == settled and info["fallbacks"] == B - settled, (K, info)
            judge("warm start" if settled else "scan behind the warm start", key, out, (K, info), levels=plan.exact_levels())
    key = ("warm", "mixed")
    B = len(reference(key).s0)
    behind = np.zeros(B, dtype=bool)
    behind[[3, 6, 8]] = True                 # (3, 6: not eligible; 8: flagged during the warm pass, status 2)
    with _plan(key, warm=(-1, 0)) as plan:
        assert plan.warm_start()["active"] == 1 and not plan.small_mode_active()
        out = plan.log_likelihood()
        info = plan.warm_start()
        assert info["settled"] == B - 3 > 0 and info["fallbacks"] == 3, info
        levels = plan.exact_levels()
        judge("warm start", key, out, info, subset=~behind, levels=levels)
        judge("scan behind the warm start", key, out, info, subset=behind & (reference(key).s0 == 0), levels=levels)


# ---- 7. exact replay and the rescue side plan ---------------------------------------------------------------------------
def _send_to_route1(plan, k):
    """test_gpu_batch.py, _send_to_route1: the k problems with the largest conditioning record leave route 0."""
    gamma, _ = plan.conditioning()
    order = np.argsort(gamma)[::-1]
    plan.set_certificate(max_gamma=0.5 * (gamma[order[k - 1]] + gamma[order[k]]))
    return np.sort(order[:k])


@pytest.mark.parametrize("JR,JC", [(2, 3), (0, 4), (1, 0), (1, 1)])
def test_forced_exact_replay(JR, JC):
    for N, nchunk in SIZES:
        for fam in SIZE_FAMILIES[N]:
            key = ("syn", fam, JR, JC, N)
            with _plan(key, nchunk) as plan:
                plan.set_exact(True)
                out = plan.log_likelihood()
                levels = plan.exact_levels()
                assert (levels != 0).all() and _scan_runs(plan), (key, levels)
                judge("exact replay", key, out, nchunk, levels=levels)


def test_route1_problems_inline_and_on_the_side_plan():
    """Two benign problems of eight sent to route 1 (the checked chunked replay) by the certificate's gamma bound: replayed
    inline (set_rescue(0)) and re-planned as a side plan with short chunks (set_rescue(1))."""
    key = ("route 1",)
    B = len(reference(key).s0)
    with _plan(key, 16) as plan:
        base = plan.log_likelihood()
        assert (plan.exact_levels() == 0).all() and _scan_runs(plan)
        judge("scan pipeline (%s)" % plan.summarize_kernel(), key, base, levels=plan.exact_levels())
        picked = _send_to_route1(plan, 2)
        expect = np.zeros(B, dtype=np.int32)
        expect[picked] = 1
        for mode in (0, 1):
            plan.set_rescue(mode)
            plan.set_coefficients(*coeffs_of(case_of(key)))
            out = plan.log_likelihood()
            levels, info = plan.exact_levels(), plan.rescue()
            assert np.array_equal(levels, expect), (mode, levels, picked)
            assert (info["last"] == 2) if mode else (info["last"] <= 0), (mode, info)
            judge("route 1, %s" % ("side plan" if mode else "inline replay"), key, out, (mode, info), levels=levels)


@pytest.mark.parametrize("JR,JC", [(2, 3), (0, 4), (2, 1), (8, 0)])
def test_exact_replay_and_rescue_on_the_adversarial_family(JR, JC):
    """The routes the ill-conditioned problems take by themselves (levels 0, 1, 2, each named in its line), with the
    inline replay and with the side plan, and the forced exact replay."""
    key = ("adv", JR, JC)
    seen = set()
    for mode in (0, 1):
        with _plan(key, ADV_CHUNKS) as plan:
            plan.set_rescue(mode)
            plan.set_coefficients(*coeffs_of(case_of(key)))
            out = plan.log_likelihood()
            levels, info = plan.exact_levels(), plan.rescue()
            # (8, 0): no problem of the batch leaves route 0 for the checked replay -- nothing to re-plan, and the line says so
            replanned = mode == 1 and (JR, JC) != (8, 0)
            assert _scan_runs(plan) and ((info["last"] > 0) if replanned else (info["last"] <= 0)), (mode, info)
            judged = judge("scan pipeline, %s" % ("side plan" if replanned else "inline replay" if mode == 0 else
                                                  "side plan asked for, no route-1 problem"), key, out, (mode, info), levels=levels)
            seen |= set(levels[judged].tolist())
            print("adversarial %s rescue mode %d: levels of the judged problems %s, rescue %s" %
                  ((JR, JC), mode, np.bincount(levels[judged], minlength=3), info))
    with _plan(key, ADV_CHUNKS) as plan:
        plan.set_exact(True)
        out = plan.log_likelihood()
        levels = plan.exact_levels()
        assert (levels != 0).all()
        judge("exact replay", key, out, levels=levels)
    if (JR, JC) == (0, 4):   # (its ill-conditioned problem: level 2 after the inline replay, level 1 on the side plan)
        assert seen == {0, 1, 2}, seen


# ---- 8. the materialising run -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("JR,JC", [(2, 3), (0, 4)])
@pytest.mark.parametrize("layout", ["reference", "lean"])
def test_materialising_run(layout, JR, JC):
    for fam in ("bench", "accuracy"):
        key = ("syn", fam, JR, JC, STRUCT_N)
        with _plan(key, STRUCT_CHUNKS) as plan:
            plan.set_factor_layout(layout)
            out = plan.log_likelihood(materialize=True)
            assert _scan_runs(plan) and plan.rescue()["last"] == 0 and plan.factor_bytes() > 0
            D = plan.factor(0)[3]            # (the factor is there: the values are the replay's)
            assert D.shape == (STRUCT_N,) and np.all(D > 0)
            judge("materialising run, %s factor" % layout, key, out, levels=plan.exact_levels())


# ---- 9. per-problem lengths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("JR,JC", [(2, 3), (1, 0), (0, 4)])
def test_per_problem_lengths(JR, JC):
    key = ("ragged", JR, JC)
    lengths = ragged_lengths()
    with _plan(key, STRUCT_CHUNKS, lengths=lengths) as plan:
        assert np.array_equal(plan.lengths, lengths) and plan.summarize_kernel() == KERNELS[0] and _scan_runs(plan)
        judge("scan pipeline (single wave), per-problem lengths", key, plan.log_likelihood(), levels=plan.exact_levels())


# ---- 10. library trig ----------------------------------------------------------------------------------------------------
def test_library_trig_at_large_t():
    """t ~ 3e8: max d x max t above the fast-trig limit.  The truth takes each phase as fl(d t), as the device does;
    the log-likelihood alone is judged, against 30 x the double twin's distance (floored as everywhere)."""
    case = large_t_case()
    truth, twin = large_t_reference()
    B, N = case["t"].shape
    plan = batch.BatchedGP(B, N, 2, 3)
    try:
        plan.set_small_mode(0)
        plan.set_warm_start(0)
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case), jitter=LARGE_T_JITTER)
        sb = plan.selection_bounds()
        assert sb["dmax"] * sb["tmax"] >= 1e9 and _scan_runs(plan), sb
        ll, ld, q, st = plan.log_likelihood()
        levels = plan.exact_levels()
    finally:
        plan.close()
    assert (st == 0).all()
    assert np.allclose(ll, -0.5 * (q + ld + N * np.log(2 * np.pi)), rtol=1e-14, atol=0)
    # (the gradient oracles' value carries pi log N where the plan's carries N log 2 pi: solver.cpp:415, celerite.py:214-216)
    shift = 0.5 * (np.pi * np.log(N) - N * np.log(2 * np.pi))
    truth, twin = truth + shift, twin + shift
    e_dev, e_ref = np.abs(ll - truth) / np.abs(truth), np.abs(twin - truth) / np.abs(truth)
    bar = np.minimum(FACTOR * max(e_ref.max(), np.sqrt(N) * 2.0 ** -53), REL)
    print("library trig at t ~ 3e8: loglike e_dev %s, e_ref %s, bar %.2e, levels %s" % (e_dev, e_ref, bar, levels))
    within("library trig at t ~ 3e8: loglike e_dev / (%g x Y)" % FACTOR, np.max(e_dev / bar), 1.0, (e_dev, e_ref, levels))
