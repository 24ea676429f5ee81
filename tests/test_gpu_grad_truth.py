# -*- coding: utf-8 -*-
"""Every route of the device gradient against the binary128 tangents (oracle.ref.quad_grad), per partial.

Until now the gradient's references were oracle/grad.py (double, affordable at a few thousand samples), the device's
own sequential tangent kernel and central differences, with bars relative to the LARGEST partial.  Here every partial
(or, at the wide shapes, every chosen direction) is held against the truth, with the double-precision twin of the
oracle (oracle.ref.double_grad) measured beside it on the same problem -- so each deviation has a known side.

Metrics:  per partial  |g_i - q_i| / max(|q_i|, 1e-3 max|q|);
          per direction |g.v - q_v| / max(sum |r_i v_i|, 1e-3 max|r| max|v|)   (r: the double twin's full gradient --
          the binary128 oracle is run on the chosen directions only; the scale does not depend on the device's answer).
Directions at the wide shapes: the jitter, the first and last term of each coefficient family, two random ones.
Every oracle result is computed once per module (the ``truth`` fixture).
"""
import json
import os

import numpy as np
import pytest

from celerite_amd import batch
from oracle import ref
from _cases import (ALL_WIDTH_SHAPES, GRAD_FAMILIES, GRAD_FAMILY_SHAPE, NO_GENERAL, adversarial, coeffs_of, synthetic,
                    within)

pytestmark = pytest.mark.gpu

BAR = 1e-10          # chunked routes, per partial (today's level, now against the truth)
BAR_VALUE = 1e-10    # the value, relative (as "plan gradient: value vs oracle")
BAR_SEQ = 1e-8       # the sequential tangent kernel (its bound at N = 1e5 in test_gpu_batch.py)
TWIN_BAR = 1e-6      # the double twin is recorded, not judged: a bound that only catches a broken oracle


def _nparams(JR, JC):
    return 1 + 2 * JR + 4 * JC


def _subset(JR, JC, seed=0):
    """The jitter, the first and last term of each coefficient family, two random directions over all partials."""
    G = _nparams(JR, JC)
    idx = [0]
    start = 1
    for n in (JR, JR, JC, JC, JC, JC):
        if n:
            idx += sorted({start, start + n - 1})
        start += n
    rows = np.eye(G)[idx]
    rng = np.random.RandomState(seed)
    return np.vstack([rows, rng.randn(2, G)])


def _per_partial(g, q):
    g, q = np.asarray(g), np.asarray(q)
    return float(np.max(np.abs(g - q) / np.maximum(np.abs(q), 1e-3 * np.max(np.abs(q)))))


def _direction_scale(dirs, r):
    r = np.asarray(r)
    return np.maximum(np.abs(dirs) @ np.abs(r), 1e-3 * np.max(np.abs(r)) * np.max(np.abs(dirs), axis=1))


def _per_direction(got, dirs, dq, r):
    """|got - q_v| per direction on the scale of the double twin's full gradient r (``got``: directional derivatives)."""
    return float(np.max(np.abs(np.asarray(got) - dq) / _direction_scale(dirs, r)))


class _Truth(object):
    """(value, partials or directional derivatives) in binary128 and in double, the double full gradient (the scale of
    the per-direction metric), one oracle run per key."""

    def __init__(self):
        self.cache = {}

    def __call__(self, key, jitter, coeffs, gen, t, y, diag, dirs=None, phase_in_double=False):
        if key not in self.cache:
            kw = dict(directions=dirs, phase_in_double=phase_in_double)
            q = ref.quad_grad(jitter, *coeffs, *gen, t, y, diag, **kw)
            d = ref.double_grad(jitter, *coeffs, *gen, t, y, diag, **kw)
            r = d[1] if dirs is None else ref.double_grad(jitter, *coeffs, *gen, t, y, diag, phase_in_double=phase_in_double)[1]
            self.cache[key] = (q, d, dirs, r)
        return self.cache[key]


@pytest.fixture(scope="module")
def truth():
    return _Truth()


def _judge(name, v, g, tr, bar, ctx, bar_value=BAR_VALUE):
    """Device (v, g) against the truth, the double twin recorded beside it."""
    (vq, gq), (vd, gd), dirs, r = tr
    within(name + ": value vs binary128", abs(v - vq) / abs(vq), bar_value, ctx)
    if dirs is None:
        dev, twin = _per_partial(g, gq), _per_partial(gd, gq)
        within(name + ": per partial vs binary128", dev, bar, ctx)
        within(name + ": double oracle per partial vs binary128", twin, TWIN_BAR, ctx)
    else:
        dev, twin = _per_direction(dirs @ np.asarray(g), dirs, gq, r), _per_direction(gd, dirs, gq, r)
        within(name + ": per direction vs binary128", dev, bar, ctx)
        within(name + ": double oracle per direction vs binary128", twin, TWIN_BAR, ctx)
    return dev, twin


def _judge_against_twin(name, v, g, tr, bar, ctx, JR, JC, bar_value=BAR_VALUE):
    """As _judge, where plain double precision itself is far from the truth on the d-partials (t ~ 3e8: every d-partial
    sums terms ~ t sin(d t) that cancel).  A partial / direction with any weight on a d-partial is held to
    max(bar, 30 x the double twin's worst distance on this problem) -- the device evaluates the same cancelling sums in
    another order, so its error on one direction follows the problem's scale, not the twin's luck on that direction --
    every other one to ``bar``; reported as the ratio to its bar."""
    (vq, gq), (vd, gd), dirs, r = tr
    within(name + ": value vs binary128", abs(v - vq) / abs(vq), bar_value, ctx)
    G = len(r)
    d_cols = np.arange(1 + 2 * JR + 3 * JC, 1 + 2 * JR + 4 * JC)
    if dirs is None:
        scale = np.maximum(np.abs(gq), 1e-3 * np.max(np.abs(gq)))
        dev, twin = np.abs(g - gq) / scale, np.abs(gd - gq) / scale
        on_d = np.zeros(G, dtype=bool)
        on_d[d_cols] = True
    else:
        scale = _direction_scale(dirs, r)
        dev, twin = np.abs(dirs @ g - gq) / scale, np.abs(gd - gq) / scale
        on_d = np.any(dirs[:, d_cols] != 0, axis=1)
    print("%s %s: worst %.2e (double oracle %.2e)" % (name, ctx, np.max(dev), np.max(twin)))
    print("  per partial / direction: device %s; double oracle %s; on d %s" %
          (np.array2string(dev, precision=1), np.array2string(twin, precision=1), on_d.astype(int)))
    bars = np.where(on_d, max(bar, 30 * np.max(twin)), bar)
    within(name + ": worst deviation vs binary128 / its bar (%g; d-partials: 30 x double oracle's worst)" % bar,
           np.max(dev / bars), 1.0, ctx)
    within(name + ": double oracle vs binary128 (worst partial / direction)", np.max(twin), 1e-3, ctx)


def _general(t, JG, seed):
    rng = np.random.RandomState(seed)
    z = (t - t.mean()) / (t.max() - t.min())
    U = np.vander(z, JG).T.copy()
    V = U * rng.rand(JG)[:, None]
    A = np.sum(U * V, axis=0) + 1e-8
    return A, U, V


def _problem(case, b):
    return [c[b] for c in coeffs_of(case)], case["t"][b], case["y"][b], case["diag"][b]


# ---- narrow plan (widths 1..8): clr_batch_grad, csrc/clr_grad_core.h ---------------------------------------------------
@pytest.mark.parametrize("JR,JC", ALL_WIDTH_SHAPES)
def test_narrow_plan_gradient_every_shape_against_binary128(JR, JC, truth):
    """All 24 shapes at N = 20000, one problem of each synthetic family in the plan, the automatic chunking and 7 chunks
    (a ragged last chunk), reverse / reverse with direct riders / forward."""
    N = 20000
    bench_case = synthetic(1, N, JR, JC, "bench", seed=300 + 10 * JR + JC)
    acc_case = synthetic(1, N, JR, JC, "accuracy", seed=301 + 10 * JR + JC)
    case = {k: np.concatenate([bench_case[k], acc_case[k]]) for k in bench_case}
    jit = np.array([0.05, 0.0])
    trs = []
    for b in range(2):
        co, t, y, diag = _problem(case, b)
        trs.append(truth(("narrow", JR, JC, b), jit[b], co, NO_GENERAL, t, y, diag))
    plan = batch.BatchedGP(2, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case), jitter=jit)
        for nchunk in (0, 7):
            plan.set_chunks(nchunk)
            for mode in ("reverse", "reverse-direct-riders", "forward"):
                plan.set_grad_mode(mode)
                v, g, st = plan.grad_log_likelihood()
                info = plan.grad_info()
                assert (st == 0).all() and plan.grad_fallbacks() == 0 and info["forward_reruns"] == 0, (mode, info)
                for b in range(2):
                    _judge("narrow plan gradient, %s" % mode, v[b], g[b], trs[b], BAR, (JR, JC, nchunk, b))
    finally:
        plan.close()


def test_two_level_adjoint_walk_against_binary128(truth):
    """B = 1, N = 40000 in 1000 scan chunks: hundreds of gradient chunks, the adjoint walk in two levels."""
    JR, JC, N = 2, 3, 40000
    case = synthetic(1, N, JR, JC, "bench", seed=45)
    co, t, y, diag = _problem(case, 0)
    tr = truth(("two-level",), 0.02, co, NO_GENERAL, t, y, diag)
    plan = batch.BatchedGP(1, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_chunks(1000)
        plan.set_coefficients(*coeffs_of(case), jitter=0.02)
        plan.set_grad_mode("reverse")
        v, g, st = plan.grad_log_likelihood()
        info = plan.grad_info()
        assert (st == 0).all() and info["reverse"] and info["forward_reruns"] == 0, info
        _judge("narrow plan gradient, two-level adjoint walk", v[0], g[0], tr, BAR, info)
    finally:
        plan.close()


def test_stored_state_distance_against_binary128(truth):
    """The reverse sweep's stored states at the host's distance, every 4 steps, and one per chunk (too few: the drift
    certificate sends problems to forward mode) -- right against the truth every time.  (On this family, c dt ~ 6 per
    sample, even 4 steps between stored states let the rebuilt states drift far -- measured 3e59 -- and the certificate
    reruns those problems forwards.)"""
    JR, JC, N, B = 2, 3, 6000, 2
    case = synthetic(B, N, JR, JC, "accuracy", seed=5)
    trs = []
    for b in range(B):
        co, t, y, diag = _problem(case, b)
        trs.append(truth(("distance", b), 0.0, co, NO_GENERAL, t, y, diag))
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        plan.set_chunks(8)
        for distance, reruns in ((0, False), (4, None), (750, True)):
            plan.set_grad_mode("reverse", stored_state_distance=distance)
            v, g, st = plan.grad_log_likelihood()
            info = plan.grad_info()
            assert (st == 0).all() and info["reverse"], (distance, info)
            assert reruns is None or (info["forward_reruns"] >= 1) == reruns, (distance, info)
            print("stored-state distance %d: %s" % (distance, info))
            for b in range(B):
                _judge("narrow plan gradient, stored-state distance %d" % distance, v[b], g[b], trs[b], BAR, (b, info))
    finally:
        plan.close()


@pytest.mark.parametrize("name", sorted(GRAD_FAMILIES))
def test_gradient_families_against_binary128(name, truth):
    """The adversarial families of the reverse sweep (tests/_cases.py): whatever route the plan takes -- reverse with
    its drift certificate, forward reruns, the sequential fallback -- every partial against the truth."""
    JR, JC = GRAD_FAMILY_SHAPE
    N = 20000
    c = GRAD_FAMILIES[name](N, JR, JC)
    tr = truth(("family", name), 0.01, coeffs_of(c), NO_GENERAL, c["t"], c["y"], c["diag"])
    case = {k: np.asarray(v)[None] for k, v in c.items()}
    plan = batch.BatchedGP(1, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case), jitter=0.01)
        for mode in ("reverse", "forward"):
            plan.set_grad_mode(mode)
            v, g, st = plan.grad_log_likelihood()
            info, fb = plan.grad_info(), plan.grad_fallbacks()
            assert st[0] == 0
            dev, twin = _judge("gradient families, %s" % mode, v[0], g[0], tr, BAR, (name, info, fb))
            if name.startswith("G4"):
                # the tiny term's c and d partials (~1e-8 of the largest), with no floor.  Forward mode carries their
                # tangents on their own scale: BAR (measured 2.6e-13).  The reverse sweep forms them as contractions of
                # adjoints that live on the scale of the whole gradient, so its error there is absolute, at rounding level
                # of the largest partial (measured 3.1e-16 of it; bar 1e-13) -- 9.2e-7 of the tiny partials' own size
                # (bar 1e-5).
                idx = [2 * JR + 3 * JC, 2 * JR + 4 * JC]
                gq = tr[0][1]
                err = np.abs(g[0][idx] - gq[idx])
                print("  G4 tiny term's c / d partials: %s relative, %s of the largest" %
                      (err / np.abs(gq[idx]), err / np.max(np.abs(gq))))
                within("gradient families, %s: G4 tiny term's c / d partials vs binary128 (of the largest partial)" % mode,
                       np.max(err) / np.max(np.abs(gq)), 1e-13, (info, fb))
                within("gradient families, %s: G4 tiny term's c / d partials vs binary128 (relative, unfloored)" % mode,
                       np.max(err / np.abs(gq[idx])), BAR if mode == "forward" else 1e-5, (info, fb))
            print("%s %s: per partial %.2e (double oracle %.2e); reverse %s, forward reruns %d, drift %.2e, fallbacks %d"
                  % (name, mode, dev, twin, info["reverse"], info["forward_reruns"], info["drift_max"], fb))
    finally:
        plan.close()


# ---- narrow, sequential fallback ----------------------------------------------------------------------------------------
def test_sequential_fallback_on_level2_problems_against_binary128(truth):
    """Problems the evaluation settles sequentially (level 2) take the sequential tangent kernel.  They are the
    ill-conditioned ones: the double twin is as far from the truth as their conditioning makes it, and the device -- the
    same recurrence in another operation order -- may be that far too, on other partials: the bar is BAR_SEQ or 100 x
    the double twin's worst distance, whichever is larger (measured: 2.1e-6 where the twin's worst is ~1e-6)."""
    JR, JC = 2, 3
    seen = 0
    for trial in range(6):
        B, N = 6, 3000
        case = adversarial(B, N, JR, JC, seed=4000 + trial)
        plan = batch.BatchedGP(B, N, JR, JC)
        try:
            plan.set_series(case["t"], case["diag"], case["y"])
            plan.set_coefficients(*coeffs_of(case))
            v, g, st = plan.grad_log_likelihood()
            levels = plan.exact_levels()
        finally:
            plan.close()
        for b in np.nonzero((st == 0) & (levels >= 2))[0]:
            co, t, y, diag = _problem(case, b)
            tr = truth(("level2", trial, b), 0.0, co, NO_GENERAL, t, y, diag)
            twin = _per_partial(tr[1][1], tr[0][1])
            dev = _per_partial(g[b], tr[0][1])
            print("level 2 (trial %d, problem %d): per partial %.2e, double oracle %.2e" % (trial, b, dev, twin))
            within("sequential fallback (level 2): per partial vs binary128 / max(1e-8, 100 x double oracle)",
                   dev / max(BAR_SEQ, 100 * twin), 1.0, (trial, b, dev, twin))
            within("sequential fallback (level 2): double oracle per partial vs binary128", twin, 1.0, (trial, b))
            seen += 1
    assert seen >= 1


def test_library_trig_fallback_at_large_t_against_binary128(truth):
    """A series offset to t ~ 3e8: max d x max t above the fast-trig limit, so the narrow plan hands every problem to
    the sequential tangent kernel with library sincos.  The truth takes the phase as fl(d t), as the device does."""
    JR, JC, N, B = 2, 3, 4000, 2
    case = synthetic(B, N, JR, JC, "accuracy", seed=8)
    case["t"] = case["t"] + 3e8
    assert np.max(case["d_comp"]) * np.max(case["t"]) > 1e9
    trs = []
    for b in range(B):
        co, t, y, diag = _problem(case, b)
        trs.append(truth(("large-t narrow", b), 0.03, co, NO_GENERAL, t, y, diag, phase_in_double=True))
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case), jitter=0.03)
        v, g, st = plan.grad_log_likelihood()
        assert (st == 0).all() and plan.grad_fallbacks() == B
    finally:
        plan.close()
    for b in range(B):
        _judge_against_twin("sequential fallback, library trig at t ~ 3e8", v[b], g[b], trs[b], BAR_SEQ, b, JR, JC)


# ---- wide plans ---------------------------------------------------------------------------------------------------------
def _wide_plan_run(JR, JC, JG, N, nchunks, truth, key, t_offset=0.0, seed=0, expect_fallback=None):
    case = synthetic(1, N, JR, JC, "bench", seed=seed)
    case["t"] = case["t"] + t_offset
    co, t, y, diag = _problem(case, 0)
    gen = _general(t, JG, seed) if JG else NO_GENERAL
    dirs = _subset(JR, JC, seed)
    tr = truth(key, 0.05, co, gen, t, y, diag, dirs=dirs, phase_in_double=t_offset > 0)
    plan = batch.BatchedGP(1, N, JR, JC)
    out = []
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        if JG:
            plan.set_general(gen[0][None], gen[1][None], gen[2][None])
        for nchunk in nchunks:
            plan.set_chunks(nchunk)
            plan.set_coefficients(*coeffs_of(case), jitter=0.05)
            v, g, st = plan.grad_log_likelihood()
            assert st[0] == 0
            out.append((nchunk, v[0], g[0], plan.grad_fallbacks()))
    finally:
        plan.close()
    return tr, out


@pytest.mark.parametrize("JR,JC,JG", [(1, 6, 0), (2, 11, 0), (2, 3, 4), (1, 12, 5)])
def test_wide_plan_gradient_9_to_32_against_binary128(JR, JC, JG, truth):
    """Widths 9..32 (padded 16 and 32: wide_grad2_kernel / wide_grad_riders_kernel), general terms at total width
    <= 32, 4 and 11 chunks of N = 6000."""
    tr, out = _wide_plan_run(JR, JC, JG, 6000, (4, 11), truth, ("wide", JR, JC, JG), seed=17 + JR + 5 * JC + JG)
    for nchunk, v, g, fb in out:
        assert fb == 0
        _judge("wide plan gradient 9..32", v, g, tr, BAR, (JR, JC, JG, nchunk))


@pytest.mark.parametrize("JR,JC", [(2, 16), (0, 25), (64, 0), (2, 31)])
def test_wide_plan_gradient_33_to_64_against_binary128(JR, JC, truth):
    """Widths 33..64 (wide_grad_riders64_kernel, wide_grad_kernel<64>): N = 6000 in 4 chunks, and the one-chunk plan
    (the sequential tangent kernel, counted as a fallback)."""
    tr, out = _wide_plan_run(JR, JC, 0, 6000, (4, 1), truth, ("wide64", JR, JC), seed=3 + JR + JC)
    for nchunk, v, g, fb in out:
        assert (fb == 1) == (nchunk == 1)
        _judge("wide plan gradient 33..64" + (" (one chunk: sequential)" if nchunk == 1 else ""), v, g, tr,
               BAR, (JR, JC, nchunk))


@pytest.mark.parametrize("JR,JC", [(1, 6), (2, 11)])
def test_wide_plan_gradient_library_trig_against_binary128(JR, JC, truth):
    """The <JP, false> instantiations of the chunked wide tangents: t ~ 3e8, max d x max t above the fast-trig limit;
    the truth takes the phase as fl(d t) in double (the value is also recorded against exact phases).  The d-partials
    carry a factor t ~ 3e8 whose terms cancel: there each direction is held to 30 x the double recurrence's own
    distance.  (The lazy summaries, which rotate the phases instead of taking sincos of fl(d t), once settled this case
    ~3e-4 from the truth at padded width 32; test_lazy_phase_rotation_is_off_at_large_phases pins them off here.)"""
    tr, out = _wide_plan_run(JR, JC, 0, 6000, (4,), truth, ("wide-large-t", JR, JC), t_offset=3e8, seed=29 + JC)
    case = synthetic(1, 6000, JR, JC, "bench", seed=29 + JC)
    co, t, y, diag = _problem(case, 0)
    vx = truth(("wide-large-t exact phase", JR, JC), 0.05, co, NO_GENERAL, t + 3e8, y, diag, dirs=tr[2])[0][0]
    for nchunk, v, g, fb in out:
        assert fb == 0                   # the chunked <JP, false> tangents, not the sequential kernel
        within("wide plan gradient, library trig at t ~ 3e8: value vs binary128 with exact phases (recorded)",
               abs(v - vx) / abs(vx), 1e-6, (JR, JC))
        _judge_against_twin("wide plan gradient, library trig at t ~ 3e8", v, g, tr, BAR, (JR, JC, nchunk, fb), JR, JC)


# ---- object API: CholeskySolver.grad_log_likelihood (csrc/api_solver.hip) ---------------------------------------------
# routes of clr_solver_debug_grad_route: 0 sequential tangent kernel, 1 narrow plan, 2 wide plan, 3 any-width kernel
@pytest.mark.parametrize("JR,JC,JG,N,option,route", [
    (2, 3, 0, 2000, None, 1),                   # narrow plan (N >= 1024)
    (2, 3, 0, 800, None, 0),                    # sequential tangent kernel
    (1, 6, 0, 5000, None, 2),                   # wide plan (N >= 4096)
    (1, 6, 0, 3000, None, 0),                   # sequential below it
    (3, 30, 4, 2000, None, 3),                  # width 67: grad_any
    (2, 62, 4, 2000, None, 3),                  # width 130: grad_any
    (0, 20, 0, 3000, "CLR_GRAD_ANY_WIDTH", 3),  # grad_any forced at width 40
])
def test_object_api_gradient_routes_against_binary128(JR, JC, JG, N, option, route, truth):
    import celerite_amd

    case = synthetic(1, N, JR, JC, "accuracy", seed=50 + JR + JC + N % 97)
    co, t, y, diag = _problem(case, 0)
    gen = _general(t, JG, JC) if JG else NO_GENERAL
    W = JR + 2 * JC
    dirs = None if W <= 8 else _subset(JR, JC, W)
    tr = truth(("object", JR, JC, JG, N, option), 0.05, co, gen, t, y, diag, dirs=dirs)
    solver = celerite_amd.CholeskySolver()
    if option:
        with batch.option(option):
            v, g = solver.grad_log_likelihood(0.05, *co, *gen, t, y, diag)
    else:
        v, g = solver.grad_log_likelihood(0.05, *co, *gen, t, y, diag)
    assert solver._grad_route() == route
    chunked = route in (1, 2)
    _judge("object API gradient, %s" % ("chunked" if chunked else "sequential"), v, g, tr,
           BAR if chunked else BAR_SEQ, (JR, JC, JG, N, option))


# ---- one-shot batch_grad_log_likelihood, the sequential batched form (N < 512) ----------------------------------------
@pytest.mark.parametrize("JR,JC", [(2, 5), (0, 20)])
def test_one_shot_batched_gradient_shared_series_against_binary128(JR, JC, truth):
    B, N = 3, 400
    case = synthetic(B, N, JR, JC, "accuracy", seed=60 + JC)
    t, diag, y = case["t"][0], case["diag"][0], case["y"][0]
    jit = np.array([0.0, 0.01, 0.2])
    v, g, st = batch.batch_grad_log_likelihood(*coeffs_of(case), t, diag, y, jitter=jit)
    assert (st == 0).all()
    for b in range(B):
        co = [c[b] for c in coeffs_of(case)]
        tr = truth(("one-shot", JR, JC, b), jit[b], co, NO_GENERAL, t, y, diag, dirs=_subset(JR, JC, b))
        _judge("one-shot batched gradient (sequential, t_stride = 0)", v[b], g[b], tr, BAR_SEQ, (JR, JC, b))


# ---- the headline shape -------------------------------------------------------------------------------------------------
def test_headline_shape_gradient_routes_against_binary128(truth):
    """The golden problem (N = 1e5, width 8): reverse and forward plan gradients, the object API and the sequential
    tangent kernel against binary128 per partial, the double-precision fixture tests/golden/grad_n1e5_w8.json beside."""
    import bench
    import celerite_amd

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grad_n1e5_w8.json")) as f:
        gold = json.load(f)
    N, JR, JC, jit = gold["N"], gold["J_real"], gold["J_comp"], gold["jitter"]
    coeffs, t, diag, y = bench.make_inputs(2, N, JR, JC, 42)
    co = [c[0] for c in coeffs]
    tr = truth(("headline",), jit, co, NO_GENERAL, t[0], y[0], diag[0])
    gq = tr[0][1]
    within("headline N = 1e5: fixture (double oracle) per partial vs binary128", _per_partial(gold["grad"], gq), 1e-11)
    plan = batch.BatchedGP(2, N, JR, JC)
    try:
        plan.set_series(t, diag, y)
        plan.set_coefficients(*coeffs, jitter=jit)
        plan.set_chunks(64)
        for mode in ("reverse", "forward"):
            plan.set_grad_mode(mode)
            v, g, st = plan.grad_log_likelihood()
            assert (st == 0).all() and plan.grad_fallbacks() == 0 and plan.grad_info()["forward_reruns"] == 0
            _judge("headline N = 1e5, plan %s" % mode, v[0], g[0], tr, BAR, mode)
    finally:
        plan.close()
    v1, g1 = celerite_amd.CholeskySolver().grad_log_likelihood(jit, *co, *NO_GENERAL, t[0], y[0], diag[0])
    _judge("headline N = 1e5, object API", v1, g1, tr, BAR, None)
    with batch.option("CLR_GRAD_SEQUENTIAL"):
        v2, g2, st2 = batch.batch_grad_log_likelihood(*[c[:1] for c in coeffs], t[:1], diag[:1], y[:1], jitter=jit)
    assert st2[0] == 0
    _judge("headline N = 1e5, sequential tangent kernel", v2[0], g2[0], tr, BAR_SEQ, None)


def test_lazy_phase_rotation_is_off_at_large_phases():
    """The lazy summaries rotate every (cos, sin) pair through d dt between anchors instead of taking sincos of fl(d t)
    at each sample, as the reference does; the two differ by the rounding of d t.  They run on dense series whose
    max |d| max |t| stays below 2^20 (csrc/api_internal.h, lazy_phases_ok) -- the same series shifted to t ~ 3e8 takes the
    plain summarize, at widths 7..8 (role split) and on wide plans."""
    for JR, JC, N, nchunk, lazy, plain in ((2, 3, 20000, 0, "role split, lazy decay", "role split"),
                                           (2, 11, 6000, 4, "role split, lazy decay", "single wave")):
        case = synthetic(1, N, JR, JC, "bench", seed=29 + JC)
        plan = batch.BatchedGP(1, N, JR, JC)
        try:
            plan.set_chunks(nchunk)
            plan.set_series(case["t"], case["diag"], case["y"])
            plan.set_coefficients(*coeffs_of(case))
            assert plan.summarize_kernel() == lazy, (JR, JC)
            plan.set_series(case["t"] + 3e8, case["diag"], case["y"])
            assert plan.summarize_kernel() == plain, (JR, JC)
        finally:
            plan.close()
