# -*- coding: utf-8 -*-
"""`-m gpu`: per-problem series lengths on batched plans (``BatchedGP.set_series(..., lengths=)``,
``clr_batch_set_series_ragged``).  Problem ``b`` of a plan of ``N`` samples holds ``n_b <= N``; its log-determinant,
quadratic form, log-likelihood, gradient and status must be those of ``t[b, :n_b]``, ``diag[b, :n_b]``, ``y[b, :n_b]``
alone -- the oracle is ``oracle.ref.RefSolver`` / ``oracle.grad`` on exactly those slices -- whatever the rest of the row
holds (the tests fill it with NaN).

Bars (the project's own): ``REL = 1e-10`` relative on the log-determinant, the quadratic form and the log-likelihood
(tests/test_gpu_batch.py); 1e-10 on the gradient's value and on its partials relative to the largest partial
(test_plan_gradient_parallel_in_n).  Every deviation goes through ``_cases.within`` (the worst per name is printed at the
end of the session) and the worst of each test is printed by the test itself.

Largest deviations measured on an MI355X (the run of this file, 47 tests in 6.4 s), every bar 1e-10:
  every narrow shape (20 shapes x N = 130, 1000 x bench, accuracy)          8.3e-12   (shape (3, 0); the rest <= 2.4e-13)
  summarize modes -1, 0 at widths 7 / 8 (single-wave kernel; 1, 2 refused)  2.1e-13 / 1.4e-12
  layouts, prefix modes, forced exact, plans of one chunk                   1.3e-14
  route-1 problems, inline replay and re-planned side plan                  9.0e-15
  the small-mode shape / a warm-start shape with lengths                    2.7e-15 / 3.5e-15
  neighbours of an indefinite short problem                                 1.0e-15
  gradient vs oracle.grad: value                                            2.8e-15
  gradient partials (of the largest): reverse / direct riders / forward     2.3e-13 / 3.0e-13 / 3.7e-14
  under a constant mean: value / partials / d/dmu (also sequential kernel)  2.0e-15 / 6.4e-14 / 9.2e-14
  from kernel parameters: values / grad_parameters vs the chain rule        8.0e-14 / 0.22 of its bound
  linear mean with fresh weights vs y - mean over [:n_b] on the host        1.4e-14
  bit-for-bit: lengths all N vs none; NaN / descending tails vs held tails; 2 and 3 shards vs one plan -- equal
"""
import ctypes as C

import numpy as np
import pytest

from celerite_amd import batch, terms
from oracle import ref
from _cases import ALL_WIDTH_SHAPES, synthetic, coeffs_of, within

pytestmark = pytest.mark.gpu
REL = 1e-10
EMPTY, EMPTY2 = np.empty(0), np.empty((0, 0))
LOG2PI = 1.8378770664093453
CLR_UNSUPPORTED = 7          # include/celerite_hip.h
_ip = C.POINTER(C.c_int)
_dp = C.POINTER(C.c_double)

# the two plan sizes of the issue: N = 130 in two chunks of 72, N = 1000 in 21 chunks of 48 -- a one-sample problem, both
# sides of a chunk edge, one exactly on it, chunks that are all padding, the full length
SIZES = {130: (2, 72, [1, 2, 71, 72, 73, 100, 129, 130]), 1000: (24, 48, [1, 2, 47, 48, 49, 96, 999, 1000])}


def oracle(case, lens, jitter=0.0):
    """``(loglike, logdet, quad, status)`` of every problem's first ``lens[b]`` samples by ``RefSolver``."""
    B = len(lens)
    jit = np.broadcast_to(np.asarray(jitter, dtype=float), (B,))
    ll, ld, q, st = np.full(B, -np.inf), np.full(B, np.nan), np.full(B, np.nan), np.zeros(B, dtype=np.int32)
    for b, n in enumerate(lens):
        s = ref.RefSolver()
        try:
            s.compute(jit[b], *coeffs_of(case, b), EMPTY, EMPTY2, EMPTY2, case["t"][b, :n], case["diag"][b, :n])
            ld[b] = s.log_determinant()
            q[b] = s.dot_solve(case["y"][b, :n])
            ll[b] = -0.5 * (q[b] + ld[b] + n * LOG2PI)
        except ref.RefLinAlgError:
            st[b] = 2
    return ll, ld, q, st


def garbage_tail(case, lens, kind="nan"):
    """Copies of t, diag, y whose entries past each problem's length are NaN (``kind="nan"``), NaN with DESCENDING times
    ("descending"), or copies of the problem's last sample ("held")."""
    t, diag, y = case["t"].copy(), case["diag"].copy(), case["y"].copy()
    for b, n in enumerate(lens):
        m = t.shape[1] - n
        if kind == "held":
            t[b, n:], diag[b, n:], y[b, n:] = t[b, n - 1], diag[b, n - 1], y[b, n - 1]
        else:
            diag[b, n:], y[b, n:] = np.nan, np.nan
            t[b, n:] = np.nan if kind == "nan" else t[b, 0] - 1.0 - np.arange(m)
    return t, diag, y


def deviation(got, want):
    """Largest relative deviation of (loglike, logdet, quad) over the problems the oracle factorised; statuses must
    be equal and a failed problem keeps the quiet semantics."""
    ll, ld, q, st = got
    l0, d0, q0, s0 = want
    assert np.array_equal(st, s0), (st, s0)
    ok = s0 == 0
    assert np.all(np.isneginf(ll[~ok]))
    return max(float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) for a, b in ((ld, d0), (q, q0), (ll, l0)))


def ragged_plan(case, lens, nchunk, tail="nan", **settings):
    B, N = case["t"].shape
    plan = batch.BatchedGP(B, N, case["a_real"].shape[1], case["a_comp"].shape[1])
    if nchunk is not None:
        plan.set_chunks(nchunk)
    for name, value in settings.items():
        getattr(plan, "set_" + name)(value)
    plan.set_series(*garbage_tail(case, lens, tail), lengths=lens)
    plan.set_coefficients(*coeffs_of(case), jitter=case.get("jitter", 0.0))
    return plan


def _send_to_route1(plan, k):
    """(tests/test_gpu_batch.py) the bound on gamma_max just below the k-th largest conditioning record: exactly the k
    problems with the largest gamma leave route 0 -- benign problems on the checked route."""
    gamma, _ = plan.conditioning()
    order = np.argsort(gamma)[::-1]
    plan.set_certificate(max_gamma=0.5 * (gamma[order[k - 1]] + gamma[order[k]]))
    return np.sort(order[:k])


# ---- 1. every narrow shape ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("JR,JC", ALL_WIDTH_SHAPES)
def test_every_narrow_shape(JR, JC):
    worst = 0.0
    for N, (nchunk, L, lens) in SIZES.items():
        for family in ("bench", "accuracy"):
            case = synthetic(8, N, JR, JC, family, seed=N + 10 * JR + JC)
            want = oracle(case, lens)
            plan = ragged_plan(case, lens, nchunk)
            try:
                assert plan.chunks == ((N + L - 1) // L, L)
                assert np.array_equal(plan.lengths, lens)
                dev = deviation(plan.log_likelihood(), want)
                # benign families: no problem may fall to the sequential recurrence because of its padding chunks
                assert (plan.exact_levels() < 2).all(), plan.exact_levels()
            finally:
                plan.close()
            within("ragged plan, every narrow shape: vs oracle on the truncated series", dev, REL, (JR, JC, N, family))
            worst = max(worst, dev)
    print("(%d, %d): worst deviation from the oracle %.2e" % (JR, JC, worst))


# ---- 2. routes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("JR,JC", [(1, 3), (2, 3)])
def test_every_summarize_mode_at_widths_7_and_8(JR, JC):
    """The choice made for the role-split summarize of widths 7 and 8 (modes 1 and 2; what mode -1 picks on uniform
    plans of these widths): it does not carry per-problem lengths.  On sparse and on dense series (where a uniform plan
    takes the lazy role split) a plan with lengths runs the single-wave kernel under the modes -1 and 0 and says so;
    forcing mode 1 or 2 is refused, and so are lengths on a plan where one of them is forced -- the plan stays as it was."""
    N, (nchunk, L, lens) = 1000, SIZES[1000]
    worst = 0.0
    for family, scale, lazy in (("bench", 1.0, False), ("accuracy", 1.0, False), ("bench", 0.01, True)):
        case = synthetic(8, N, JR, JC, family, seed=3 + JR)
        case["t"] = case["t"] * scale  # (x 0.01: dense enough for the lazy-decay flavour of the role split)
        want = oracle(case, lens)
        uni = batch.BatchedGP(8, N, JR, JC)
        try:
            uni.set_chunks(nchunk)
            uni.set_series(case["t"], case["diag"], case["y"])
            uni.set_coefficients(*coeffs_of(case))
            if lazy:
                assert uni.summarize_kernel() == "role split, lazy decay"     # (what the uniform plan of this case runs)
            for mode in (1, 2):      # forced first, lengths second: refused, the uniform series stays in force
                uni.set_summarize_mode(mode)
                before = uni.log_likelihood()
                with pytest.raises(RuntimeError, match=r"unsupported configuration.*role-split"):
                    uni.set_series(*garbage_tail(case, lens), lengths=lens)
                assert np.array_equal(uni.lengths, np.full(8, N)) and uni.summarize_kernel().startswith("role split")
                assert all(np.array_equal(a, b) for a, b in zip(before, uni.log_likelihood()))
        finally:
            uni.close()
        for mode in (-1, 0):
            plan = ragged_plan(case, lens, nchunk, summarize_mode=mode)
            try:
                kernel = plan.summarize_kernel()
                assert kernel == "single wave"
                dev = deviation(plan.log_likelihood(), want)
                for forced in (1, 2):
                    with pytest.raises(RuntimeError, match=r"unsupported configuration.*lengths"):
                        plan.set_summarize_mode(forced)
                assert plan.summarize_kernel() == "single wave"
                assert deviation(plan.log_likelihood(), want) == dev
            finally:
                plan.close()
            within("ragged plan, summarize modes of widths 7, 8: vs oracle", dev, REL, (JR, JC, family, scale, mode, kernel))
            worst = max(worst, dev)
    print("width %d: worst deviation over the summarize modes %.2e" % (JR + 2 * JC, worst))


def test_layouts_prefix_modes_and_forced_exact():
    N, (nchunk, L, lens) = 1000, SIZES[1000]
    case = synthetic(8, N, 1, 2, "bench", seed=21)
    want = oracle(case, lens)
    worst = 0.0
    runs = [dict(layout=l) for l in ("staged", "interleaved", "rowmajor")]
    runs += [dict(prefix_mode=m) for m in ("single", "walk", "multilevel")]
    runs += [dict(exact=True), dict(exact=True, layout="interleaved")]
    for settings in runs:
        plan = ragged_plan(case, lens, nchunk, **settings)
        try:
            dev = deviation(plan.log_likelihood(), want)
            if "exact" in settings:
                assert (plan.exact_levels() >= 1).all()
        finally:
            plan.close()
        within("ragged plan, layouts / prefix modes / forced exact: vs oracle", dev, REL, settings)
        worst = max(worst, dev)
    # a plan of ONE chunk (the replay from the zero state is the whole recurrence) and the smallest plans
    for N1, lens1 in ((100, [1, 2, 50, 99, 100, 64, 7, 100]), (2, [1, 2, 1, 2, 2, 1, 1, 2])):
        c1 = synthetic(8, N1, 1, 2, "accuracy", seed=N1)
        plan = ragged_plan(c1, lens1, None)
        try:
            dev = deviation(plan.log_likelihood(), oracle(c1, lens1))
        finally:
            plan.close()
        within("ragged plan of one chunk: vs oracle", dev, REL, N1)
        worst = max(worst, dev)
    print("layouts, prefix modes, forced exact, one chunk: worst deviation %.2e" % worst)


@pytest.mark.parametrize("rescue", [0, 1])
def test_checked_replay_inline_and_replanned(rescue):
    """Two benign problems are sent to route 1 (the checked chunked replay) by lowering the bound on gamma_max, as in
    test_route1_replanning_on_a_narrow_plan_and_its_fallbacks: replayed inline (set_rescue(0)) and re-planned as a side
    plan that carries their lengths (set_rescue(1))."""
    N, (nchunk, L, lens) = 1000, SIZES[1000]
    lens = [600, 48, 47, 700, 999, 49, 300, 96]           # (no full length: whichever problems are picked are short ones)
    case = synthetic(8, N, 2, 3, "bench", seed=515)
    want = oracle(case, lens)
    plan = ragged_plan(case, lens, nchunk, rescue=rescue)
    try:
        plan.set_certificate(max_gamma=1e4)
        base = plan.log_likelihood()
        assert (plan.exact_levels() == 0).all()
        picked = _send_to_route1(plan, 2)
        plan.set_coefficients(*coeffs_of(case))
        got = plan.log_likelihood()
        levels = plan.exact_levels()
        assert np.array_equal(np.flatnonzero(levels), picked) and (levels[picked] == 1).all(), levels
        assert plan.rescue()["last"] == (2 if rescue else 0), plan.rescue()
        dev = deviation(got, want)
        within("ragged plan, route-1 problems (rescue %d): vs oracle" % rescue, dev, REL, picked)
        rest = np.setdiff1d(np.arange(8), picked)
        assert np.array_equal(got[1][rest], base[1][rest]) and np.array_equal(got[2][rest], base[2][rest])
        print("rescue %d: problems %s of lengths %s on route 1, worst deviation %.2e" % (rescue, picked, np.asarray(lens)[picked], dev))
    finally:
        plan.close()


def test_warm_start_and_small_mode_stay_off_and_refuse_forcing():
    """The choice made for the warm-started recurrence and the one-launch small mode: both are switched off while
    lengths are in force, report it, and refuse to be forced."""
    N, (nchunk, L, lens) = 1000, SIZES[1000]
    case = synthetic(8, N, 0, 2, "bench", seed=5)        # (a family that does not forget: no warm start, the one launch)
    want = oracle(case, lens)
    plan = batch.BatchedGP(8, N, 0, 2)
    try:
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        assert plan.small_mode_active()                      # (the uniform plan of this shape takes the one launch)
        plan.set_series(*garbage_tail(case, lens), lengths=lens)
        plan.set_coefficients(*coeffs_of(case))
        assert not plan.small_mode_active() and not plan.warm_start()["active"]
        for force in (lambda: plan.set_small_mode(1), lambda: plan.set_warm_start(1, 16)):
            with pytest.raises(RuntimeError, match=r"unsupported configuration.*lengths"):
                force()
        dev = deviation(plan.log_likelihood(), want)
        within("ragged plan at the small-mode shape: vs oracle", dev, REL)
        # forced first, lengths second: the lengths are refused and the plan keeps its uniform series
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_small_mode(1)
        plan.set_coefficients(*coeffs_of(case))
        uniform = plan.log_likelihood()
        with pytest.raises(RuntimeError, match=r"unsupported configuration"):
            plan.set_series(*garbage_tail(case, lens), lengths=lens)
        assert np.array_equal(plan.lengths, np.full(8, N))
        plan.set_coefficients(*coeffs_of(case))
        again = plan.log_likelihood()
        assert all(np.array_equal(a, b) for a, b in zip(uniform, again))
        plan.set_small_mode(-1)
        # a batch of the accuracy family on the warm path when uniform (512 <= N), off with lengths
        big = synthetic(8, 4096, 0, 2, "accuracy", seed=6)
        lens_big = [512, 4096, 4095, 300, 2049, 2048, 1, 4000]
        wplan = batch.BatchedGP(8, 4096, 0, 2)
        try:
            wplan.set_small_mode(0)
            wplan.set_series(big["t"], big["diag"], big["y"])
            wplan.set_coefficients(*coeffs_of(big))
            assert wplan.warm_start()["active"]
            wplan.set_series(*garbage_tail(big, lens_big), lengths=lens_big)
            wplan.set_coefficients(*coeffs_of(big))
            assert not wplan.warm_start()["active"]
            dev2 = deviation(wplan.log_likelihood(), oracle(big, lens_big))
            within("ragged plan at a warm-start shape: vs oracle", dev2, REL)
        finally:
            wplan.close()
        print("small-mode shape %.2e, warm-start shape %.2e" % (dev, dev2))
    finally:
        plan.close()


def test_an_indefinite_short_problem_keeps_the_quiet_semantics():
    N, (nchunk, L, lens) = 1000, SIZES[1000]
    case = synthetic(8, N, 2, 3, "accuracy", seed=9)
    case["a_real"][2:3] *= -50.0       # length 47: indefinite inside its own samples
    case["jitter"] = np.array([0.0, 0.01, 0.0, 0.1, 0.0, 0.3, 0.0, 0.0])
    want = oracle(case, lens, case["jitter"])
    assert want[3][2] == 2 and (want[3][[0, 1, 3, 4, 5, 6, 7]] == 0).all()
    clean = dict(case, a_real=np.abs(case["a_real"]))
    worst = 0.0
    for settings in (dict(), dict(exact=True), dict(layout="interleaved")):
        plan = ragged_plan(case, lens, nchunk, **settings)
        ref_plan = ragged_plan(clean, lens, nchunk, **settings)
        try:
            got = plan.log_likelihood()
            dev = deviation(got, want)
            base = ref_plan.log_likelihood()
            ok = [0, 1, 3, 4, 5, 6, 7]   # the neighbours: the same bits as in a batch without the indefinite problem
            assert all(np.array_equal(a[ok], b[ok]) for a, b in zip(got, base))
        finally:
            plan.close()
            ref_plan.close()
        within("ragged plan with an indefinite short problem: vs oracle", dev, REL, settings)
        worst = max(worst, dev)
    print("indefinite short problem: statuses %s, worst deviation of the others %.2e" % (want[3], worst))


# ---- 3. gradient -------------------------------------------------------------------------------------------------------
GRAD_LENS = [512, 1200, 2499, 2500, 700]
GRAD_JITTER = np.array([0.0, 0.01, 0.1, 0.3, 0.0])
_GRAD = {}


def grad_reference(JR, JC, family="bench", mean=None):
    """The case and ``oracle.grad`` on every problem's truncated series, computed once per session."""
    key = (JR, JC, family, None if mean is None else tuple(mean))
    if key not in _GRAD:
        from oracle import grad as ograd
        case = synthetic(5, 2500, JR, JC, family, seed=77 + JR + 10 * JC)
        v0, g0 = [], []
        for b, n in enumerate(GRAD_LENS):
            y = case["y"][b, :n] - (0.0 if mean is None else mean[b])
            v, g = ograd.grad_log_likelihood(GRAD_JITTER[b], *coeffs_of(case, b), EMPTY, EMPTY2, EMPTY2, case["t"][b, :n], y,
                                             case["diag"][b, :n])
            v0.append(v)
            g0.append(g)
        _GRAD[key] = (case, np.array(v0), np.array(g0))
    return _GRAD[key]


def grad_deviation(v, g, v0, g0):
    dv = float(np.max(np.abs(v - v0) / np.abs(v0)))
    dg = float(np.max(np.abs(g - g0) / np.max(np.abs(g0), axis=1, keepdims=True)))
    return dv, dg


@pytest.mark.parametrize("mode", ["reverse", "reverse-direct-riders", "forward"])
@pytest.mark.parametrize("JR,JC", [(2, 3), (1, 1)])
def test_gradient_on_the_truncated_series(JR, JC, mode):
    """A length below 512 does not occur here (the shortest is 512), one does in the next test: N >= 512 is a property of
    the plan.  The gradient's value carries the reference's constant pi log n_b of the problem's own length."""
    case, v0, g0 = grad_reference(JR, JC)
    plan = batch.BatchedGP(5, 2500, JR, JC)
    worst = (0.0, 0.0)
    try:
        plan.set_series(*garbage_tail(case, GRAD_LENS), lengths=GRAD_LENS)
        plan.set_coefficients(*coeffs_of(case), jitter=GRAD_JITTER)
        plan.set_grad_mode(mode)
        for nchunk in (0, 5, 40):
            plan.set_chunks(nchunk)
            v, g, st = plan.grad_log_likelihood()
            info = plan.grad_info()
            assert (st == 0).all() and info["reverse"] == (mode != "forward") and info["forward_reruns"] == 0, (st, info)
            assert plan.grad_fallbacks() == 0
            dv, dg = grad_deviation(v, g, v0, g0)
            within("ragged plan gradient %s: value vs oracle.grad" % mode, dv, 1e-10, (JR, JC, nchunk))
            within("ragged plan gradient %s: partials vs oracle.grad (of the largest partial)" % mode, dg, 1e-10, (JR, JC, nchunk))
            assert (g[GRAD_JITTER <= 2.3e-16, 0] == 0.0).all()      # solver.cpp:379-389
            worst = (max(worst[0], dv), max(worst[1], dg))
    finally:
        plan.close()
    print("(%d, %d) %s: value %.2e, partials %.2e" % (JR, JC, mode, worst[0], worst[1]))


def test_gradient_with_a_length_below_512_a_mean_and_the_sequential_fallback():
    from oracle import grad as ograd
    B, N, JR, JC = 5, 2500, 1, 1
    lens = [100, 1, 2500, 511, 48]
    case = synthetic(B, N, JR, JC, "bench", seed=4)      # (a family that does not forget: replayed end states differ from
    mu = np.array([0.3, -0.2, 0.0, 1.5, 0.7])            #  the scanned start states in their last bits)
    v0, g0, m0 = np.empty(B), np.empty((B, 7)), np.empty(B)
    for b, n in enumerate(lens):
        r = case["y"][b, :n] - mu[b]
        v0[b], g0[b] = ograd.grad_log_likelihood(GRAD_JITTER[b], *coeffs_of(case, b), EMPTY, EMPTY2, EMPTY2, case["t"][b, :n], r,
                                                 case["diag"][b, :n])
        s = ref.RefSolver()
        s.compute(GRAD_JITTER[b], *coeffs_of(case, b), EMPTY, EMPTY2, EMPTY2, case["t"][b, :n], case["diag"][b, :n])
        m0[b] = float(np.sum(s.solve(r)))           # d loglike / d mu = 1^T K^-1 r
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_mean(mu)
        plan.set_series(*garbage_tail(case, lens), lengths=lens)
        plan.set_coefficients(*coeffs_of(case), jitter=GRAD_JITTER)
        for mode, nchunk in (("reverse", 0), ("forward", 40), ("reverse", 5)):
            plan.set_grad_mode(mode)
            plan.set_chunks(nchunk)
            v, g, dm, st = plan.grad_log_likelihood(mean_partial=True)
            assert (st == 0).all()
            dv, dg = grad_deviation(v, g, v0, g0)
            dmu = float(np.max(np.abs(dm - m0) / np.abs(m0)))
            within("ragged plan gradient under a constant mean: value vs oracle.grad", dv, 1e-10, (mode, nchunk))
            within("ragged plan gradient under a constant mean: partials vs oracle.grad (of the largest partial)", dg, 1e-10, (mode, nchunk))
            within("ragged plan gradient under a constant mean: d / d mu vs RefSolver", dmu, 1e-10, (mode, nchunk))
            print("mean, %s, chunks %d: value %.2e, partials %.2e, d/dmu %.2e" % (mode, nchunk, dv, dg, dmu))
        # no conditioning record passes and no replay residual but an exact zero either: the evaluation settles such
        # problems by the sequential recurrence and the gradient takes the sequential tangent kernel for them
        plan.set_grad_mode("reverse")
        plan.set_chunks(40)
        plan.set_certificate(max_gamma_over_mu=1e-30, max_residual=1e-30)
        plan.set_coefficients(*coeffs_of(case), jitter=GRAD_JITTER)
        v, g, dm, st = plan.grad_log_likelihood(mean_partial=True)
        if plan.grad_fallbacks() > 0:
            dv, dg = grad_deviation(v, g, v0, g0)
            dmu = float(np.max(np.abs(dm - m0) / np.abs(m0)))
            within("ragged plan gradient, sequential fallback: value vs oracle.grad", dv, 1e-10)
            within("ragged plan gradient, sequential fallback: partials vs oracle.grad (of the largest partial)", dg, 1e-10)
            within("ragged plan gradient, sequential fallback: d / d mu vs RefSolver", dmu, 1e-10)
        print("sequential fallback took %d problems" % plan.grad_fallbacks())
        assert plan.grad_fallbacks() > 0
    finally:
        plan.close()


def test_parameters_to_likelihood_to_gradient_on_a_terms_kernel():
    B, N, lens = 5, 2500, GRAD_LENS
    kernel = terms.RealTerm(1.0, 0.1) + terms.SHOTerm(0.1, 1.0, 1.5)
    rng = np.random.RandomState(8)
    p0 = kernel.get_parameter_vector()
    draws = p0[None, :] + 0.1 * np.clip(rng.randn(B, len(p0)), -3, 3)
    case = dict(t=np.sort(rng.rand(B, N), axis=1), diag=rng.uniform(0.1, 0.2, (B, N)) ** 2)
    case["y"] = np.sin(case["t"]) + 0.3
    mean = rng.uniform(0.0, 0.6, B)
    plan = batch.BatchedGP(B, N, 1, 1)
    try:
        plan.set_series(*garbage_tail(case, lens), lengths=lens)
        plan.set_kernel(kernel)
        got = plan.evaluate_parameters(draws, mean=mean)
        tab = batch.kernel_coefficient_table(kernel, draws, compiled=False)
        keys = ("a_real", "c_real", "a_comp", "b_comp", "c_comp", "d_comp")
        ocase = dict(zip(keys, tab[:6]), t=case["t"], diag=case["diag"], y=case["y"] - mean[:, None])
        dev = deviation(got, oracle(ocase, lens, tab[6]))
        within("ragged plan from kernel parameters: vs oracle", dev, REL)
        value, g, gst = plan.grad_parameters(mean_partial=True)
        v2, cg, dm, st2 = plan.grad_log_likelihood(mean_partial=True)
        jac, jj = plan.kernel_program.jacobian(draws)
        want = batch.chain_gradient(cg, jac, jj, dmean=dm)
        assert (gst == 0).all() and np.array_equal(value, v2) and np.array_equal(g[:, -1], dm)
        P = draws.shape[1]
        terms_abs = np.einsum("bpc,bc->bp", np.abs(jac), np.abs(cg[:, 1:])) + np.abs(jj * cg[:, :1])
        chain = float(np.max(np.abs(g[:, :P] - want[:, :P]) / np.maximum(P * 2.0 ** -52 * terms_abs, 1e-300)))
        within("ragged plan grad_parameters vs chain_gradient(host Jacobian) / (P 2^-52 sum |terms|)", chain, 1.0)
        # ... and the value is the oracle's on the truncated series, with the reference's constant of n_b samples
        from oracle import grad as ograd
        b = 0
        v0, g0 = ograd.grad_log_likelihood(tab[6][b], *[c[b] for c in tab[:6]], EMPTY, EMPTY2, EMPTY2, case["t"][b, :lens[b]],
                                           ocase["y"][b, :lens[b]], case["diag"][b, :lens[b]])
        within("ragged plan grad_parameters: value vs oracle.grad", abs(value[b] - v0) / abs(v0), 1e-10)
        within("ragged plan grad_parameters: coefficient partials vs oracle.grad (of the largest partial)",
               np.max(np.abs(cg[b] - g0)) / np.max(np.abs(g0)), 1e-10)
        print("from parameters: %.2e; chain rule %.3f of its bound" % (dev, chain))
    finally:
        plan.close()


# ---- 4. bit-for-bit invariants ---------------------------------------------------------------------------------------
def _same(a, b, what):
    for x, z in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(z), equal_nan=True), what


@pytest.mark.parametrize("JR,JC", [(2, 3), (0, 2)])
def test_lengths_all_equal_to_N_are_the_uniform_plan(JR, JC):
    B, N = 8, 1000
    case = synthetic(B, N, JR, JC, "accuracy", seed=31)
    out = []
    for lens in (None, np.full(B, N)):
        plan = batch.BatchedGP(B, N, JR, JC)
        try:
            plan.set_series(case["t"], case["diag"], case["y"], lengths=lens)
            plan.set_coefficients(*coeffs_of(case), jitter=0.01)
            assert np.array_equal(plan.lengths, np.full(B, N))
            active = (plan.small_mode_active(), plan.warm_start()["active"])
            res = plan.log_likelihood()
            grad = plan.grad_log_likelihood()
            fact = plan.log_likelihood(materialize=True)
            x = plan.solve()
            out.append((active, res, grad, fact, x))
        finally:
            plan.close()
    assert out[0][0] == out[1][0]
    _same(out[0][1], out[1][1], "evaluation")
    _same(out[0][2], out[1][2], "gradient")
    _same(out[0][3], out[1][3], "materialising run")
    assert np.array_equal(out[0][4], out[1][4])


def test_the_tail_is_never_read():
    N, (nchunk, L, lens) = 1000, SIZES[1000]
    case = synthetic(8, N, 2, 3, "bench", seed=12)
    out = {}
    for kind in ("held", "nan", "descending"):
        for layout in ("staged", "interleaved"):
            plan = ragged_plan(case, lens, nchunk, tail=kind, layout=layout)
            try:
                bounds = plan.selection_bounds()
                out[kind, layout] = (plan.log_likelihood(), plan.grad_log_likelihood(),
                                     tuple(bounds[k] for k in ("tmax", "dxmax", "dmax", "cmax")))
            finally:
                plan.close()
    for layout in ("staged", "interleaved"):
        for kind in ("nan", "descending"):
            _same(out[kind, layout][0], out["held", layout][0], (kind, layout))
            _same(out[kind, layout][1], out["held", layout][1], (kind, layout))
            assert out[kind, layout][2] == out["held", layout][2], (kind, layout)    # tmax, dxmax, dmax, cmax
        assert all(np.isfinite(v) for v in out["held", layout][2])
    # the same garbage without lengths is refused as before: unsorted times raise, NaN times do not pass for sorted
    plan = batch.BatchedGP(8, N, 2, 3)
    try:
        with pytest.raises(ValueError, match="must be sorted"):
            plan.set_series(*garbage_tail(case, lens, "descending"))
        plan.set_series(*garbage_tail(case, lens, "nan"))
        plan.set_coefficients(*coeffs_of(case))
        ll, ld, q, st = plan.log_likelihood()
        short = np.asarray(lens) < N
        assert not np.isfinite(ll[short]).any() or (st[short] != 0).all()
        # ... and a sorted series that is only unsorted inside a problem's own samples is still refused WITH lengths
        t, diag, y = garbage_tail(case, lens, "nan")
        t[3, 10], t[3, 11] = t[3, 11], t[3, 10]
        with pytest.raises(ValueError, match="must be sorted"):
            plan.set_series(t, diag, y, lengths=lens)
        # the rejected series is dropped and its lengths with it: nothing is refused on their account afterwards
        plan.set_summarize_mode(1)
        plan.set_summarize_mode(-1)
        plan.set_series(case["t"], case["diag"], case["y"])
        assert np.array_equal(plan.lengths, np.full(8, N))
    finally:
        plan.close()


@pytest.mark.parametrize("nshards", [2, 3])
def test_sharding_a_ragged_batch_does_not_change_a_single_bit(nshards):
    N, nchunk = 1000, 24
    lens = [1000, 1000, 1000, 1, 2, 47, 48, 49, 96, 999, 1000, 500]   # (the first of 3 or 4 shards holds full lengths only)
    B = len(lens)
    case = synthetic(B, N, 0, 2, "accuracy", seed=77)
    plan = ragged_plan(case, lens, nchunk)
    try:
        want = plan.log_likelihood()
        gwant = plan.grad_log_likelihood()
    finally:
        plan.close()
    within("ragged plan (sharding test): vs oracle", deviation(want, oracle(case, lens)), REL)
    sh = batch.ShardedBatchedGP(B, N, 0, 2, devices=[0] * nshards)
    try:
        sh.set_chunks(nchunk)
        sh.set_series(*garbage_tail(case, lens), lengths=lens)
        assert np.array_equal(sh.lengths, lens)
        sh.set_coefficients(*coeffs_of(case))
        _same(sh.log_likelihood(), want, "sharded evaluation")
        _same(sh.grad_log_likelihood(), gwant, "sharded gradient")
        with pytest.raises(RuntimeError, match=r"unsupported configuration.*lengths"):
            sh.materialize()
        _same(sh.log_likelihood(), want, "sharded evaluation after a refusal")
    finally:
        sh.close()


def test_linear_mean_with_fresh_weights_against_the_mean_subtracted_on_the_host():
    N, (nchunk, L, lens) = 1000, SIZES[1000]
    B, K = 8, 3
    case = synthetic(B, N, 1, 2, "bench", seed=41)
    rng = np.random.RandomState(2)
    t, diag, y = garbage_tail(case, lens)
    Phi = np.stack([np.ones((B, N)), case["t"], np.sin(7.0 * case["t"])], axis=1)       # (B, K, N), finite everywhere
    w = rng.randn(B, K)
    host = dict(case, y=case["y"] - np.einsum("bk,bkn->bn", w, Phi))
    want = oracle(host, lens)
    plan = batch.BatchedGP(B, N, 1, 2)
    try:
        plan.set_chunks(nchunk)
        plan.set_mean_basis(Phi)
        plan.set_series(t, diag, y, lengths=lens)
        got = plan.evaluate(*coeffs_of(case), mean_weights=w)
        dev = deviation(got, want)
        within("ragged plan, linear mean with fresh weights: vs oracle on y - mean over [:n_b]", dev, REL)
        # the same numbers from a plan that is given the residual itself
        direct = ragged_plan(host, lens, nchunk)
        try:
            dev2 = deviation(direct.log_likelihood(), want)
        finally:
            direct.close()
        within("ragged plan, residual formed on the host: vs oracle", dev2, REL)
        print("linear mean on the device %.2e, on the host %.2e" % (dev, dev2))
    finally:
        plan.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def _consumers(plan, xs, Phi_x):
    return {
        "log_likelihood(materialize=True)": lambda: plan.log_likelihood(materialize=True),
        "solve": lambda: plan.solve(),
        "predict": lambda: plan.predict(xs),
        "predict(return_var)": lambda: plan.predict(xs, return_var=True),
        "predict(method=recurrence)": lambda: plan.predict(np.sort(xs), return_var=True, method="recurrence"),
        "forecast": lambda: plan.forecast(np.sort(xs)),
        "one_step_ahead": lambda: plan.one_step_ahead(),
        "predict_terms": lambda: plan.predict_terms(np.sort(xs)),
        "predict_cov": lambda: plan.predict_cov(np.sort(xs)),
        "sample_conditional": lambda: plan.sample_conditional(np.sort(xs), normals=np.zeros((plan.B, len(xs)))),
        "leave_one_out": lambda: plan.leave_one_out(),
        "dot_L": lambda: plan.dot_L(np.ones((plan.B, plan.N))),
        "dot": lambda: plan.dot(np.ones((plan.B, plan.N))),
    }


def test_the_materialised_factor_and_its_consumers_refuse_a_ragged_plan():
    N, (nchunk, L, lens) = 1000, SIZES[1000]
    B = 8
    case = synthetic(B, N, 1, 2, "bench", seed=51)
    want = oracle(case, lens)
    xs = np.linspace(0.1, 0.9, 5)
    plan = batch.BatchedGP(B, N, 1, 2)
    lib = batch._load()
    try:
        plan.set_chunks(nchunk)
        # a factor from BEFORE the lengths must not serve a consumer afterwards
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        plan.log_likelihood(materialize=True)
        uniform_x = plan.solve()
        plan.set_series(*garbage_tail(case, lens), lengths=lens)
        plan.set_coefficients(*coeffs_of(case))
        for name, call in _consumers(plan, xs, None).items():
            with pytest.raises(RuntimeError, match=r"unsupported configuration.*lengths"):
                call()
            dev = deviation(plan.log_likelihood(), want)
            within("ragged plan after a refusal: vs oracle", dev, REL, name)
        # output arrays stay untouched (the C ABI directly)
        x = np.full((B, N), -7.0)
        lib.clr_batch_solve.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        assert lib.clr_batch_solve(plan._h, 1, None, x.ctypes.data_as(_dp)) == CLR_UNSUPPORTED and (x == -7.0).all()
        lib.clr_batch_dot.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        z = np.ones((B, N))
        assert lib.clr_batch_dot(plan._h, 1, z.ctypes.data_as(_dp), x.ctypes.data_as(_dp)) == CLR_UNSUPPORTED and (x == -7.0).all()
        out = [np.full((B, N), -7.0), np.full((B, N), -7.0), np.full(B, -7.0)]
        stat = np.full(B, -7, dtype=np.int32)
        assert lib.clr_batch_leave_one_out(plan._h, *[o.ctypes.data_as(_dp) for o in out], stat.ctypes.data_as(_ip)) == CLR_UNSUPPORTED
        assert all((o == -7.0).all() for o in out) and (stat == -7).all()
        # ... and so for every other refused consumer
        M, G = len(xs), 1
        xp, stat = np.ascontiguousarray(xs).ctypes.data_as(_dp), np.full(B, -7, dtype=np.int32)
        sp = stat.ctypes.data_as(_ip)
        fresh = lambda *shape: np.full(shape, -7.0)
        ptr = lambda a: a.ctypes.data_as(_dp)
        groups = np.ones((G, 3), dtype=np.uint8)              # (one group of the plan's three terms)
        normals = np.zeros((B, M))
        o = [fresh(B, M), fresh(B, M), fresh(B, G, M), fresh(B, G, M), fresh(B, M, M), fresh(B, N), fresh(B, N), fresh(N - 1, 3),
             fresh(N - 1, 3), fresh(N, 3), fresh(N)]
        lib.clr_batch_get_factor.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
        lib.clr_batch_dot_L.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        calls = {
            "predict": lambda: lib.clr_batch_predict(plan._h, M, xp, 0, ptr(o[0])),
            "predict_var": lambda: lib.clr_batch_predict_var(plan._h, M, xp, 0, ptr(o[0])),
            "predict_var_recurrence": lambda: lib.clr_batch_predict_var_recurrence(plan._h, M, xp, 0, ptr(o[0])),
            "forecast": lambda: lib.clr_batch_forecast(plan._h, M, xp, 0, ptr(o[0]), ptr(o[1])),
            "one_step_ahead": lambda: lib.clr_batch_one_step_ahead(plan._h, 1, None, ptr(o[5]), ptr(o[6]), sp),
            "predict_terms": lambda: lib.clr_batch_predict_terms(plan._h, M, xp, 0, G, groups.ctypes.data, ptr(o[2]), ptr(o[3])),
            "predict_cov": lambda: lib.clr_batch_predict_cov(plan._h, M, xp, 0, ptr(o[4])),
            "sample_conditional": lambda: lib.clr_batch_sample_conditional(plan._h, M, xp, 0, 1, ptr(normals), 0.0, 1e-10, ptr(o[0]), sp),
            "dot_L": lambda: lib.clr_batch_dot_L(plan._h, 1, ptr(z), ptr(o[5])),
            "get_factor": lambda: lib.clr_batch_get_factor(plan._h, 0, ptr(o[7]), ptr(o[8]), ptr(o[9]), ptr(o[10])),
        }
        for e in ("clr_batch_predict_var", "clr_batch_predict_var_recurrence"):
            getattr(lib, e).argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, _dp]
        for name, call in calls.items():
            assert call() == CLR_UNSUPPORTED, name
            assert b"lengths" in lib.clr_last_error(), name
            assert all((a == -7.0).all() for a in o) and (stat == -7).all(), name
        # the linear mean's consumers
        plan.set_mean_basis(np.stack([np.ones((B, N)), case["t"]], axis=1))
        plan.set_mean_weights(np.full((B, 2), 0.1))
        for call in (plan.fit_mean_weights, plan.grad_mean_weights):
            with pytest.raises(RuntimeError, match=r"unsupported configuration.*lengths"):
                call()
        w = [fresh(B, 2), fresh(B, 2, 2), fresh(B, 3, 3), fresh(B), fresh(B)]
        assert lib.clr_batch_fit_mean_weights(plan._h, 1e-10, *[ptr(a) for a in w], sp) == CLR_UNSUPPORTED
        assert lib.clr_batch_grad_mean_weights(plan._h, ptr(w[0]), sp) == CLR_UNSUPPORTED
        assert all((a == -7.0).all() for a in w) and (stat == -7).all()
        plan.set_mean_basis(None)
        within("ragged plan after the mean consumers' refusals: vs oracle", deviation(plan.log_likelihood(), want), REL)
        # without lengths the same consumers answer again
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        plan.log_likelihood(materialize=True)
        assert np.array_equal(plan.solve(), uniform_x)
        for name, call in _consumers(plan, xs, None).items():
            call()
    finally:
        plan.close()


def test_bad_lengths_and_shared_arrays_leave_the_plan_unchanged():
    N, (nchunk, L, lens) = 1000, SIZES[1000]
    B = 8
    case = synthetic(B, N, 1, 2, "accuracy", seed=61)
    want = oracle(case, lens)
    plan = ragged_plan(case, lens, nchunk)
    lib = batch._load()
    lib.clr_batch_set_series_ragged.argtypes = [C.c_void_p, _dp, C.c_long, _dp, C.c_long, _dp, C.c_long, _ip]
    try:
        before = plan.log_likelihood()
        t, diag, y = [np.ascontiguousarray(a) for a in garbage_tail(case, lens, "held")]
        for bad in (0, N + 1, -3):
            l2 = np.array(lens, dtype=np.int32)
            l2[5] = bad
            st = lib.clr_batch_set_series_ragged(plan._h, t.ctypes.data_as(_dp), N, diag.ctypes.data_as(_dp), N, y.ctypes.data_as(_dp), N,
                                                 l2.ctypes.data_as(_ip))
            assert st == batch.CLR_INVALID_ARGUMENT and b"outside [1, N" in lib.clr_last_error()
            with pytest.raises(ValueError, match="outside"):        # (the Python front end refuses it before the device)
                plan.set_series(t, diag, y, lengths=l2)
        for shared in range(3):                                       # a shared (N,) array together with lengths
            arrs = [t, diag, y]
            arrs[shared] = np.ascontiguousarray(arrs[shared][7])
            with pytest.raises(RuntimeError, match=r"invalid argument.*\[B\]\[N\]"):
                plan.set_series(*arrs, lengths=lens)
        arrs = [t[7], diag[7], y[7]]                                  # (problem 7 has the full length)
        plan_lengths = plan.lengths
        assert np.array_equal(plan_lengths, lens)
        _same(plan.log_likelihood(), before, "after the refused calls")
        within("ragged plan after refused set_series calls: vs oracle", deviation(plan.log_likelihood(), want), REL)
        # shared arrays with lengths that all equal N are the uniform plan with a shared series
        plan.set_series(*arrs, lengths=np.full(B, N))
        plan.set_coefficients(*coeffs_of(case))
        shared_case = dict(case, t=np.tile(t[7], (B, 1)), diag=np.tile(diag[7], (B, 1)), y=np.tile(y[7], (B, 1)))
        within("uniform lengths with a shared series: vs oracle", deviation(plan.log_likelihood(), oracle(shared_case, [N] * B)), REL)
        # wide plans and plans with general terms refuse lengths
        wide = batch.BatchedGP(4, N, 1, 4)
        try:
            c9 = synthetic(4, N, 1, 4, "bench", seed=1)
            with pytest.raises(RuntimeError, match=r"unsupported configuration.*narrow plans"):
                wide.set_series(c9["t"], c9["diag"], c9["y"], lengths=[5, 1000, 999, 1000])
        finally:
            wide.close()
    finally:
        plan.close()
