# -*- coding: utf-8 -*-
"""`-m gpu`: random walks over a plan's public calls, every state against a fresh plan (tests/_plan_model.py).

A seeded generator draws sequences of ``BatchedGP`` calls -- new series at the same or at other strides, with and without
lengths; constant and linear means; noise bases and weights; amplitude bases (shared, per problem, NaN past the lengths)
and amplitudes (new ones, the ones in force, a zero scale on one problem); coefficient tables and kernel parameters;
chunks, layout, summarize mode, factor layout, rescue, exact; an evaluation left in flight -- and a model says what state
the plan should be in.  After every observation (a plain or a materialising evaluation, ``results()`` with no evaluation
of its own, the gradients with respect to the coefficients, the kernel parameters and the three kinds of weights, the
information matrix in both parametrisations, one of the factor's consumers) the reused plan must give, BIT FOR BIT, what
a plan built directly at the model's state gives; after a materialising run the factors of the first and the last
problem too.  ``results()`` is compared with what a fresh plan at the state of the EVALUATION IN FORCE returns behind the
same call, whatever input setter or ``set_chunks`` came since: that is the call that reaches ``amplitude_snapshot``,
``pin_results`` and ``warm_resolve`` from every setter.  An expected refusal must raise with the message of the code's
own rule and leave the plan as it was: the next observation is compared like any other.  After every settings operation
the route the family is about (the summarize kernel, the one-launch path, the warm start, the chunking) is asserted on
the reused plan and is the fresh plan's.  tests/test_plan_walk_cpu.py shows that the walks visit every pair of kinds
that can be adjacent.

Equal bits on two wrong plans must not pass: at every tenth state, where the generator places an ``evaluate``, and at
the last one, ``loglike / logdet / quad / status`` of the reused plan are held to ``oracle.ref.batch_log_likelihood`` on
``effective(state)`` -- the residual and the variances as NumPy forms them, divided by the host-formed scale where
amplitudes are in force, rows truncated to their lengths, the coefficients formed on the host -- with the amplitude
model's log term folded in as the library states it (``loglike' - L``, ``logdet' + (L + L)``), at the project's 1e-10; a
problem with a zero scale must be NaN with ``CLR_INVALID_ARGUMENT``.  The anchor runs no evaluation of its own between two
operations of a walk.  A narrow family's first compared ``information`` is held to ``_information_ref.dense_information``
(``scaled_dev < 1e-10``) and its first compared ``grad_amplitudes`` to the oracle's c and alpha in
``_amplitude_cases.amplitude_gradient`` (deviation ``/ S_k <= 1e-10``), both on ``effective(state)``.

Families (the smallest shapes at which the route's own check holds; B x N, width):
  narrow          5 x 601, width 4, 7 | 4 chunks of 88 | 152 samples with a ragged last one; staged and interleaved; lengths
                  set and cleared around a factor (consumers refused under them, the factor gone when they go)
  role split 8/7  3 x 720 | 717, widths 8 | 7, 5 | 3 chunks, t squeezed by 0.03 (dense for the lazy kernels); modes 1, 2, 0
  warm            5 x 1536, width 6, forced (1, 128): 3 | 6 warm chunks; one term that does not forget; never materialises
  one launch      5 x 1000, width 4, set_small_mode(1), one near-singular problem left pending; never materialises
  lengths         5 x 1000, width 8, summarize automatic, lengths below and above 512 and one equal to N; set and cleared
  wide            3 x 600, width 21, 5 | 3 chunks; refuses lengths and the information matrix
  wide 64 one chunk  3 x 120, width 35, ONE chunk: the plan gradient is the sequential tangent kernel on the series in force
                  and runs no evaluation -- ``results()`` behind it is still the earlier evaluation, bit for bit (the model
                  records the route as "no evaluation": ``_plan_model.gradient_evaluates``); never materialises
  sharded         the narrow family on ShardedBatchedGP(devices=[0, 0]) against a fresh UNSHARDED plan
Every problem is held at 1e-10 but the one-launch family's near-singular one, for which no truth at 1e-10 exists in double
precision: the double oracle is itself up to 3.3e-10 from its binary128 twin on it (tests/test_plan_walk_cpu.py).
tests/test_gpu_batch.py::test_short_narrow_problems_in_one_launch takes the same problem out of its comparison with the
oracle; here it keeps the oracle's status, the fresh plan's bits at every observation, and a bound of 1e-9 -- three times
the oracle's own error -- that only a gross error would cross.

Two defects the walks' literal sequences were written for, each seen failing on the library before its fix:
  ``information_parameters()`` behind ``set_coefficients`` chained the tables' information matrix through the Jacobian at
      the stale parameter rows where ``grad_parameters()`` refuses ("no refusal": ``narrow``, literal 7, step 4; in the walks
      first at ``lengths``, seed 14, step 15).  Both plan classes now drop the rows wherever coefficients are replaced.
  ``wide_batch_grad``'s one-chunk branch set ``amp_eval`` without an evaluation: ``results()`` behind evaluate (a1),
      ``set_amplitudes(a2)``, ``grad_log_likelihood()`` returned loglike (-130.98, -191.22, -160.70) for the a1 evaluation's
      (-168.53, -106.30, -122.52) -- its loglike' under a2's log term -- and (-129.34, -139.93, -134.15), loglike' with no log
      term, with the basis removed in between (``wide 64 one chunk``, literals 0 and 1, step 5).

That the walks can fail: the library built with one line of a cause function removed, this file run once per build.
  ``h->scan_series.d_stale = true`` (variance_replaced): 48 of the 158 tests fail, in every family that reads the scan's
      copy, each at the first compared observation behind a change of the variances -- ``narrow``, seed 0, step 49 (evaluate
      behind noise_basis_none), ``lengths``, seed 3, step 29, ``one launch``, seed 5, step 74 (the scan behind the one-launch
      kernel), ``role split 7``, seed 0, step 26 and ``role split 8``, seed 1, step 7 (materialize behind noise_weights).
  ``h->pv_S_valid = h->loo_Q_valid = false`` (factor_written): 16 walks fail at a consumer behind a SECOND materialising
      run -- ``narrow``, seed 1, step 54 (forecast), ``role split 8``, seed 0, step 8 (predict_cov), ``role split 7``,
      seed 0, step 75 (predict_cov).
  ``h->scan_series.stale = true`` under the stride test (residual_replaced): survives, and changes no result as the code
      stands.  The line is reached (244 mean calls of the walks change the residual's stride while the scan reads its
      copy), but ``y_stale`` alone already transposes the whole of Y again, at the stride in force and into a buffer
      that ``batch_params`` has re-sized (SeriesJobs::reserve), and T and D hold nothing of y.
  the ``launch_pad_tail`` line of apply_noise: survives, and changes no result as the code stands.  The line is reached
      (``noise_basis_nan_tails``: a basis that is NaN past the lengths, so that the variances' tail is NaN without it), but
      every kernel of a plan with lengths counts the samples below ``len[b]`` alone (clr_batch_kernels.h: series_len) and
      no public call returns anything from behind them.  A route that counted tail samples would reach it; none does.
(These four were measured on the 158 tests before the amplitude model and the information matrix joined the walks.)  With
them in, three more lines, each changing values only:
  the ``amplitude_divide`` call at the end of apply_mean: 136 of the 375 tests fail, in every family (narrow 24, role split
      8 | 7 23 | 17, sharded 17, wide 14, lengths 13, wide 64 one chunk 11, one launch 9, warm 8), first at ``lengths``, seed 12
      (evaluate behind mean_weights with amplitudes in force: the residual is read undivided).
  ``variance_replaced(h, N)`` in amplitude_divide: 83 tests fail, in every family (narrow 15, role split 8 | 7 14 | 11, sharded
      9, wide 9, lengths 8, wide 64 one chunk 7, one launch 5, warm 5), first at ``lengths``, seed 1; ``lengths``, seed 5, step 59
      is an evaluate behind series_y_stride, amplitude_basis_per, amplitudes.
  the ``amplitude_snapshot`` call in apply_amplitudes: ONE test fails -- ``wide 64 one chunk``, seed 17: results() behind an
      evaluation left in flight, then amplitudes_zero and a new basis, returns the evaluation's loglike' under the later log
      term (NaN for the zeroed problem).  Nearly a survivor, and for a reason: ``amplitude_adjust`` takes the same snapshot
      the first time an evaluation's results are read, and evaluate, the gradients and the information matrix all read
      them at once, so the call in apply_amplitudes alone protects only an ``enqueue()`` whose results are first read
      behind new amplitudes.  The walks reach that order once; a literal sequence for it would be the next addition.

Measured on an MI355X: 375 tests (361 walks of 80 calls, 14 literal sequences; 29076 calls, 8984 compared observations,
2913 anchored states) in 81.0 s with the walks' generation -- the file before the amplitude model and the information
matrix joined it: 158 tests in 33.4 s -- the slowest 1.8 s (the first of a family, which draws the walks and anchors the
information matrix), the others below 0.7 s.  Without a GPU tests/test_plan_walk_cpu.py takes 17.8 s (13.4 s before, with 151
walks).  Largest deviations from the oracle, every bar 1e-10 (loglike / logdet / quad): narrow 2.4e-12 / 1.9e-14 / 7.3e-14,
role split 5.0e-12 / 4.9e-14 / 2.5e-13, warm 2.0e-15 / 4.1e-15 / 3.8e-15, lengths 3.5e-12 / 1.6e-14 / 6.1e-14, wide 7.0e-14 /
1.8e-13 / 6.5e-14, wide 64 one chunk 1.9e-14 / 9.5e-13 / 3.2e-13, sharded 1.1e-12 / 8.5e-15 / 3.5e-14, one launch 1.4e-11 /
1.0e-14 / 1.1e-13 without the near-singular problem and 4.3e-10 / 2.4e-13 / 3.8e-10 on it (bound 1e-9).  The information
matrix is at most 1.5e-12 from the dense reference (role split 8; warm 1.4e-12, lengths 5.9e-13, the others below 1.1e-13),
``grad_amplitudes`` at most 3.8e-15 of ``S_k`` from the oracle's.
"""
import functools
import re

import numpy as np
import pytest

from celerite_amd import batch, terms
from oracle import ref
from _cases import within
from _noise_cases import oracle_c_alpha
from _amplitude_cases import amplitude_gradient, host_scale
import _information_ref as iref
import _plan_model as pm

pytestmark = pytest.mark.gpu

REL = 1e-10     # the project's bar on loglike, logdet and quad against the oracle
REL_NEAR_SINGULAR = 1e-9   # three times the double oracle's own distance from binary128 on that problem (3.3e-10)
COMPARED = {"states": 0}
ANCHORED = set()           # (family, kind): the new observations are held to their references once per family


pm.kernel_factory = lambda JR, JC: pm.make_kernel(terms, JR, JC)


def _classes(fam):
    """``(the reused plan's class, the fresh plan's)``."""
    if pm.FAMILIES[fam]["sharded"]:
        return functools.partial(batch.ShardedBatchedGP, devices=[0, 0]), batch.BatchedGP
    return batch.BatchedGP, batch.BatchedGP


def _route(plan):
    rep = {"kernel": plan.summarize_kernel()}
    if hasattr(plan, "small_mode_active"):
        rep.update(small=plan.small_mode_active(), warm=plan.warm_start()["active"], chunks=plan.chunks)
    return rep


def _assert_route(state, plan, other, ctx):
    """The family's route on the reused plan, and the same report from the fresh plan."""
    a, b = _route(plan), _route(other)
    assert all(a[k] == b[k] for k in a if k in b), (a, b, ctx())
    c = state.cfg
    if "small" in a:
        assert a["warm"] == (1 if state.warm[0] == 1 else 0), (a, ctx())
        assert a["small"] == (state.small == 1 and not state.exact), (a, ctx())
        assert (a["chunks"][0] > 1) == (state.chunks > 1), (a, ctx())
    if c["JR"] + 2 * c["JC"] in (7, 8) and state.summarize > 0:
        assert a["kernel"].startswith("role split"), (a, ctx())
    if state.summarize == 0:
        assert a["kernel"] == "single wave", (a, ctx())


def _same(got, want, ctx):
    got, want = pm.flatten(got), pm.flatten(want)
    assert len(got) == len(want) and len(got) > 0, ctx()
    for i, (x, z) in enumerate(zip(got, want)):
        assert x.shape == z.shape and np.array_equal(x, z, equal_nan=(x.dtype.kind == "f")), ("array %d of the result" % i, x, z, ctx())


def _anchor(state, got, ctx):
    """``got``, an evaluation of the reused plan in ``state``, against the oracle on ``effective(state)`` and on
    coefficients formed on the host (kernel parameters: by the ``terms`` kernel, not by the plan's program)."""
    ll, ld, q, st = got
    tabs = pm.host_coefficients(state)
    t, d, r, lens, L = pm.effective(state)
    B = state.cfg["B"]
    # a problem with a zero scale: NaN and CLR_INVALID_ARGUMENT, whatever its series (the oracle is given the plain ones)
    zero = _zero_scale(state)
    if zero.any():
        plain = state.copy()
        plain.gam = plain.amp = None
        _, d0, r0, _, _ = pm.effective(plain)
        d = [d0[b] if zero[b] else d[b] for b in range(B)]
        r = [r0[b] if zero[b] else r[b] for b in range(B)]
        L = np.where(zero, 0.0, L)
    jit = np.broadcast_to(np.asarray(tabs[6], dtype=np.float64), (B,))

    def oracle(dd):
        if len(set(lens)) == 1:
            return ref.batch_log_likelihood(jit, *tabs[:6], np.stack(t), np.stack(dd), np.stack(r))
        rows = [ref.batch_log_likelihood(jit[b], *[x[b:b + 1] for x in tabs[:6]], t[b], dd[b], r[b]) for b in range(B)]
        return [np.concatenate([np.atleast_1d(row[i]) for row in rows]) for i in range(4)]

    want = [np.array(x, copy=True) for x in oracle(d)]
    # the amplitude model's log term, as the library states it: loglike = loglike' - L, logdet = logdet' + (L + L), quad = quad'
    want[0], want[1] = want[0] - L, want[1] + (L + L)
    want[3][zero] = batch.CLR_INVALID_ARGUMENT
    assert np.array_equal(st, np.asarray(want[3])), (st, want[3], ctx())
    assert all(np.isnan(x[zero]).all() for x in (ll, ld, q)), (ll, ld, q, ctx())
    ok = np.asarray(st) == 0
    assert ok.sum() >= B - 1, (st, ctx())
    # The one-launch family's near-singular problem (variances of 1e-14) is outside the project's 1e-10 as
    # tests/test_gpu_batch.py applies it to this very shape (test_short_narrow_problems_in_one_launch: ``ok = (s0 == 0) &
    # (np.arange(B) != 3)``): the double oracle is itself up to 3.3e-10 from its binary128 twin there
    # (tests/test_plan_walk_cpu.py shows it), so no truth at 1e-10 exists for it.  It keeps the oracle's status, the fresh
    # plan's bits at every observation, and three times the oracle's own error, 1e-9, against the oracle.
    ill = np.zeros(B, dtype=bool)
    if state.cfg["ill"] is not None:
        ill[state.cfg["ill"]] = True
    for name, x, x0 in zip(("loglike", "logdet", "quad"), (ll, ld, q), want):
        dev = np.abs(x - np.asarray(x0)) / np.abs(np.asarray(x0))
        within("plan walks (%s): %s of the reused plan vs oracle.ref.batch_log_likelihood on effective(state)" % (state.fam, name),
               np.max(dev[ok & ~ill]), REL, (list(dev), ctx()))
        if (ok & ill).any():
            within("plan walks (%s): %s of the near-singular problem vs oracle.ref.batch_log_likelihood" % (state.fam, name),
                   np.max(dev[ok & ill]), REL_NEAR_SINGULAR, (list(dev), ctx()))


def _zero_scale(state):
    zero = np.zeros(state.cfg["B"], dtype=bool)
    if state.amp is not None and state.amp_zero:
        zero[pm.ZERO_PROBLEM] = True
    return zero


def _jitter(state, tabs):
    return np.broadcast_to(np.asarray(tabs[6], dtype=np.float64), (state.cfg["B"],))


def _anchor_information(state, op, got, ctx):
    """``information`` of the reused plan against tests/_information_ref.py's dense reference on ``effective(state)``, at
    tests/test_gpu_batch_information.py's bar and scale.  O(N^3) per direction: the first and the last problem that
    are ``CLR_OK`` (rows truncated to their lengths), above 800 samples the shortest one alone -- up to 2.6 s at N = 1536."""
    info, st = got
    tabs = pm.host_coefficients(state)
    jit = _jitter(state, tabs)
    t, d, r, lens, _ = pm.effective(state)
    mean = op.k % 2 == 1
    good = [b for b in range(state.cfg["B"]) if st[b] == 0]
    assert good and not _zero_scale(state)[good].any(), (st, ctx())
    which = sorted(set([good[0], good[-1]])) if state.cfg["N"] <= 800 else [min(good, key=lambda b: lens[b])]
    for b in which:
        want = iref.dense_information(t[b], d[b], r[b], *[x[b] for x in tabs[:6]], jit[b], mean=mean)
        if not jit[b] > 2.220446049250313e-16:       # (the jitter's row and column are zeroed: BatchedGP.information)
            assert not info[b][0, :].any() and not info[b][:, 0].any(), ctx()
            dev = iref.scaled_dev(info[b][1:, 1:], want[1:, 1:])
        else:
            dev = iref.scaled_dev(info[b], want)
        within("plan walks (%s): information of the reused plan vs _information_ref.dense_information on effective(state)" % state.fam,
               dev, REL, (b, ctx()))


def _anchor_grad_amplitudes(state, got, ctx):
    """``grad_amplitudes`` of the reused plan against ``_amplitude_cases.oracle_gradient``'s statement -- the oracle's c and
    alpha (``RefSolver``) on the host-formed series, the same sums and the same scale ``S_k`` -- with the state's jitter on
    the oracle's diagonal (``oracle_gradient`` itself is the case of no jitter: d' enters the formula without it)."""
    da, st = got
    tabs = pm.host_coefficients(state)
    jit = _jitter(state, tabs)
    t, dp, yp, lens, _ = pm.effective(state)
    case = dict(zip(("a_real", "c_real", "a_comp", "b_comp", "c_comp", "d_comp"), tabs[:6]), t=np.stack(t))
    s = host_scale(pm.amplitudes_of(state), pm.gamma_of(state))
    G = np.broadcast_to(pm.gamma_of(state), (state.cfg["B"], pm.AMP_K, state.cfg["N"]))
    zero = _zero_scale(state)
    for b in range(state.cfg["B"]):
        if zero[b] or st[b] != 0:
            assert not da[b].any(), (da[b], ctx())
            continue
        c, al = oracle_c_alpha(case, b, dp[b] + jit[b], yp[b])
        g, S = amplitude_gradient(G[b], al, c, yp[b], dp[b], s[b])
        within("plan walks (%s): grad_amplitudes of the reused plan vs the oracle's c and alpha on effective(state), / S_k" % state.fam,
               np.max(np.abs(da[b] - g) / S), REL, (b, list(da[b]), list(g), ctx()))


def run(fam, seed, ops):
    """The operations on one reused plan; every compared observation against a fresh plan that is built for it and closed."""
    reused_cls, fresh_cls = _classes(fam)
    state = pm.initial(fam, seed)
    plan = pm.fresh(state, reused_cls)
    due = False
    try:
        for i, op in enumerate(ops):
            ctx = lambda: "family %r, seed %d, step %d (%s): replay(%r, %d, %s)" % (fam, seed, i, op.expected, fam, seed, pm.printable(ops[:i + 1]))
            got = None
            if op.expected == "ok":
                try:
                    got = op.call(plan)
                except Exception as e:
                    raise AssertionError("%s raised %r" % (ctx(), e))
            elif op.expected == "undefined":
                try:
                    op.call(plan)
                except (RuntimeError, ValueError):
                    pass
            else:
                with pytest.raises((RuntimeError, ValueError), match=re.escape(op.expected.split(":", 1)[1])):
                    op.call(plan)
                    raise AssertionError("no refusal: " + ctx())
            state = op.apply_to
            if op.expected == "ok" and op.kind == "results":
                made = []
                try:
                    # what a fresh plan at the state of the evaluation in force returns behind the same call, bit for bit
                    _same(got, op.reference(lambda at: made.append(pm.fresh(at, fresh_cls)) or made[-1]), ctx)
                    COMPARED["states"] += 1
                finally:
                    for other in made:
                        other.close()
            elif op.expected == "ok" and (op.observes or op.settings):
                other = pm.fresh(op.before if op.observes else state, fresh_cls)
                try:
                    if op.observes:
                        if op.observes in ("consumer",) or op.kind in ("grad_mean_weights", "grad_noise_weights", "grad_amplitudes"):
                            other.log_likelihood(True)
                        _same(got, op.call(other), ctx)
                        if op.observes == "mat" and hasattr(plan, "factor"):
                            for p in (0, plan.B - 1):
                                _same(plan.factor(p), other.factor(p), ctx)
                        COMPARED["states"] += 1
                    _assert_route(state, plan, other, ctx)
                finally:
                    other.close()
                # equal bits on two wrong plans must not pass: a narrow family's first compared observation of each new kind
                # (walk 0's, where it has one) against the existing references
                if op.kind in ("information", "grad_amplitudes") and (fam, op.kind) not in ANCHORED \
                        and state.cfg["JR"] + 2 * state.cfg["JC"] <= 8:
                    ANCHORED.add((fam, op.kind))
                    if op.kind == "information":
                        _anchor_information(op.before, op, got, ctx)
                    else:
                        _anchor_grad_amplitudes(op.before, got, ctx)
            # the anchor runs nothing of its own between two operations: every tenth call of a generated walk IS an
            # ``evaluate`` (tests/_plan_model.py), whose result it takes; in a literal sequence the first compared
            # ``evaluate`` at or behind every tenth step; behind the last step, where nothing follows, an evaluation of its own
            due, anchored = due or i % 10 == 9, False
            if (due or i == len(ops) - 1) and op.kind == "evaluate" and op.expected == "ok":
                _anchor(state, got, ctx)
                due, anchored = False, True
        if not anchored:
            _anchor(state, plan.log_likelihood(), ctx)
    finally:
        plan.close()


CASES = [(fam, seed) for fam in sorted(pm.FAMILIES) for seed in range(pm.SEEDS[fam])]


@pytest.mark.parametrize("fam,seed", CASES, ids=["%s-%d" % c for c in CASES])
def test_walk(fam, seed):
    run(fam, seed, pm.walk(fam, seed, pm.STEPS))


LITERALS = [(fam, i) for fam in sorted(pm.LITERAL) for i in range(len(pm.LITERAL[fam]))]


@pytest.mark.parametrize("fam,i", LITERALS, ids=["%s-%d" % c for c in LITERALS])
def test_literal_sequence(fam, i):
    seed, seq = pm.LITERAL[fam][i]
    run(fam, seed, pm.replay(fam, seed, seq))
