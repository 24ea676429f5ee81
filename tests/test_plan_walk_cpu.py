# -*- coding: utf-8 -*-
"""The generator and the model of tests/_plan_model.py, without a GPU: that the walks test_gpu_plan_walk.py runs are
deterministic, visit every pair of operation kinds that can be adjacent, put every kind in front of every class of
observation, keep the expected refusals rare and end in a compared observation -- the conditions that stop the walks from
quietly never visiting a composition -- and that ``effective()`` is the NumPy statement of the residual and variances."""
import numpy as np
import pytest

import _plan_model as pm
from _noise_cases import host_diag

FAMILIES = sorted(pm.FAMILIES)


def _walks(fam):
    return [pm.walk(fam, seed, pm.STEPS) for seed in range(pm.SEEDS[fam])] + [pm.replay(fam, seed, seq) for seed, seq in pm.LITERAL.get(fam, [])]


def _ok_kinds(state):
    """The kinds whose call in ``state`` is legal and compared."""
    return [cls.kind for cls in pm.OPS if cls(0).legal(state) and cls(0).expect(state) == "ok"]


@pytest.mark.parametrize("fam", FAMILIES)
def test_a_walk_is_a_function_of_family_seed_and_steps(fam):
    for seed in (0, 3):         # (without the cache a walk is drawn again behind the walks of the seeds below it)
        a = pm.printable(pm.walk(fam, seed, pm.STEPS))
        b = pm.printable(pm.walk(fam, seed, pm.STEPS, cache=False))
        assert a == b and len(pm.walk(fam, seed, pm.STEPS)) == pm.STEPS
    # ... and a walk written out literally is the same operations with the same expectations
    ops = pm.walk(fam, 1, pm.STEPS)
    again = pm.replay(fam, 1, [(op.kind, op.k) for op in ops])
    assert pm.printable(again) == pm.printable(ops) and [op.expected for op in again] == [op.expected for op in ops]


@pytest.mark.parametrize("fam", FAMILIES)
def test_every_adjacent_pair_of_kinds_is_visited(fam):
    """Over the seeds the family uses on the GPU: every ordered pair (kind_i, kind_j) that can legally be adjacent in the
    family, both calls compared -- ``reachable_pairs``: a breadth-first search over the model's abstract state, not over
    what the walks happened to reach -- occurs at least once.  Nothing runs between two operations on the GPU either: the
    oracle anchor uses the result of an ``evaluate`` operation of the walk."""
    visited, met = set(), set()
    for ops in _walks(fam):
        prev = None
        for op in ops:
            if op.expected == "ok":
                if prev is not None:
                    visited.add((prev, op.kind))
                met.update((op.kind, kind) for kind in _ok_kinds(op.apply_to))
                prev = op.kind
            else:
                prev = None
    possible = pm.reachable_pairs(fam)
    assert len(possible) > 400 and not met - possible, (len(possible), sorted(met - possible))
    assert not possible - visited, sorted(possible - visited)


@pytest.mark.parametrize("fam", FAMILIES)
def test_every_kind_comes_directly_before_every_class_of_observation(fam):
    """... compared observations: a plain evaluation (``results`` among them), a materialising one, a gradient, an
    information matrix, a consumer -- wherever the family has the class at all and the kind leaves it legal (a consumer is never legal directly behind ``set_chunks``)."""
    before, could, refused_then_observed, refused = set(), set(), set(), set()
    for ops in _walks(fam):
        for op, nxt in zip(ops[:-1], ops[1:]):
            if op.expected != "ok":
                refused.add(pm.label(op))
                if nxt.observes and nxt.expected == "ok":
                    refused_then_observed.add(pm.label(op))
                continue
            for kind in _ok_kinds(op.apply_to):
                if pm.KINDS[kind].observes:
                    could.add((op.kind, pm.KINDS[kind].observes))
            if nxt.observes and nxt.expected == "ok":
                before.add((op.kind, nxt.observes))
    assert not could - before, sorted(could - before)
    kinds = set(k for k, _ in could)
    assert all((k, "eval") in before for k in kinds)
    # the plan is as it was after a refusal: every refused or undefined kind is followed by a compared observation somewhere
    assert not refused - refused_then_observed, sorted(refused - refused_then_observed)


@pytest.mark.parametrize("fam", FAMILIES)
def test_refusals_stay_rare_and_every_walk_ends_in_a_compared_observation(fam):
    seen = set()
    for ops in _walks(fam):
        quiet = sum(op.expected != "ok" for op in ops)
        assert 4 * quiet <= len(ops), (quiet, len(ops))
        assert ops[-1].observes and ops[-1].expected == "ok"
        seen.update(pm.label(op) for op in ops)
    # the refusals the code's own rules give do occur
    want = {"narrow": ["consumer!", "grad_noise_weights!", "grad_mean_weights!", "grad_amplitudes!", "mean_const!", "mean_per!",
                       "amplitude_basis_shared!", "amplitude_basis_per!", "information!", "grad_parameters!",
                       "information_parameters!"],
            "lengths": ["materialize!", "consumer!", "set_summarize_mode!", "grad_amplitudes!", "amplitude_basis_nan_tails!"],
            "wide": ["series_lengths!", "information!", "grad_parameters!", "information_parameters!", "grad_amplitudes!"],
            "warm": ["series_lengths!", "information!", "grad_parameters!", "information_parameters!"],
            "one launch": ["series_lengths!", "mean_const!"], "role split 8": ["series_lengths!", "grad_amplitudes!"],
            "sharded": ["information_parameters!", "grad_parameters!"],
            "wide 64 one chunk": ["series_lengths!", "information!", "information_parameters!", "grad_parameters!"]}
    for lab in want.get(fam, []):
        assert lab in seen, (fam, lab)


class _Recorder(object):
    """Stands in for a plan: takes every call and keeps its name."""
    B = 0

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def method(*args, **kwargs):
            self.calls.append(name)
        return method


@pytest.mark.parametrize("fam", FAMILIES)
def test_every_call_of_every_walk_forms_its_arguments(fam):
    """... also a call the model expects to be refused, whose state behind it holds nothing of what the call passes."""
    from celerite_amd import terms
    saved = pm.kernel_factory
    pm.kernel_factory = lambda JR, JC: pm.make_kernel(terms, JR, JC)
    try:
        for ops in _walks(fam):
            plan = _Recorder()
            for op in ops:
                n = len(plan.calls)
                op.call(plan)
                assert len(plan.calls) > n, op
                if op.kind == "results":
                    made = []
                    op.reference(lambda at: made.append(pm.fresh(at, lambda *shape: _Recorder())) or made[-1])
                    assert made[0].calls[-1] == "results" and made[0].calls.count("results") == 1
    finally:
        pm.kernel_factory = saved


def test_the_compositions_the_walks_are_for_occur():
    """The sequences the suite did not compose before, each found in some walk of the family named."""
    def some(fam, pred):
        for ops in _walks(fam):
            for i, op in enumerate(ops):
                if pred(ops, i, op):
                    return True
        return False

    # a noise basis removed while lengths are in force
    assert some("lengths", lambda ops, i, op: op.kind == "noise_basis_none" and op.before.ragged)
    # set_series under a mean basis AND a noise basis, the caller's stride changing
    assert some("narrow", lambda ops, i, op: op.kind in ("series_y_stride", "series_d_stride") and op.before.phi is not None
                and op.before.psi is not None)
    # the residual and the variances both pending, then a stride change, with no evaluation in between
    assert some("narrow", lambda ops, i, op: i >= 2 and op.kind in ("series_y_stride", "series_d_stride")
                and {ops[i - 1].kind, ops[i - 2].kind} == {"mean_weights", "noise_weights"})
    # a weight change while the scan does not read its copy, then the layout or the summarize mode makes it read one
    assert some("narrow", lambda ops, i, op: i >= 4 and op.kind == "set_layout" and op.before.layout == "staged"
                and op.apply_to.layout == "interleaved" and all(o.kind == "evaluate" for o in ops[i - 2:i])
                and {ops[i - 3].kind, ops[i - 4].kind} == {"noise_weights", "mean_weights"})
    assert some("role split 8", lambda ops, i, op: i >= 2 and op.kind == "set_summarize_mode" and op.before.summarize == 0
                and op.apply_to.summarize > 0 and ops[i - 1].kind == "evaluate" and ops[i - 2].kind in ("noise_weights", "mean_weights"))
    # set_chunks between a weight change and the next evaluation
    assert some("narrow", lambda ops, i, op: i >= 1 and op.kind == "set_chunks" and ops[i - 1].kind == "noise_weights")
    # a lean factor after a variance change (refused), materialised again, then a consumer
    assert some("narrow", lambda ops, i, op: op.kind == "consumer" and op.expected == "refuses:materialise again")
    assert some("narrow", lambda ops, i, op: i >= 1 and op.kind == "consumer" and op.expected == "ok" and op.before.f_lean
                and ops[i - 1].kind == "materialize")
    # lengths set and cleared
    assert some("lengths", lambda ops, i, op: op.kind == "series_no_lengths")
    # ... around a factor: a factor in HBM when the lengths come, consumers refused under them, the factor gone when they
    # are cleared, and a compared consumer behind the next materialising run
    assert some("narrow", lambda ops, i, op: op.kind == "series_lengths" and op.expected == "ok" and op.before.factor_state() == "ok")
    assert some("narrow", lambda ops, i, op: i >= 1 and op.kind == "consumer" and op.expected == "refuses:per-problem lengths"
                and ops[i - 1].kind == "series_lengths")
    assert some("narrow", lambda ops, i, op: i >= 1 and op.kind == "consumer" and op.expected == "refuses:no materialising run"
                and ops[i - 1].kind == "series_no_lengths")
    assert some("narrow", lambda ops, i, op: i >= 3 and op.kind == "consumer" and op.expected == "ok"
                and [o.kind for o in ops[i - 3:i]] == ["consumer", "evaluate", "materialize"] and ops[i - 3].expected != "ok")
    # kernel parameters alternating with coefficient tables
    assert some("narrow", lambda ops, i, op: i >= 1 and op.kind == "coef_draw" and ops[i - 1].kind == "kernel_params")
    assert some("narrow", lambda ops, i, op: i >= 1 and op.kind == "kernel_params" and ops[i - 1].kind == "coef_draw")
    # every setter with an evaluation in flight
    for kind in ("series_new", "mean_const", "mean_basis", "mean_weights", "noise_basis_per", "noise_weights", "coef_draw",
                 "kernel_params", "set_chunks", "set_layout", "set_rescue", "amplitude_basis_shared", "amplitude_basis_per",
                 "amplitude_basis_none", "amplitudes", "amplitudes_same", "amplitudes_zero"):
        assert some("narrow", lambda ops, i, op: i >= 1 and op.kind == kind and ops[i - 1].kind == "enqueue"), kind
    # ---- the amplitude model: "the first transform to arrive moves the caller's array aside, the last to leave moves it back"
    bases = ("amplitude_basis_shared", "amplitude_basis_per", "amplitude_basis_nan_tails", "amplitude_basis_none")
    ok = lambda op: op.expected == "ok"
    for mean in (False, True):
        for noise in (False, True):
            under = lambda s: (s.phi is not None) == mean and (s.psi is not None) == noise
            # amplitudes arriving and leaving under each combination of a mean basis and a noise basis ...
            assert some("narrow", lambda ops, i, op: op.kind == "amplitudes" and op.before.amp is None and under(op.before)), (mean, noise)
            assert some("narrow", lambda ops, i, op: op.kind in bases and ok(op) and op.before.amp is not None and under(op.before)), (mean, noise)
    # ... and in the other order: the mean basis, the noise basis arriving while amplitudes are in force, and removed while they stay
    for kind in ("mean_basis", "noise_basis_shared", "noise_basis_per", "mean_basis_none", "noise_basis_none"):
        assert some("narrow", lambda ops, i, op: op.kind == kind and ok(op) and op.before.amp is not None
                    and (not kind.endswith("none") or op.apply_to.amp is not None)), kind
    # results() directly behind a setter, the evaluation in force one with amplitudes (amplitude_snapshot, pin_results)
    for kind in ("amplitudes", "amplitude_basis_none", "series_new", "noise_weights"):
        assert some("narrow", lambda ops, i, op: i >= 1 and op.kind == "results" and ops[i - 1].kind == kind and ok(ops[i - 1])
                    and op.before.evaluated[2].amp is not None), kind
    # new amplitudes directly behind a zero scale (the per-problem flags clear again), then a compared evaluation
    assert some("narrow", lambda ops, i, op: 1 <= i < len(ops) - 1 and op.kind == "amplitudes" and ops[i - 1].kind == "amplitudes_zero"
                and ops[i + 1].observes == "eval" and ok(ops[i + 1]))
    # a stride change of y and of diag, lengths set and cleared, with amplitudes in force
    for kind in ("series_y_stride", "series_d_stride", "series_lengths", "series_no_lengths"):
        assert some("narrow", lambda ops, i, op: op.kind == kind and ok(op) and op.before.amp is not None), kind
    assert some("lengths", lambda ops, i, op: op.kind == "series_no_lengths" and op.before.amp is not None)
    # fit_mean_weights refused under amplitudes, whatever the factor's state
    assert some("narrow", lambda ops, i, op: op.kind == "consumer" and op.expected == "refuses:amplitudes are in force")
    # the parameter calls behind tables that replaced what the parameters formed (refused), and behind new parameters
    for kind in ("grad_parameters", "information_parameters"):
        assert some("narrow", lambda ops, i, op: op.kind == kind and op.expected == pm.NOT_FROM_PARAMETERS)
        assert some("narrow", lambda ops, i, op: op.kind == kind and ok(op))
    # the one-chunk plan of width 35: results() behind a gradient that runs no evaluation, new amplitudes or none in between
    for kind in ("amplitudes", "amplitude_basis_none"):
        assert some("wide 64 one chunk", lambda ops, i, op: i >= 2 and op.kind == "results" and ops[i - 1].kind == "grad_log_likelihood"
                    and ops[i - 2].kind == kind and op.before.evaluated[2].amp is not None), kind


def test_the_model_follows_the_code_s_rules_for_the_factor():
    """require_factor, refuse_ragged, variance_changed and factor_dropped, on literal sequences."""
    def last(fam, seq):
        return pm.replay(fam, 0, seq)[-1].expected

    assert last("narrow", [("consumer", 0)]) == "refuses:no materialising run"
    assert last("narrow", [("materialize", 0), ("consumer", 0)]) == "ok"
    assert last("narrow", [("materialize", 0), ("mean_basis", 0), ("mean_weights", 1), ("consumer", 0)]) == "ok"
    assert last("narrow", [("materialize", 0), ("coef_draw", 1), ("consumer", 0)]) == "undefined"
    assert last("narrow", [("set_factor_layout", 1), ("materialize", 0), ("coef_draw", 1), ("consumer", 0)]) == "refuses:materialise again"
    assert last("narrow", [("materialize", 0), ("set_chunks", 0), ("consumer", 0)]) == "refuses:no materialising run"
    assert last("narrow", [("materialize", 0), ("set_factor_layout", 1), ("consumer", 0)]) == "refuses:no materialising run"
    assert last("narrow", [("noise_basis_per", 0), ("materialize", 0), ("grad_noise_weights", 0)]) == "ok"
    assert last("narrow", [("noise_basis_per", 0), ("materialize", 0), ("noise_weights", 1), ("grad_noise_weights", 0)]) == "refuses:materialise again"
    assert last("narrow", [("noise_basis_per", 0), ("materialize", 0), ("noise_weights_same", 1), ("grad_noise_weights", 0)]) == "ok"
    assert last("lengths", [("series_lengths", 0), ("materialize", 0)]) == "refuses:a materialising run"
    assert last("lengths", [("series_lengths", 0), ("consumer", 0)]) == "refuses:per-problem lengths"
    assert last("lengths", [("series_lengths", 0), ("set_summarize_mode", 2)]) == "refuses:the forced role-split summarize"
    assert last("warm", [("series_lengths", 0)]) == "refuses:do not carry per-problem lengths"
    assert last("wide", [("series_lengths", 0)]) == "refuses:per-problem lengths cover narrow plans"
    with pytest.raises(AssertionError):
        pm.replay("narrow", 0, [("materialize", 0), ("set_exact", 1), ("consumer", 0)])   # (the factor is the old settings')


def test_the_amplitudes_the_walks_draw_keep_the_scale_away_from_zero():
    """``min |s| >= _amplitude_cases.S_MIN`` within every length, for every basis and every amplitudes the walks can draw
    (kind, ``k % 4``, index 1..6, every seed a family uses); the deliberate zero is zero on ZERO_PROBLEM alone, inside its
    shortest length."""
    from _amplitude_cases import S_MIN, host_scale
    for fam in FAMILIES:
        c = pm.FAMILIES[fam]
        seeds = set(range(pm.SEEDS[fam])) | set(seed for seed, _ in pm.LITERAL.get(fam, []))
        kinds = ("shared", "per") + (("nan",) if c["lengths"] else ())
        shortest = np.min(c["lengths"], axis=0) if c["lengths"] else [c["N"]] * c["B"]
        for seed in sorted(seeds):
            for kind in kinds:
                for k in range(4):
                    G = pm.gamma(fam, seed, kind, k)
                    for a in range(1, 7):
                        s = np.abs(host_scale(pm.amplitude_values(fam, seed, a, -1), G))
                        assert np.nanmin(s) >= S_MIN, (fam, seed, kind, k, a, np.nanmin(s))
                        if kind == "nan":
                            assert not np.isnan(s[:, :int(np.min(np.max(c["lengths"], axis=0)))]).any() and np.isnan(s[:, -1]).any()
                    st = pm.PlanState(fam, seed)
                    st.gam, st.amp, st.amp_zero = (kind, k), 1 + k, True
                    s = np.abs(host_scale(pm.amplitudes_of(st), G))
                    z = pm.ZERO_PROBLEM
                    assert (s[z, :shortest[z]] == 0.0).any() and np.nanmin(np.delete(s, z, axis=0)) >= S_MIN, (fam, seed, kind, k)


def test_effective_with_amplitudes_is_the_host_formed_series_and_its_log_term():
    import math
    fam, seed = "lengths", 2
    s = pm.PlanState(fam, seed)
    s.ser, s.lengths, s.phi, s.mw, s.psi, s.nw, s.gam, s.amp = 3, 0, 0, 2, ("shared", 1), 3, ("nan", 1), 4
    plain = s.copy()
    plain.gam, plain.amp = None, None
    t0, d0, r0, lens0, L0 = pm.effective(plain)
    t, d, r, lens, L = pm.effective(s)
    a, G = pm.amplitude_values(fam, seed, 4, -1), pm.gamma(fam, seed, "nan", 1)
    assert tuple(lens) == tuple(lens0) == pm.FAMILIES[fam]["lengths"][0] and not L0.any() and G.shape == (5, 3, 1000)
    for b, n in enumerate(lens):
        sc = (a[b, 0] * G[b, 0] + a[b, 1] * G[b, 1]) + a[b, 2] * G[b, 2]
        assert np.array_equal(r[b], r0[b] / sc[:n]) and np.array_equal(d[b], d0[b] / (sc[:n] * sc[:n])) and np.array_equal(t[b], t0[b])
        assert L[b] == math.fsum(np.log(np.abs(sc[:n]))) and np.isfinite(L[b]) and L[b] != 0.0
    # the deliberate zero: that problem's rows and its L are not finite, the others are as without it
    s.gam, s.amp_zero = ("per", 2), True
    t, d, r, lens, L = pm.effective(s)
    z = pm.ZERO_PROBLEM
    assert not np.isfinite(L[z]) and not np.isfinite(d[z]).all() and all(np.isfinite(L[b]) and np.isfinite(d[b]).all() for b in range(5) if b != z)


def test_effective_is_the_numpy_statement_of_the_residual_and_the_variances():
    fam, seed = "lengths", 3
    s = pm.PlanState(fam, seed)
    s.ser, s.lengths, s.phi, s.mw, s.psi, s.nw = 2, 1, 1, 4, ("per", 2), 5
    t, diag, y = pm.series(fam, seed, 2)
    w, Phi = pm.mean_weights(fam, seed, 4), pm.mean_basis(fam, 1)
    sw, Psi = pm.psi_weights(fam, seed, 5), pm.psi(fam, seed, True, 2)
    resid = y - (w[:, 0, None] * Phi[0] + w[:, 1, None] * Phi[1])
    var = diag + ((sw[:, 0, None] * Psi[:, 0] + sw[:, 1, None] * Psi[:, 1]) + sw[:, 2, None] * Psi[:, 2])
    assert np.array_equal(var, host_diag(diag, sw, Psi)) and (var > 0).all() and not np.array_equal(var, diag)
    et, ed, ey, lens, _ = pm.effective(s)
    assert tuple(lens) == pm.FAMILIES[fam]["lengths"][1] == (300, 1000, 513, 511, 77)
    for b, n in enumerate(lens):
        assert et[b].shape == (n,) and np.array_equal(et[b], t[b, :n])
        assert np.array_equal(ed[b], var[b, :n]) and np.array_equal(ey[b], resid[b, :n])
    # what set_series is given: NaN past the lengths
    at, ad, ay, alens = pm.arrays(s)
    assert np.isnan(at[0, 300:]).all() and np.isnan(ad[4, 77:]).all() and np.isnan(ay[2, 513:]).all() and not np.isnan(ay[1]).any()
    # a constant mean on a shared y and a shared diagonal under a shared noise basis, no lengths
    s = pm.PlanState("narrow", 2)
    s.y_shared, s.d_shared, s.mean, s.psi, s.nw = True, True, ("per", 3), ("shared", 1), 2
    t, diag, y = pm.series("narrow", 2, 0)
    mu, sw, Psi = pm.mean_values("narrow", 2, 3), pm.psi_weights("narrow", 2, 2), pm.psi("narrow", 2, False, 1)
    et, ed, ey, lens, _ = pm.effective(s)
    assert Psi.shape == (3, 601) and set(lens) == {601}
    for b in range(5):
        assert np.array_equal(ey[b], y[0] - mu[b])
        assert np.array_equal(ed[b], diag[0] + ((sw[b, 0] * Psi[0] + sw[b, 1] * Psi[1]) + sw[b, 2] * Psi[2]))
    s.mean = ("const", 3)
    assert np.array_equal(pm.effective(s)[2][4], y[0] - mu[0])


def test_the_double_oracle_is_no_truth_at_1e_10_on_the_near_singular_problem():
    """Why test_gpu_plan_walk's anchor takes the one-launch family's near-singular problem out of the 1e-10: at a state the
    walks anchor (a new series, a shared noise basis with weights, kernel parameters; the plan was measured 1.1e-10 from
    the oracle in quad there) ``oracle.ref.batch_log_likelihood`` is itself more than 1e-10 from the same recurrences
    carried in binary128 (``ref.quad_factor_solve``) on that problem -- and within 1e-13 of them on a problem beside it."""
    from celerite_amd import terms
    from oracle import ref

    fam, seed = "one launch", 10
    cfg = pm.FAMILIES[fam]
    saved = pm.kernel_factory
    pm.kernel_factory = lambda JR, JC: pm.make_kernel(terms, JR, JC)
    try:
        state = pm.final_state(fam, seed, pm.replay(fam, seed, [("series_new", 6), ("noise_basis_shared", 1), ("noise_weights", 4),
                                                                ("kernel_params", 7)]))
        assert (state.ser, state.psi, state.nw, state.coef, cfg["ill"]) == (7, ("shared", 1), 5, ("kernel", 7), 3)
        tabs = pm.host_coefficients(state)
    finally:
        pm.kernel_factory = saved
    t, d, r, _, _ = pm.effective(state)
    own = {}
    for b in (cfg["ill"], 0):
        co = [x[b] for x in tabs[:6]]
        _, ld, q, st = ref.batch_log_likelihood(0.0, *[x[None] for x in co], t[b], d[b], r[b])
        _, _, _, ld128, q128 = ref.quad_factor_solve(0.0, *co, t[b], d[b], r[b], want_factor=False)
        assert st[0] == 0
        own[b] = max(abs(ld[0] - ld128) / abs(ld128), abs(q[0] - q128) / abs(q128))
    assert own[cfg["ill"]] > 1e-10 and own[cfg["ill"]] < 1e-9 / 2, own
    assert own[0] < 1e-13, own
