# -*- coding: utf-8 -*-
"""`-m gpu`: a noise model that is linear in its parameters on batched plans (``set_noise_basis`` / ``set_noise_weights``
/ ``grad_noise_weights``; clr_batch_set_noise_basis / _set_noise_weights / _grad_noise_weights and their sharded twins).

The variances ``diag + (s_0 * Psi_0 + s_1 * Psi_1 + ...)`` are formed on the device in a fixed order with every product
and sum rounded on its own, so every route must give the SAME BITS as a fresh plan whose ``set_series`` was given the
diagonal formed on the host by that NumPy expression (``_noise_cases.host_diag``) -- after every change of the weights, on
every route that reads a derived copy of the diagonal.  The values are held against ``oracle.ref.batch_log_likelihood`` on
the host-formed diagonal at the project's 1e-10, and the gradient against ``1/2 sum_n Psi_k (alpha0_n^2 - c0_n)`` with
c0, alpha0 from the oracle as tests/test_gpu_batch_leave_one_out.py obtains them, summed with ``math.fsum``: deviation
<= 1e-10 S_k, ``S_k = 1/2 sum_n |Psi_k[n]| (alpha0_n^2 + c0_n)`` (tests/test_batch_noise_cpu.py shows the oracle itself
5.5e-14 S_k from a 40-digit dense inverse).

Largest deviations measured on an MI355X (the run of this file, 45 tests in 6.1 s), every bar 1e-10:
  loglike / logdet / quad vs oracle.ref.batch_log_likelihood, widths 1, 4, 8, 21      3.9e-14 / 7.9e-15 / 1.2e-14
  grad_noise_weights vs the oracle's sum, of S_k: narrow plans (162 partials) / wide   7.6e-15 / 1.4e-14
  K = 1, Psi = 1 vs column 0 of grad_log_likelihood(), of the largest partial          4.6e-15
  per-problem lengths: loglike / logdet / quad vs the oracle on the truncated series   3.7e-15 / 9.3e-16 / 1.9e-15
  per-problem lengths: gradient value / partials (of the largest) vs oracle.grad       1.2e-15 / 4.9e-14
  bit for bit: every width, K and layout of Psi vs the host-formed diagonal; three changes of the weights on every route;
  1, 2 and 3 shards vs one plan -- equal
"""
import functools

import numpy as np
import pytest

from celerite_amd import batch
from oracle import ref
from _cases import synthetic, coeffs_of, within
from _noise_cases import host_diag, noise_basis, noise_weights, oracle_gradient

pytestmark = pytest.mark.gpu

REL = 1e-10                       # tests/test_gpu_batch_mean.py, test_gpu_batch_linear_mean.py: the project's bar
WIDTHS = [(1, 0), (2, 1), (2, 3)]  # widths 1, 4, 8
WIDE = (1, 10)                     # width 21
EMPTY, EMPTY2 = np.empty(0), np.empty((0, 0))
CLR_NOT_COMPUTED = 3               # include/celerite_hip.h


def _plan(case, JR, JC, diag, setup=None, y=None, cls=batch.BatchedGP, **kw):
    B, N = case["t"].shape
    plan = cls(B, N, JR, JC, **kw)
    if setup:
        setup(plan)
    plan.set_series(case["t"], diag, case["y"] if y is None else y)
    plan.set_coefficients(*coeffs_of(case))
    return plan


def _same(a, b, what):
    for x, z, name in zip(a, b, ("loglike", "logdet", "quad", "status")):
        assert np.array_equal(np.asarray(x), np.asarray(z), equal_nan=(name != "status")), (what, name, x, z)


CHUNKS = {130: 2, 300: 5, 4100: 33}     # N = 130: two chunks of 72, the last one ragged; 300: 5 of 64; 4100: 33 of 128


def _chunked(N):
    return (lambda p: p.set_chunks(CHUNKS[N])) if N in CHUNKS else None


def _fresh_against(plan, case, JR, JC, d, setup, what, materialize=False, deep=False):
    """``plan`` (noise model in force) against a fresh plan whose set_series was given the host-formed diagonal ``d``."""
    fresh = _plan(case, JR, JC, d, setup)
    try:
        got, want = plan.log_likelihood(materialize), fresh.log_likelihood(materialize)
        _same(got, want, what)
        if deep:
            assert np.array_equal(plan.solve(), fresh.solve(), equal_nan=True), what
            for x, z in zip(plan.grad_log_likelihood(), fresh.grad_log_likelihood()):
                assert np.array_equal(x, z, equal_nan=True), what
    finally:
        fresh.close()
    return got


# ---- 1. bits --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("JR,JC", WIDTHS + [WIDE])
def test_noise_model_is_bit_identical_to_the_host_formed_diagonal(JR, JC, K):
    """Every width, K and layout of Psi; a shared diagonal too (it becomes per-problem variances); the basis before and
    after the series; the evaluation, and after a materialising run ``solve()`` and ``grad_log_likelihood()``."""
    B = 3
    for i, N in enumerate([600] if (JR, JC) == WIDE else [130, 300]):
        case = synthetic(B, N, JR, JC, "bench", seed=11 + JR + 7 * JC + N)
        setup = _chunked(N)
        for j, per in enumerate([False, True]):
            diag = case["diag"] if (i + j) % 2 == 0 else case["diag"][0]
            Psi = noise_basis(case["diag"], K, per, seed=K)
            s = noise_weights(B, K, seed=K + N)
            d = host_diag(diag, s, Psi)
            assert (d > 0).all() and (Psi > 0).any() and (Psi < 0).any() and np.abs(Psi).max() > 100 * np.abs(Psi).min()
            a = batch.BatchedGP(B, N, JR, JC)
            try:
                if setup:
                    setup(a)
                if j == 0:                      # basis and weights before the series: set_series applies them
                    a.set_noise_basis(Psi)
                    a.set_noise_weights(s)
                    a.set_series(case["t"], diag, case["y"])
                else:
                    a.set_series(case["t"], diag, case["y"])
                    a.set_noise_basis(Psi)
                    a.set_noise_weights(s)
                a.set_coefficients(*coeffs_of(case))
                what = (JR, JC, K, N, per)
                got = _fresh_against(a, case, JR, JC, d, setup, what)
                assert (got[3] == 0).all()
                _fresh_against(a, case, JR, JC, d, setup, what, materialize=True, deep=True)
            finally:
                a.close()


@pytest.mark.parametrize("JR,JC", [(2, 1), WIDE])
def test_zero_weights_and_a_removed_basis_are_the_plain_plan(JR, JC):
    B, N, K = 3, 600 if (JR, JC) == WIDE else 300, 3
    case = synthetic(B, N, JR, JC, "bench", seed=21)
    Psi = noise_basis(case["diag"], K, True, seed=1)
    s = noise_weights(B, K, seed=1)
    plain = _plan(case, JR, JC, case["diag"])
    a = _plan(case, JR, JC, case["diag"])
    try:
        base = plain.log_likelihood()
        a.set_noise_basis(Psi)
        _same(a.log_likelihood(), base, "zero weights")
        a.set_noise_weights(s)
        moved = a.log_likelihood()
        assert not np.array_equal(moved[1], base[1])
        a.set_noise_weights(np.zeros(K))
        _same(a.log_likelihood(), base, "weights back to zero")
        a.set_noise_weights(s)
        _same(a.log_likelihood(), moved, "the weights again")
        a.set_noise_basis(None)
        _same(a.log_likelihood(), base, "basis removed")
        with pytest.raises(ValueError):
            a.set_noise_weights(s)
        a.set_noise_basis(Psi)                    # a new basis starts from zero weights
        _same(a.log_likelihood(), base, "a new basis: zero weights")
    finally:
        plain.close()
        a.close()


def test_a_problem_driven_to_a_non_positive_variance_shows_in_its_status_alone():
    B, N, JR, JC = 5, 300, 2, 1
    case = synthetic(B, N, JR, JC, "bench", seed=23)
    Psi = np.stack([np.ones(N), noise_basis(case["diag"], 1, False, seed=3)[0]])
    s = np.column_stack([np.zeros(B), noise_weights(B, 1, seed=3)[:, 0]])
    s[3, 0] = -50.0                                # every variance of problem 3 far below zero
    d = host_diag(case["diag"], s, Psi)
    assert (d[3] < 0).all() and (np.delete(d, 3, axis=0) > 0).all()
    a = _plan(case, JR, JC, case["diag"])
    try:
        a.set_noise_basis(Psi)
        a.set_noise_weights(s)
        got = _fresh_against(a, case, JR, JC, d, None, "one indefinite problem")
    finally:
        a.close()
    assert got[3][3] == batch.CLR_NOT_POSITIVE_DEFINITE and (np.delete(got[3], 3) == 0).all()


# ---- 2. nothing stale ----------------------------------------------------------------------------------------------

def _role_split(p):
    p.set_summarize_mode(1)


ROUTES = {
    # name: (B, N, JR, JC, family, setup, check) -- the smallest such shapes of tests/test_gpu_batch_linear_mean.py
    "staged": (5, 4000, 2, 1, "bench", lambda p: p.set_layout("staged"), None),
    "interleaved": (5, 4000, 2, 1, "bench", lambda p: p.set_layout("interleaved"), None),
    "role split": (16, 20000, 2, 3, "bench", _role_split, lambda p: p.summarize_kernel().startswith("role split")),
    "small mode": (4, 2000, 2, 1, "bench", lambda p: p.set_small_mode(1), lambda p: p.small_mode_active()),
    "warm start": (9, 12000, 2, 3, "accuracy", lambda p: p.set_warm_start(1, 128), lambda p: p.warm_start()["active"] == 1),
    "wide": (3, 600, 1, 10, "bench", None, None),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_three_changes_of_the_weights_leave_nothing_stale(route):
    """Each route reads its own derived copy of the diagonal (the scan's chunk-interleaved D, the one-launch copy, the
    warm kernel's copy) or the row-major array: after each of three changes of the weights on ONE plan the bits are a
    fresh plan's.  The first change makes a shared diagonal per problem (a change of stride)."""
    B, N, JR, JC, family, setup, check = ROUTES[route]
    K = 3
    case = synthetic(B, N, JR, JC, family, seed=31)
    diag = case["diag"][0]
    Psi = noise_basis(case["diag"], K, False, seed=4)
    a = _plan(case, JR, JC, diag, setup)
    try:
        a.set_noise_basis(Psi)
        seen = []
        for i in range(3):
            s = noise_weights(B, K, seed=40 + i)
            a.set_noise_weights(s)
            got = _fresh_against(a, case, JR, JC, host_diag(diag, s, Psi), setup, (route, i))
            assert (got[3] == 0).all()
            assert check is None or check(a), route
            seen.append(got[1].copy())
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    finally:
        a.close()


@pytest.mark.parametrize("route", ["interleaved", "role split", "warm start"])
def test_weight_changes_interleaved_with_mean_weights_and_coefficients(route):
    """Noise weights, mean weights and coefficients replaced in both orders: D, Y and the coefficients follow their own
    causes; weights set while an ``enqueue()`` is in flight settle that evaluation first."""
    B, N, JR, JC, family, setup, check = ROUTES[route]
    K = 3
    case = synthetic(B, N, JR, JC, family, seed=33)
    other = synthetic(B, N, JR, JC, family, seed=34)
    Psi = noise_basis(case["diag"], K, True, seed=5)
    Phi = np.stack([np.ones(N), np.linspace(-1.0, 1.0, N)])
    s1, s2 = noise_weights(B, K, seed=51), noise_weights(B, K, seed=52)
    w1, w2 = np.random.RandomState(6).uniform(-0.5, 0.5, (2, B, 2))
    resid = lambda w: case["y"] - (w[:, 0, None] * Phi[0] + w[:, 1, None] * Phi[1])
    a = _plan(case, JR, JC, case["diag"], setup)
    try:
        a.set_noise_basis(Psi)
        a.set_mean_basis(Phi)
        steps = [("noise", s1), ("mean", w1), ("coeffs", other), ("mean", w2), ("noise", s2), ("coeffs", case), ("noise", s1)]
        s, w, co = np.zeros((B, K)), np.zeros((B, 2)), case
        for i, (kind, value) in enumerate(steps):
            if i == 4:
                a.enqueue()                      # in flight while the weights change
            if kind == "noise":
                a.set_noise_weights(value)
                s = value
            elif kind == "mean":
                a.set_mean_weights(value)
                w = value
            else:
                a.set_coefficients(*coeffs_of(value))
                co = value
            fresh = _plan(dict(co, t=case["t"]), JR, JC, host_diag(case["diag"], s, Psi), setup, y=resid(w))
            try:
                _same(a.log_likelihood(), fresh.log_likelihood(), (route, i, kind))
            finally:
                fresh.close()
            assert check is None or check(a), route
    finally:
        a.close()


# ---- 3. the values against the oracle ------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC", WIDTHS + [WIDE])
def test_values_against_the_oracle_on_the_host_formed_diagonal(JR, JC):
    B, K = 3, 3
    for N in ([600] if (JR, JC) == WIDE else [130, 300, 4100]):
        case = synthetic(B, N, JR, JC, "bench", seed=61 + N)
        Psi = noise_basis(case["diag"], K, True, seed=6)
        s = noise_weights(B, K, seed=6)
        d = host_diag(case["diag"], s, Psi)
        a = _plan(case, JR, JC, case["diag"], _chunked(N))
        try:
            a.set_noise_basis(Psi)
            ll, ld, q, st = a.evaluate(*coeffs_of(case), noise_weights=s)
        finally:
            a.close()
        ll0, ld0, q0, st0 = ref.batch_log_likelihood(0.0, *coeffs_of(case), case["t"], d, case["y"])
        assert (st == 0).all() and (np.asarray(st0) == 0).all()
        for name, x, x0 in (("loglike", ll, ll0), ("logdet", ld, ld0), ("quad", q, q0)):
            within("noise model: %s vs oracle.ref.batch_log_likelihood on the host-formed diagonal" % name,
                   np.max(np.abs(x - x0) / np.abs(x0)), REL, (JR, JC, N))


# ---- 4. the gradient -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gradient_case(JR, JC, N, per):
    """The case, its basis and weights and the oracle's gradient, once per session (the arrays are not written to)."""
    B, K = 3, 3
    case = synthetic(B, N, JR, JC, "bench", seed=71 + JR + N)
    Psi = noise_basis(case["diag"], K, per, seed=7)
    s = noise_weights(B, K, seed=7)
    return case, Psi, s, oracle_gradient(case, s, Psi)


def _gradient(JR, JC, N, per, layout, tag):
    case, Psi, s, (g0, S) = _gradient_case(JR, JC, N, per)
    B, K = s.shape

    def setup(p):
        if N in CHUNKS:
            p.set_chunks(CHUNKS[N])
        p.set_factor_layout(layout)

    a = _plan(case, JR, JC, case["diag"], setup)
    try:
        a.set_noise_basis(Psi)
        a.set_noise_weights(s)
        assert (a.log_likelihood(True)[3] == 0).all()
        g, st = a.grad_noise_weights()
        g2, _ = a.grad_noise_weights()
        ms = a.leave_one_out_ms()[:2] + (a.noise_project_ms(),)
    finally:
        a.close()
    assert (st == 0).all() and g.shape == (B, K) and np.array_equal(g, g2) and all(m > 0 for m in ms)
    for p in range(B):
        for k in range(K):
            within("grad_noise_weights vs 1/2 sum Psi_k (alpha0^2 - c0) of the oracle / S_k: " + tag,
                   abs(g[p, k] - g0[p, k]) / S[p, k], REL, (JR, JC, N, per, layout, p, k))


@pytest.mark.parametrize("layout", ["reference", "lean"])
@pytest.mark.parametrize("JR,JC", WIDTHS)
def test_gradient_on_narrow_plans_against_the_oracle(JR, JC, layout):
    """N = 130 (two chunks, the last ragged), 300, and 4100: two slabs of the projection, the second of four samples."""
    for i, N in enumerate([130, 300, 4100]):
        _gradient(JR, JC, N, (i + JR) % 2 == 0, layout, "narrow")


@pytest.mark.parametrize("per", [False, True])
def test_gradient_on_a_wide_plan_against_the_oracle(per):
    _gradient(*WIDE, 600, per, "reference", "wide")


@pytest.mark.parametrize("JR,JC", [(2, 3), WIDE])
def test_one_basis_function_of_ones_is_the_jitter_partial(JR, JC):
    """K = 1, Psi = 1: d K / d s is the identity -- column 0 of ``grad_log_likelihood()`` at a positive jitter, held to
    the bar the existing tests hold that partial to (tests/test_gpu_batch_ragged.py, test_plan_gradient_parallel_in_n):
    1e-10 of the problem's largest partial."""
    B, N = 3, 600
    case = synthetic(B, N, JR, JC, "bench", seed=81)
    s = np.array([[0.01], [0.1], [0.3]])
    a = _plan(case, JR, JC, case["diag"])
    b = batch.BatchedGP(B, N, JR, JC)
    try:
        a.set_noise_basis(np.ones((1, N)))
        a.set_noise_weights(s)
        assert (a.log_likelihood(True)[3] == 0).all()
        g, st = a.grad_noise_weights()
        b.set_series(case["t"], case["diag"], case["y"])
        b.set_coefficients(*coeffs_of(case), jitter=s[:, 0])
        _, gj, st2 = b.grad_log_likelihood()
    finally:
        a.close()
        b.close()
    assert (st == 0).all() and (st2 == 0).all()
    for p in range(B):
        within("grad_noise_weights, K = 1, Psi = 1, vs the jitter partial of grad_log_likelihood (of the largest partial)",
               abs(g[p, 0] - gj[p, 0]) / np.max(np.abs(gj[p])), REL, (JR, JC, p))


# ---- 5. rules ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC", [(2, 1), WIDE])
def test_the_gradient_needs_a_materialising_run_made_after_the_weights(JR, JC):
    B, N, K = 3, 600, 3
    case = synthetic(B, N, JR, JC, "bench", seed=91)
    Psi = noise_basis(case["diag"], K, True, seed=9)
    s1, s2 = noise_weights(B, K, seed=91), noise_weights(B, K, seed=92)
    a = _plan(case, JR, JC, case["diag"])
    try:
        a.set_noise_basis(Psi)
        a.set_noise_weights(s1)
        with pytest.raises(RuntimeError, match="clr_batch_grad_noise_weights"):
            a.grad_noise_weights()                       # no materialising run at all
        a.log_likelihood(True)
        g1, _ = a.grad_noise_weights()
        a.set_noise_weights(s1)                          # identical weights: a no-op, the factor is still theirs
        assert np.array_equal(a.grad_noise_weights()[0], g1)
        a.set_noise_weights(s2)
        for _ in range(2):
            with pytest.raises(RuntimeError, match="clr_batch_grad_noise_weights.*materialise again"):
                a.grad_noise_weights()
            assert batch._load().clr_batch_grad_noise_weights(a._h, batch._ptr(np.empty((B, K))), None) == CLR_NOT_COMPUTED
            a.log_likelihood()                           # a plain evaluation does not write the factor
        a.log_likelihood(True)
        g2, st = a.grad_noise_weights()
        assert (st == 0).all() and not np.array_equal(g1, g2)
        a.set_series(case["t"], case["diag"], case["y"])   # a new series: new variances
        with pytest.raises(RuntimeError, match="materialise again"):
            a.grad_noise_weights()
        a.log_likelihood(True)
        assert np.array_equal(a.grad_noise_weights()[0], g2)
    finally:
        a.close()


def test_an_indefinite_problem_gets_a_row_of_zeros_and_disturbs_no_other():
    B, N, JR, JC, K = 5, 600, 2, 3, 3
    good = synthetic(B, N, JR, JC, "bench", seed=101)
    bad = dict(good, a_real=good["a_real"].copy())
    bad["a_real"][2] *= -40.0                        # not positive definite
    Psi = noise_basis(good["diag"], K, True, seed=10)
    s = noise_weights(B, K, seed=10)
    out = []
    for case in (good, bad):
        a = _plan(case, JR, JC, case["diag"])
        try:
            a.set_noise_basis(Psi)
            a.set_noise_weights(s)
            st = a.log_likelihood(True)[3]
            g, gst = a.grad_noise_weights()
        finally:
            a.close()
        assert np.array_equal(st, gst)
        out.append((g, gst))
    (g0, st0), (g1, st1) = out
    assert (st0 == 0).all() and st1[2] == batch.CLR_NOT_POSITIVE_DEFINITE and (np.delete(st1, 2) == 0).all()
    assert (g1[2] == 0.0).all()
    keep = [0, 1, 3, 4]
    assert np.array_equal(g1[keep], g0[keep]) and np.isfinite(g0).all() and np.abs(g0).min() > 0


def test_refusals_name_the_entry_and_leave_the_plan_as_it_was():
    B, N, JR, JC, K = 3, 600, 2, 1, 3
    case = synthetic(B, N, JR, JC, "bench", seed=111)
    Psi = noise_basis(case["diag"], K, True, seed=11)
    s = noise_weights(B, K, seed=11)
    lens = [600, 350, 599]
    a = batch.BatchedGP(B, N, JR, JC)
    try:                                                 # per-problem lengths
        a.set_series(case["t"], case["diag"], case["y"], lengths=lens)
        a.set_coefficients(*coeffs_of(case))
        a.set_noise_basis(Psi)
        a.set_noise_weights(s)
        before = a.log_likelihood()
        with pytest.raises(RuntimeError, match="clr_batch_grad_noise_weights.*per-problem lengths"):
            a.grad_noise_weights()
        _same(a.log_likelihood(), before, "after the refusal (lengths)")
    finally:
        a.close()
    a = _plan(case, JR, JC, case["diag"])
    try:                                                 # general terms
        rng = np.random.RandomState(3)
        a.set_general(0.01 * rng.rand(N), 0.1 * rng.rand(1, N), 0.1 * rng.rand(1, N))
        a.set_noise_basis(Psi)
        a.set_noise_weights(s)
        before = a.log_likelihood()
        with pytest.raises(RuntimeError, match="clr_batch_grad_noise_weights covers celerite-only plans"):
            a.grad_noise_weights()
        _same(a.log_likelihood(), before, "after the refusal (general terms)")
        # the library's own argument checks, past the Python layer's
        lib = batch._load()
        seventeen = np.ones((17, N))
        assert lib.clr_batch_set_noise_basis(a._h, 17, batch._ptr(seventeen), 0) == batch.CLR_INVALID_ARGUMENT
        assert lib.clr_batch_set_noise_basis(a._h, 3, batch._ptr(seventeen), 7) == batch.CLR_INVALID_ARGUMENT
        nan_basis = Psi.copy()
        nan_basis[1, 2, 17] = np.nan
        assert lib.clr_batch_set_noise_basis(a._h, K, batch._ptr(nan_basis), K * N) == batch.CLR_INVALID_ARGUMENT
        nan_s = s.copy()
        nan_s[2, 1] = np.inf
        assert lib.clr_batch_set_noise_weights(a._h, batch._ptr(nan_s)) == batch.CLR_INVALID_ARGUMENT
        _same(a.log_likelihood(), before, "after the refused arguments")
        a.set_noise_basis(None)
        assert lib.clr_batch_set_noise_weights(a._h, batch._ptr(s)) == batch.CLR_INVALID_ARGUMENT      # no basis
    finally:
        a.close()


# ---- 6. per-problem lengths ----------------------------------------------------------------------------------------

def test_noise_weights_on_a_plan_with_per_problem_lengths():
    """NaN in the tails of Psi and of diag: ``log_likelihood()`` and ``grad_log_likelihood()`` are those of each truncated
    series with the host-formed diagonal; the bars of tests/test_gpu_batch_ragged.py (1e-10 on the values and on the
    gradient's value, 1e-10 of the largest partial on the partials)."""
    from oracle import grad as ograd

    B, N, JR, JC, K = 5, 1000, 2, 3, 3
    lens = [1000, 512, 999, 700, 641]
    jitter = np.array([0.0, 0.01, 0.1, 0.3, 0.0])
    case = synthetic(B, N, JR, JC, "bench", seed=121)
    Psi = noise_basis(case["diag"], K, True, seed=12)
    s1, s = noise_weights(B, K, seed=120), noise_weights(B, K, seed=12)
    d = host_diag(case["diag"], s, Psi)
    t, diag, y, Psi_nan = case["t"].copy(), case["diag"].copy(), case["y"].copy(), Psi.copy()
    for b, n in enumerate(lens):
        t[b, n:], diag[b, n:], y[b, n:], Psi_nan[b, :, n:] = np.nan, np.nan, np.nan, np.nan
    a = batch.BatchedGP(B, N, JR, JC)
    try:
        a.set_chunks(24)
        a.set_series(t, diag, y, lengths=lens)
        a.set_noise_basis(Psi_nan)
        a.set_noise_weights(s1)
        a.set_coefficients(*coeffs_of(case), jitter=jitter)
        first = a.log_likelihood()
        a.set_noise_weights(s)
        ll, ld, q, st = a.log_likelihood()
        v, g, gst = a.grad_log_likelihood()
    finally:
        a.close()
    assert (st == 0).all() and (gst == 0).all() and not np.array_equal(first[1], ld)
    for b, n in enumerate(lens):
        r = ref.RefSolver()
        r.compute(jitter[b], *coeffs_of(case, b), EMPTY, EMPTY2, EMPTY2, case["t"][b, :n], d[b, :n])
        ld0, q0 = r.log_determinant(), r.dot_solve(case["y"][b, :n])
        ll0 = -0.5 * (q0 + ld0 + n * 1.8378770664093453)
        for name, x, x0 in (("loglike", ll[b], ll0), ("logdet", ld[b], ld0), ("quad", q[b], q0)):
            within("ragged plan with noise weights: %s vs oracle on the truncated series" % name, abs(x - x0) / abs(x0), REL, b)
        v0, g0 = ograd.grad_log_likelihood(jitter[b], *coeffs_of(case, b), EMPTY, EMPTY2, EMPTY2, case["t"][b, :n], case["y"][b, :n],
                                           d[b, :n])
        within("ragged plan with noise weights: gradient value vs oracle.grad", abs(v[b] - v0) / abs(v0), 1e-10, b)
        within("ragged plan with noise weights: gradient partials vs oracle.grad (of the largest partial)",
               np.max(np.abs(g[b] - g0)) / np.max(np.abs(g0)), 1e-10, b)


# ---- 7. sharding ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", [False, True])
def test_sharded_plans_return_the_unsharded_bits(per):
    B, N, JR, JC, K = 5, 600, 2, 1, 3
    case = synthetic(B, N, JR, JC, "bench", seed=131)
    Psi = noise_basis(case["diag"], K, per, seed=13)
    s = noise_weights(B, K, seed=13)
    single = _plan(case, JR, JC, case["diag"], lambda p: p.set_chunks(8))
    try:
        single.set_noise_basis(Psi)
        want = single.evaluate(*coeffs_of(case), noise_weights=s)
        want_m = single.log_likelihood(True)
        g0, st0 = single.grad_noise_weights()
        assert (st0 == 0).all() and single.noise_project_ms() > 0
        for devices in ([0], [0, 0], [0, 0, 0]):
            sh = batch.ShardedBatchedGP(B, N, JR, JC, devices=devices)
            try:
                sh.set_chunks(8)
                sh.set_series(case["t"], case["diag"], case["y"])
                sh.set_noise_basis(Psi)
                _same(sh.evaluate(*coeffs_of(case), noise_weights=s), want, ("sharded evaluation", len(devices)))
                with pytest.raises(RuntimeError, match="clr_batch_grad_noise_weights"):
                    sh.grad_noise_weights()              # no materialising run yet
                _same(sh.materialize(), want_m, ("sharded materialising run", len(devices)))
                g, st = sh.grad_noise_weights()
                assert np.array_equal(g, g0) and np.array_equal(st, st0) and sh.noise_project_ms() > 0
            finally:
                sh.close()
    finally:
        single.close()
