# -*- coding: utf-8 -*-
"""`-m gpu`: the per-sample amplitude model on batched plans (``set_amplitude_basis`` / ``set_amplitudes`` /
``log_amplitude_sum`` / ``grad_amplitudes``; clr_batch_set_amplitude_basis / _set_amplitudes / _get_log_amplitude_sum /
_grad_amplitudes and their sharded twins).

The scale ``s = a_0 * Gamma_0 + a_1 * Gamma_1 + ...`` and the series ``y' = r / s``, ``d' = d / (s * s)`` are formed on the
device in a fixed order with every operation rounded on its own, so every route must give the SAME BITS as a fresh plan
whose ``set_series`` was given the series formed on the host by those NumPy expressions (``_amplitude_cases.host_scale`` /
``host_series``): ``quad`` and ``status`` equal, ``logdet == fresh + (L + L)`` and ``loglike == fresh - L`` with
``L = log_amplitude_sum()``.  The values are held against ``oracle.ref.batch_log_likelihood`` on the host-formed series
combined with the ``fsum`` of ``log|s|`` at the project's 1e-10, and the gradient against
``sum_n Gamma_k (alpha'_n y'_n + d'_n (c'_n - alpha'_n^2) - 1) / s_n`` with c', alpha' from the oracle, summed with
``math.fsum``: deviation <= 1e-10 S_k, ``S_k = sum_n |Gamma_k[n]| (|alpha'_n y'_n| + d'_n (c'_n + alpha'_n^2) + 1) / |s_n|``
(tests/test_batch_amplitude_cpu.py shows the oracle's own sum 7.3e-15 S_k from the 40-digit dense truth of S K S + D).

Largest deviations measured on an MI355X (the run of this file, 52 tests in 5.4 s), every bar 1e-10 unless stated:
  loglike / logdet / quad vs oracle.ref.batch_log_likelihood and fsum(log|s|), widths 1, 4, 8, 21   3.2e-14 / 3.0e-15 / 1.2e-14
  log_amplitude_sum vs fsum(log|s|), of sum |log|s_n||: uniform plans / per-problem lengths          2.0e-16 / 1.4e-16
  grad_amplitudes vs the oracle's sum, of S_k: narrow plans (162 partials) / wide (18)               4.7e-15 / 2.3e-14
  ... with a linear mean and a noise model in force                                                  2.0e-15
  K = 1, Gamma = 1 vs a central difference of evaluate(), of S_0 (bar 1e-5)                           1.1e-9
  grad_mean_weights / grad_noise_weights with amplitudes in force, of their scales                   5.0e-15 / 1.9e-14
  per-problem lengths: loglike / logdet / quad vs the oracle on the truncated, host-scaled series    1.1e-14 / 6.1e-16 / 6.4e-15
  latent posterior mean / variance vs the dense NumPy expression, of k(0)                             1.2e-14 / 1.9e-15
  bit for bit: every width, K and layout of Gamma vs the host-formed series; three changes of the amplitudes on every
  route; every order of mean weights, noise weights, amplitudes and coefficients; removal; 1, 2 and 3 shards -- equal
"""
import functools

import numpy as np
import pytest

from celerite_amd import batch
from oracle import dense, ref
from _cases import synthetic, coeffs_of, within
from _noise_cases import host_diag, noise_basis, noise_weights, oracle_c_alpha
from _amplitude_cases import (S_MIN, amplitudes, band_basis, host_scale, host_series, log_sum, mean_gradient_scaled,
                              noise_gradient_scaled, oracle_gradient, smooth_basis)

pytestmark = pytest.mark.gpu

REL = 1e-10                        # the project's bar (tests/test_gpu_batch_noise.py)
WIDTHS = [(1, 0), (2, 1), (2, 3)]  # widths 1, 4, 8
WIDE = (1, 10)                     # width 21
EMPTY, EMPTY2 = np.empty(0), np.empty((0, 0))
CLR_NOT_COMPUTED, CLR_UNSUPPORTED = 3, 7   # include/celerite_hip.h
CHUNKS = {130: 2, 300: 5, 4100: 33}  # N = 130: two chunks, the last one ragged; 300: 5 of 64; 4100: 33 of 128


def _chunked(N):
    return (lambda p: p.set_chunks(CHUNKS[N])) if N in CHUNKS else None


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


def _scaled(want, L):
    """The results a plan with amplitudes reports, from those of the fresh plan on the host-formed series."""
    ll, ld, q, st = want
    return ll - L, ld + (L + L), q, st


def _fresh_against(plan, case, JR, JC, yp, dp, setup, what, materialize=False, deep=False):
    """``plan`` (amplitudes in force) against a fresh plan whose set_series was given the host-formed ``yp``, ``dp``."""
    assert yp.shape == dp.shape == case["t"].shape
    fresh = _plan(case, JR, JC, dp, setup, y=yp)
    try:
        L = plan.log_amplitude_sum()
        got, want = plan.log_likelihood(materialize), fresh.log_likelihood(materialize)
        _same(got, _scaled(want, L), what)
        if deep:
            assert np.array_equal(plan.solve(), fresh.solve(), equal_nan=True), what
            (v, g, st), (v0, g0, st0) = plan.grad_log_likelihood(), fresh.grad_log_likelihood()
            assert np.array_equal(g, g0, equal_nan=True) and np.array_equal(st, st0) and np.array_equal(v, v0 - L), what
    finally:
        fresh.close()
    return got


def _check_inputs(s):
    assert np.abs(s).min() >= S_MIN and (s[0] > 0).all() and (s[1] < 0).all()


# ---- 1. bits --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("JR,JC", WIDTHS + [WIDE])
def test_amplitude_model_is_bit_identical_to_the_host_formed_series(JR, JC, K):
    """Every width, K and layout of Gamma (band indicators and a non-indicator basis); a shared y / diag row too (they
    become per problem); the basis before and after the series; the evaluation, L against its ``fsum``, and after a
    materialising run ``solve()`` and ``grad_log_likelihood()``."""
    B = 3
    for i, N in enumerate([600] if (JR, JC) == WIDE else [130, 300]):
        case = synthetic(B, N, JR, JC, "bench", seed=11 + JR + 7 * JC + N)
        setup = _chunked(N)
        for j, per in enumerate([False, True]):
            shared_row = (i + j) % 2 == 1
            diag, y = (case["diag"][0], case["y"][0]) if shared_row else (case["diag"], case["y"])
            G = (band_basis if (i + j + K) % 2 else smooth_basis)(B, N, K, per, seed=K)
            a = amplitudes(B, K, seed=K + N)
            s = host_scale(a, G)
            _check_inputs(s)
            yp, dp = host_series(np.broadcast_to(y, (B, N)), np.broadcast_to(diag, (B, N)), s)
            p = batch.BatchedGP(B, N, JR, JC)
            try:
                if setup:
                    setup(p)
                if j == 0:                      # basis and amplitudes before the series: set_series applies them
                    p.set_amplitude_basis(G)
                    p.set_amplitudes(a)
                    assert (p.log_amplitude_sum() == 0).all()
                    p.set_series(case["t"], diag, y)
                else:
                    p.set_series(case["t"], diag, y)
                    p.set_amplitude_basis(G)
                    p.set_amplitudes(a)
                p.set_coefficients(*coeffs_of(case))
                what = (JR, JC, K, N, per)
                got = _fresh_against(p, case, JR, JC, yp, dp, setup, what)
                assert (got[3] == 0).all()
                _fresh_against(p, case, JR, JC, yp, dp, setup, what, materialize=True, deep=True)
                L, (L0, A) = p.log_amplitude_sum(), log_sum(s)
                within("log_amplitude_sum vs fsum(log|s|), of sum |log|s_n||", np.max(np.abs(L - L0) / A), REL, what)
            finally:
                p.close()


@pytest.mark.parametrize("JR,JC", [(2, 1), WIDE])
def test_a_basis_alone_changes_nothing_and_removal_restores_the_plain_plan(JR, JC):
    B, N, K = 3, 600 if (JR, JC) == WIDE else 300, 3
    case = synthetic(B, N, JR, JC, "bench", seed=21)
    G = band_basis(B, N, K, True, seed=1)
    a = amplitudes(B, K, seed=1)
    plain = _plan(case, JR, JC, case["diag"][0])
    p = _plan(case, JR, JC, case["diag"][0])           # (a shared diagonal: the strides come back too)
    try:
        base = plain.log_likelihood()
        p.set_amplitude_basis(G)
        _same(p.log_likelihood(), base, "a basis alone")
        assert (p.log_amplitude_sum() == 0).all()
        p.set_amplitudes(a)
        moved = p.log_likelihood()
        assert not np.array_equal(moved[1], base[1]) and not np.array_equal(moved[2], base[2])
        p.set_amplitudes(a)                            # equal amplitudes: nothing is done
        _same(p.log_likelihood(), moved, "equal amplitudes")
        p.set_amplitude_basis(G)                       # a new basis drops the amplitudes in force
        _same(p.log_likelihood(), base, "a new basis")
        assert (p.log_amplitude_sum() == 0).all()
        p.set_amplitudes(a)
        _same(p.log_likelihood(), moved, "the amplitudes again")
        p.set_amplitude_basis(None)
        _same(p.log_likelihood(), base, "basis removed")
        _same(p.log_likelihood(True), plain.log_likelihood(True), "basis removed, materialising")
        assert np.array_equal(p.solve(), plain.solve())
        with pytest.raises(ValueError):
            p.set_amplitudes(a)
        # unit amplitudes on a band basis: s = 1, L = 0, the plain plan's bits
        p.set_amplitude_basis(G)
        p.set_amplitudes(np.ones(K))
        _same(p.log_likelihood(), base, "unit amplitudes")
    finally:
        plain.close()
        p.close()


# ---- 2. nothing stale ----------------------------------------------------------------------------------------------

def _role_split(p):
    p.set_summarize_mode(1)


ROUTES = {
    # name: (B, N, JR, JC, family, setup, check) -- the shapes of tests/test_gpu_batch_noise.py
    "staged": (5, 4000, 2, 1, "bench", lambda p: p.set_layout("staged"), None),
    "interleaved": (5, 4000, 2, 1, "bench", lambda p: p.set_layout("interleaved"), None),
    "role split": (16, 20000, 2, 3, "bench", _role_split, lambda p: p.summarize_kernel().startswith("role split")),
    "small mode": (4, 2000, 2, 1, "bench", lambda p: p.set_small_mode(1), lambda p: p.small_mode_active()),
    "warm start": (9, 12000, 2, 3, "accuracy", lambda p: p.set_warm_start(1, 128), lambda p: p.warm_start()["active"] == 1),
    "wide": (3, 600, 1, 10, "bench", None, None),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_three_changes_of_the_amplitudes_leave_nothing_stale(route):
    """Each route reads its own derived copy of the series (the scan's chunk-interleaved Y and D, the one-launch copy, the
    warm kernel's copy) or the row-major arrays: after each of three changes of the amplitudes on ONE plan the bits are a
    fresh plan's.  The first change makes a shared y and diagonal per problem (a change of stride)."""
    B, N, JR, JC, family, setup, check = ROUTES[route]
    K = 3
    case = synthetic(B, N, JR, JC, family, seed=31)
    diag, y = case["diag"][0], case["y"][0]
    G = band_basis(B, N, K, False, seed=4)
    p = _plan(case, JR, JC, diag, setup, y=y)
    try:
        p.set_amplitude_basis(G)
        seen = []
        for i in range(3):
            a = amplitudes(B, K, seed=40 + i)
            p.set_amplitudes(a)
            s = host_scale(a, G)
            _check_inputs(s)
            yp, dp = host_series(np.broadcast_to(y, (B, N)), np.broadcast_to(diag, (B, N)), s)
            got = _fresh_against(p, case, JR, JC, yp, dp, setup, (route, i))
            assert (got[3] == 0).all()
            assert check is None or check(p), route
            seen.append(got[2].copy())
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    finally:
        p.close()


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("route", ["interleaved", "role split", "warm start", "wide"])
def test_amplitudes_composed_with_mean_weights_and_noise_weights(route, order):
    """Amplitudes, mean weights, noise weights and coefficients replaced in every order, the three models set up in both
    orders: y' = (y - Phi w) / s and d' = (diag + Psi q) / (s * s) after every step; a model removed in between; amplitudes
    set while an ``enqueue()`` is in flight settle that evaluation first."""
    B, N, JR, JC, family, setup, check = ROUTES[route]
    K = 3
    case = synthetic(B, N, JR, JC, family, seed=33)
    other = synthetic(B, N, JR, JC, family, seed=34)
    Psi = noise_basis(case["diag"], K, True, seed=5)
    Phi = np.stack([np.ones(N), np.linspace(-1.0, 1.0, N)])
    G = smooth_basis(B, N, K, True, seed=5)
    q1, q2 = noise_weights(B, K, seed=51), noise_weights(B, K, seed=52)
    w1, w2 = np.random.RandomState(6).uniform(-0.5, 0.5, (2, B, 2))
    a1, a2 = amplitudes(B, K, seed=61), amplitudes(B, K, seed=62)
    resid = lambda w: case["y"] - (w[:, 0, None] * Phi[0] + w[:, 1, None] * Phi[1])
    p = _plan(case, JR, JC, case["diag"], setup)
    try:
        if order == 0:                       # the amplitude model first, then the two others
            p.set_amplitude_basis(G)
            p.set_amplitudes(a1)
            p.set_noise_basis(Psi)
            p.set_mean_basis(Phi)
        else:
            p.set_mean_basis(Phi)
            p.set_noise_basis(Psi)
            p.set_amplitude_basis(G)
            p.set_amplitudes(a1)
        steps = [("noise", q1), ("mean", w1), ("amp", a2), ("coeffs", other), ("mean", w2), ("noise", q2), ("amp", a1),
                 ("coeffs", case), ("drop mean", None), ("amp", a2), ("drop noise", None), ("noise basis", None), ("noise", q1),
                 ("mean basis", None), ("mean", w1), ("amp", a1)]
        a, q, w, co = a1, np.zeros((B, K)), np.zeros((B, 2)), case
        for i, (kind, value) in enumerate(steps):
            if i in (2, 6):
                p.enqueue()                  # in flight while the amplitudes change
            if kind == "noise":
                p.set_noise_weights(value); q = value
            elif kind == "mean":
                p.set_mean_weights(value); w = value
            elif kind == "amp":
                p.set_amplitudes(value); a = value
            elif kind == "coeffs":
                p.set_coefficients(*coeffs_of(value)); co = value
            elif kind == "drop mean":
                p.set_mean_basis(None); w = np.zeros((B, 2))
            elif kind == "drop noise":
                p.set_noise_basis(None); q = np.zeros((B, K))
            elif kind == "noise basis":
                p.set_noise_basis(Psi)
            elif kind == "mean basis":
                p.set_mean_basis(Phi)
            s = host_scale(a, G)
            _check_inputs(s)
            yp, dp = host_series(resid(w), host_diag(case["diag"], q, Psi), s)
            _fresh_against(p, dict(co, t=case["t"]), JR, JC, yp, dp, setup, (route, order, i, kind))
            assert check is None or check(p), route
        p.set_amplitude_basis(None)          # removal with the two others in force: their plan, bit for bit
        fresh = _plan(case, JR, JC, host_diag(case["diag"], q, Psi), setup, y=resid(w))
        try:
            _same(p.log_likelihood(), fresh.log_likelihood(), (route, order, "amplitudes removed"))
        finally:
            fresh.close()
    finally:
        p.close()


# ---- 3. the values against the oracle ------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC", WIDTHS + [WIDE])
def test_values_against_the_oracle_on_the_host_formed_series(JR, JC):
    B, K = 3, 3
    for N in ([600] if (JR, JC) == WIDE else [130, 300, 4100]):
        case = synthetic(B, N, JR, JC, "bench", seed=61 + N)
        G = band_basis(B, N, K, True, seed=6) if N != 300 else smooth_basis(B, N, K, False, seed=6)
        a = amplitudes(B, K, seed=6)
        s = host_scale(a, G)
        _check_inputs(s)
        yp, dp = host_series(case["y"], case["diag"], s)
        L0, A = log_sum(s)
        p = _plan(case, JR, JC, case["diag"], _chunked(N))
        try:
            p.set_amplitude_basis(G)
            p.set_amplitudes(a)
            ll, ld, q, st = p.evaluate(*coeffs_of(case))
            L = p.log_amplitude_sum()
        finally:
            p.close()
        ll0, ld0, q0, st0 = ref.batch_log_likelihood(0.0, *coeffs_of(case), case["t"], dp, yp)
        ll0, ld0 = ll0 - L0, ld0 + 2.0 * L0
        assert (st == 0).all() and (np.asarray(st0) == 0).all()
        for name, x, x0 in (("loglike", ll, ll0), ("logdet", ld, ld0), ("quad", q, q0)):
            within("amplitude model: %s vs oracle.ref.batch_log_likelihood on the host-formed series and fsum(log|s|)" % name,
                   np.max(np.abs(x - x0) / np.abs(x0)), REL, (JR, JC, N))
        within("log_amplitude_sum vs fsum(log|s|), of sum |log|s_n||", np.max(np.abs(L - L0) / A), REL, (JR, JC, N))


# ---- 4. the gradients ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gradient_case(JR, JC, N, per):
    """The case, its basis and amplitudes and the oracle's gradient, once per session (the arrays are not written to)."""
    B, K = 3, 3
    case = synthetic(B, N, JR, JC, "bench", seed=71 + JR + N)
    G = (smooth_basis if per else band_basis)(B, N, K, per, seed=7)
    a = amplitudes(B, K, seed=7)
    _check_inputs(host_scale(a, G))
    return case, G, a, oracle_gradient(case, a, G)


def _gradient(JR, JC, N, per, layout, tag):
    case, G, a, (g0, S) = _gradient_case(JR, JC, N, per)
    B, K = a.shape

    def setup(p):
        if N in CHUNKS:
            p.set_chunks(CHUNKS[N])
        p.set_factor_layout(layout)

    p = _plan(case, JR, JC, case["diag"], setup)
    try:
        p.set_amplitude_basis(G)
        p.set_amplitudes(a)
        assert (p.log_likelihood(True)[3] == 0).all()
        g, st = p.grad_amplitudes()
        g2, _ = p.grad_amplitudes()
        ms = p.leave_one_out_ms()[:2] + (p.amplitude_project_ms(),)
    finally:
        p.close()
    assert (st == 0).all() and g.shape == (B, K) and np.array_equal(g, g2) and all(m > 0 for m in ms)
    for b in range(B):
        for k in range(K):
            within("grad_amplitudes vs the oracle's sum / S_k: " + tag, abs(g[b, k] - g0[b, k]) / S[b, k], REL,
                   (JR, JC, N, per, layout, b, k))


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
def test_one_amplitude_for_all_samples_against_a_central_difference_of_evaluate(JR, JC):
    """K = 1, Gamma = 1: d loglike / d a by central differences of ``evaluate`` in a, at the accuracy the difference has.  A
    step h = 1e-4 |a|: each evaluation is good to the project's 1e-10 of |loglike| <= 2e3, so the difference carries at most
    2 x 2e-7 / (2 h) ~ 2e-3, and its truncation h^2 |d^3 loglike / d a^3| / 6 ~ 1e-8 N / |a|^3 ~ 1e-5; the scale S_0 is at
    least N / max|a| = 460: together below 5e-6 S_0.  Bar 1e-5 S_0."""
    B, N = 3, 600
    case = synthetic(B, N, JR, JC, "bench", seed=81)
    G = np.ones((1, N))
    a0 = np.array([[1.3], [-0.7], [0.9]])
    h = 1e-4 * np.abs(a0)
    p = _plan(case, JR, JC, case["diag"])
    try:
        p.set_amplitude_basis(G)
        p.set_amplitudes(a0)
        assert (p.log_likelihood(True)[3] == 0).all()
        g, st = p.grad_amplitudes()
        p.set_amplitudes(a0 + h)
        up = p.evaluate(*coeffs_of(case))[0]
        p.set_amplitudes(a0 - h)
        dn = p.evaluate(*coeffs_of(case))[0]
    finally:
        p.close()
    _, S = oracle_gradient(case, a0, G)
    assert (st == 0).all()
    for b in range(B):
        within("grad_amplitudes, K = 1, Gamma = 1, vs a central difference of evaluate() / S_0",
               abs(g[b, 0] - (up[b] - dn[b]) / (2 * h[b, 0])) / S[b, 0], 1e-5, (JR, JC, b))
        assert S[b, 0] >= N / 1.3 and abs(up[b]) <= 2e3


@pytest.mark.parametrize("JR,JC", [(2, 1), WIDE])
def test_mean_and_noise_weight_gradients_with_amplitudes_in_force(JR, JC):
    """``grad_mean_weights`` = sum Phi_k alpha' / s and ``grad_noise_weights`` = 1/2 sum Psi_k (alpha'^2 - c') / s^2 against
    the oracle's c', alpha' on the host-formed series, at 1e-10 of their scales; ``grad_amplitudes`` with both in force."""
    B, N, K = 3, 600 if (JR, JC) == WIDE else 300, 3
    case = synthetic(B, N, JR, JC, "bench", seed=85)
    Phi = np.stack([np.ones(N), np.linspace(-1.0, 1.0, N)])
    w = np.random.RandomState(8).uniform(-0.5, 0.5, (B, 2))
    resid = case["y"] - (w[:, 0, None] * Phi[0] + w[:, 1, None] * Phi[1])
    Psi = noise_basis(case["diag"], K, True, seed=8)
    q = noise_weights(B, K, seed=8)
    D = host_diag(case["diag"], q, Psi)
    G = smooth_basis(B, N, K, True, seed=8)
    a = amplitudes(B, K, seed=8)
    s = host_scale(a, G)
    _check_inputs(s)
    yp, dp = host_series(resid, D, s)
    p = _plan(case, JR, JC, case["diag"], _chunked(N))
    try:
        p.set_mean_basis(Phi)
        p.set_noise_basis(Psi)
        p.set_amplitude_basis(G)
        p.set_mean_weights(w)
        p.set_amplitudes(a)
        p.set_noise_weights(q)
        _fresh_against(p, case, JR, JC, yp, dp, _chunked(N), "all three models", materialize=True)
        gm, st1 = p.grad_mean_weights()
        gn, st2 = p.grad_noise_weights()
        ga, st3 = p.grad_amplitudes()
        with pytest.raises(RuntimeError, match="clr_batch_fit_mean_weights.*amplitudes are in force"):
            p.fit_mean_weights()
        assert batch._load().clr_batch_fit_mean_weights(p._h, 1e-10, *[None] * 5, None) == CLR_UNSUPPORTED
        p.set_amplitude_basis(None)
        p.log_likelihood(True)
        assert (p.fit_mean_weights().status == 0).all()        # works again after removal
    finally:
        p.close()
    assert (st1 == 0).all() and (st2 == 0).all() and (st3 == 0).all()
    ga0, Sa = oracle_gradient(case, a, G, resid=resid, diag=D)
    for b in range(B):
        c, al = oracle_c_alpha(case, b, dp[b], yp[b])
        gm0, Sm = mean_gradient_scaled(Phi, al, s[b])
        gn0, Sn = noise_gradient_scaled(Psi[b], al, c, s[b])
        for k in range(2):
            within("grad_mean_weights with amplitudes in force vs the oracle's sum / scale", abs(gm[b, k] - gm0[k]) / Sm[k], REL, (JR, JC, b, k))
        for k in range(K):
            within("grad_noise_weights with amplitudes in force vs the oracle's sum / scale", abs(gn[b, k] - gn0[k]) / Sn[k], REL, (JR, JC, b, k))
            within("grad_amplitudes with a mean and a noise model in force vs the oracle's sum / S_k", abs(ga[b, k] - ga0[b, k]) / Sa[b, k], REL,
                   (JR, JC, b, k))


# ---- 5. rules ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC", [(2, 1), WIDE])
def test_the_gradient_needs_a_materialising_run_made_after_the_amplitudes(JR, JC):
    B, N, K = 3, 600, 3
    case = synthetic(B, N, JR, JC, "bench", seed=91)
    G = band_basis(B, N, K, True, seed=9)
    Psi = noise_basis(case["diag"], K, True, seed=9)
    a1, a2 = amplitudes(B, K, seed=91), amplitudes(B, K, seed=92)
    p = _plan(case, JR, JC, case["diag"])
    try:
        p.set_amplitude_basis(G)
        p.set_noise_basis(Psi)
        p.set_amplitudes(a1)
        with pytest.raises(RuntimeError, match="clr_batch_grad_amplitudes"):
            p.grad_amplitudes()                          # no materialising run at all
        p.log_likelihood(True)
        g1, _ = p.grad_amplitudes()
        p.set_amplitudes(a1)                             # identical amplitudes: a no-op, the factor is still theirs
        assert np.array_equal(p.grad_amplitudes()[0], g1)
        changes = [lambda: p.set_amplitudes(a2), lambda: p.set_noise_weights(noise_weights(B, K, seed=9)),
                   lambda: p.set_series(case["t"], case["diag"], case["y"])]
        for change in changes:
            change()
            with pytest.raises(RuntimeError, match="clr_batch_grad_amplitudes.*materialise again"):
                p.grad_amplitudes()
            assert batch._load().clr_batch_grad_amplitudes(p._h, batch._ptr(np.empty((B, K))), None) == CLR_NOT_COMPUTED
            p.log_likelihood()                           # a plain evaluation does not write the factor
            with pytest.raises(RuntimeError, match="materialise again"):
                p.grad_amplitudes()
            p.log_likelihood(True)
            g2, st = p.grad_amplitudes()
            assert (st == 0).all() and np.isfinite(g2).all()
        assert not np.array_equal(g1, g2)
    finally:
        p.close()


def test_a_zero_scale_refuses_its_problem_alone():
    """One problem with s_n = 0 inside its length (a band whose amplitude is zero): NaN and CLR_INVALID_ARGUMENT for that
    problem wherever results come back, a row of zeros in the gradients; the other problems' bits equal the run without it."""
    B, N, JR, JC, K = 5, 300, 2, 1, 3
    case = synthetic(B, N, JR, JC, "bench", seed=101)
    G = band_basis(B, N, K, False, seed=10)
    good = amplitudes(B, K, seed=10)
    bad = good.copy()
    bad[3, 1] = 0.0
    assert (host_scale(bad, G)[3] == 0).any()
    keep = [0, 1, 2, 4]
    out = []
    for a in (good, bad):
        p = _plan(case, JR, JC, case["diag"], _chunked(N))
        try:
            p.set_amplitude_basis(G)
            p.set_amplitudes(a)
            res = p.log_likelihood(True)
            ev = p.evaluate(*coeffs_of(case))
            v, g, gst = p.grad_log_likelihood()
            p.log_likelihood(True)
            da, dst = p.grad_amplitudes()
            out.append((res, ev, v, g, gst, da, dst, p.log_amplitude_sum()))
        finally:
            p.close()
    (res0, ev0, v0, g0, gst0, da0, dst0, L0), (res1, ev1, v1, g1, gst1, da1, dst1, L1) = out
    assert (res0[3] == 0).all() and (dst0 == 0).all() and np.isfinite(da0).all()
    for r0, r1 in ((res0, res1), (ev0, ev1)):
        assert r1[3][3] == batch.CLR_INVALID_ARGUMENT and all(np.isnan(r1[i][3]) for i in range(3))
        for i in range(4):
            assert np.array_equal(r1[i][keep], r0[i][keep])
    assert np.isnan(v1[3]) and np.isnan(g1[3]).all() and gst1[3] == batch.CLR_INVALID_ARGUMENT
    assert np.array_equal(v1[keep], v0[keep]) and np.array_equal(g1[keep], g0[keep]) and np.array_equal(gst1[keep], gst0[keep])
    assert dst1[3] == batch.CLR_INVALID_ARGUMENT and (da1[3] == 0).all() and np.array_equal(da1[keep], da0[keep])
    assert np.array_equal(L1[keep], L0[keep])


def test_argument_refusals_leave_the_plan_unchanged_and_the_two_constant_rules():
    B, N, JR, JC, K = 3, 300, 2, 1, 3
    case = synthetic(B, N, JR, JC, "bench", seed=111)
    G = band_basis(B, N, K, True, seed=11)
    a = amplitudes(B, K, seed=11)
    lib = batch._load()
    p = _plan(case, JR, JC, case["diag"])
    try:
        assert lib.clr_batch_set_amplitudes(p._h, batch._ptr(a)) == batch.CLR_INVALID_ARGUMENT          # no basis
        p.set_amplitude_basis(G)
        p.set_amplitudes(a)
        before = p.log_likelihood()
        seventeen = np.ones((17, N))
        assert lib.clr_batch_set_amplitude_basis(p._h, 17, batch._ptr(seventeen), 0) == batch.CLR_INVALID_ARGUMENT
        assert lib.clr_batch_set_amplitude_basis(p._h, 3, batch._ptr(seventeen), 7) == batch.CLR_INVALID_ARGUMENT
        nan_basis = G.copy()
        nan_basis[1, 2, 17] = np.nan
        assert lib.clr_batch_set_amplitude_basis(p._h, K, batch._ptr(nan_basis), K * N) == batch.CLR_INVALID_ARGUMENT
        nan_a = a.copy()
        nan_a[2, 1] = np.inf
        assert lib.clr_batch_set_amplitudes(p._h, batch._ptr(nan_a)) == batch.CLR_INVALID_ARGUMENT
        # a constant mean while an amplitude basis is set
        with pytest.raises(RuntimeError, match="clr_batch_set_mean: an amplitude basis is set"):
            p.set_mean(0.5)
        _same(p.log_likelihood(), before, "after the refused arguments")
        # ... and the other order: the basis is refused while a constant mean is in force
        p.set_amplitude_basis(None)
        p.set_mean(0.5)
        with_mean = p.log_likelihood()
        with pytest.raises(RuntimeError, match="clr_batch_set_amplitude_basis: a constant mean is in force"):
            p.set_amplitude_basis(G)
        _same(p.log_likelihood(), with_mean, "after the refused basis")
        p.set_mean(None)
        p.set_amplitude_basis(G)
        p.set_amplitudes(a)
        _same(p.log_likelihood(), before, "the amplitude model again")
        # the gradient's domain: general terms
        rng = np.random.RandomState(3)
        p.set_general(0.01 * rng.rand(N), 0.1 * rng.rand(1, N), 0.1 * rng.rand(1, N))
        with_general = p.log_likelihood()
        with pytest.raises(RuntimeError, match="clr_batch_grad_amplitudes covers celerite-only plans"):
            p.grad_amplitudes()
        _same(p.log_likelihood(), with_general, "after the refusal (general terms)")
    finally:
        p.close()


# ---- 6. per-problem lengths ----------------------------------------------------------------------------------------

def test_amplitudes_on_a_plan_with_per_problem_lengths():
    """NaN in the tails of Gamma, y and diag: the values are those of each truncated, host-scaled series; the coefficient
    gradient equals a fresh ragged plan's, bit for bit; ``grad_amplitudes`` and ``materialize`` are refused with the
    existing message and the plan evaluates afterwards as before; a zero of s in a tail is harmless."""
    B, N, JR, JC, K = 5, 300, 2, 3, 3
    lens = [300, 1, 17, 299, 141]
    jitter = np.array([0.0, 0.01, 0.1, 0.3, 0.0])
    case = synthetic(B, N, JR, JC, "bench", seed=121)
    G = band_basis(B, N, K, True, seed=12)
    G[2] = 0.0
    G[2, 0, 17:] = 1.0                                   # problem 2: band 0 lives in its tail alone ...
    G[2, 1, :17] = 1.0                                   # ... and its 17 samples are all of band 1
    a1, a = amplitudes(B, K, seed=120), amplitudes(B, K, seed=12)
    a[2, 0] = 0.0                                        # s = 0 in problem 2's tail only
    s = host_scale(a, G)
    assert (s[2, 17:] == 0).all() and all(np.abs(s[b, :n]).min() >= S_MIN for b, n in enumerate(lens))
    yp, dp = host_series(case["y"], case["diag"], np.where(s == 0, 1.0, s))
    t, diag, y, G_nan = case["t"].copy(), case["diag"].copy(), case["y"].copy(), G.copy()
    for b, n in enumerate(lens):
        t[b, n:], diag[b, n:], y[b, n:] = np.nan, np.nan, np.nan
        if b != 2:
            G_nan[b, :, n:] = np.nan
    p = batch.BatchedGP(B, N, JR, JC)
    fresh = batch.BatchedGP(B, N, JR, JC)
    try:
        for plan in (p, fresh):
            plan.set_chunks(12)
        p.set_series(t, diag, y, lengths=lens)
        p.set_amplitude_basis(G_nan)
        p.set_amplitudes(a1)
        p.set_coefficients(*coeffs_of(case), jitter=jitter)
        first = p.log_likelihood()
        p.set_amplitudes(a)
        ll, ld, q, st = p.log_likelihood()
        L = p.log_amplitude_sum()
        v, g, gst = p.grad_log_likelihood()
        fresh.set_series(case["t"], dp, yp, lengths=lens)
        fresh.set_coefficients(*coeffs_of(case), jitter=jitter)
        _same((ll, ld, q, st), _scaled(fresh.log_likelihood(), L), "ragged: against a fresh ragged plan")
        v0, g0, gst0 = fresh.grad_log_likelihood()
        assert np.array_equal(g, g0) and np.array_equal(gst, gst0) and np.array_equal(v, v0 - L)
        with pytest.raises(RuntimeError, match="clr_batch_grad_amplitudes.*per-problem lengths"):
            p.grad_amplitudes()
        with pytest.raises(RuntimeError, match="per-problem lengths"):
            p.log_likelihood(True)
        _same(p.log_likelihood(), (ll, ld, q, st), "after the refusals (lengths)")
        # the same series set again keeps basis and amplitudes in force
        p.set_series(t, diag, y, lengths=lens)
        _same(p.log_likelihood(), (ll, ld, q, st), "the series set again")
    finally:
        p.close()
        fresh.close()
    assert (st == 0).all() and (gst == 0).all() and not np.array_equal(first[2], q)
    L0, A = log_sum(s, lens)
    within("ragged plan: log_amplitude_sum vs fsum(log|s|) over each length, of sum |log|s_n||", np.max(np.abs(L - L0) / np.maximum(A, 1e-300)), REL)
    for b, n in enumerate(lens):
        r = ref.RefSolver()
        r.compute(jitter[b], *coeffs_of(case, b), EMPTY, EMPTY2, EMPTY2, case["t"][b, :n], dp[b, :n])
        ld0, q0 = r.log_determinant(), r.dot_solve(yp[b, :n])
        ll0 = -0.5 * (q0 + ld0 + n * 1.8378770664093453) - L0[b]
        ld0 = ld0 + 2.0 * L0[b]
        for name, x, x0 in (("loglike", ll[b], ll0), ("logdet", ld[b], ld0), ("quad", q[b], q0)):
            within("ragged plan with amplitudes: %s vs the oracle on the truncated, host-scaled series" % name, abs(x - x0) / abs(x0), REL, b)


# ---- 7. sharding ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", [False, True])
def test_sharded_plans_return_the_unsharded_bits(per):
    B, N, JR, JC, K = 5, 600, 2, 1, 3
    case = synthetic(B, N, JR, JC, "bench", seed=131)
    G = (smooth_basis if per else band_basis)(B, N, K, per, seed=13)
    Psi = noise_basis(case["diag"], K, per, seed=13)
    Phi = np.stack([np.ones(N), np.linspace(-1.0, 1.0, N)])
    a, q = amplitudes(B, K, seed=13), noise_weights(B, K, seed=13)
    w = np.random.RandomState(13).uniform(-0.5, 0.5, (B, 2))

    def run(plan, materialize):
        plan.set_amplitude_basis(G)
        plan.set_noise_basis(Psi)
        plan.set_mean_basis(Phi)
        plan.set_amplitudes(a)
        ev = plan.evaluate(*coeffs_of(case), mean_weights=w, noise_weights=q)
        with pytest.raises(RuntimeError, match="clr_batch_grad_amplitudes"):
            plan.grad_amplitudes()                       # no materialising run yet
        m = materialize(plan)
        grads = plan.grad_amplitudes(), plan.grad_mean_weights(), plan.grad_noise_weights()
        assert plan.amplitude_project_ms() > 0
        return ev, m, plan.log_amplitude_sum(), grads

    single = _plan(case, JR, JC, case["diag"], lambda p: p.set_chunks(8))
    try:
        ev0, m0, L0, grads0 = run(single, lambda p: p.log_likelihood(True))
        assert (ev0[3] == 0).all() and all((st == 0).all() for _, st in grads0)
        for devices in ([0], [0, 0], [0, 0, 0]):
            sh = batch.ShardedBatchedGP(B, N, JR, JC, devices=devices)
            try:
                sh.set_chunks(8)
                sh.set_series(case["t"], case["diag"], case["y"])
                ev, m, L, grads = run(sh, lambda p: p.materialize())
                _same(ev, ev0, ("sharded evaluation", len(devices)))
                _same(m, m0, ("sharded materialising run", len(devices)))
                assert np.array_equal(L, L0)
                for (g, st), (g0, st0) in zip(grads, grads0):
                    assert np.array_equal(g, g0) and np.array_equal(st, st0), len(devices)
            finally:
                sh.close()
    finally:
        single.close()


# ---- 8. the posterior of the latent process ------------------------------------------------------------------------

def test_predict_returns_the_posterior_of_the_latent_process():
    """``predict(xs, return_var=True)`` with amplitudes in force equals a fresh plan on the host-formed series bit for bit,
    and the dense NumPy ``k*^T S K_y^-1 r`` / ``k** - k*^T S K_y^-1 S k*`` of the data-unit matrix to 1e-10 of k(0)."""
    B, N, JR, JC, K = 3, 130, 2, 1, 3
    case = synthetic(B, N, JR, JC, "bench", seed=141)
    G = band_basis(B, N, K, True, seed=14)
    a = amplitudes(B, K, seed=14)
    s = host_scale(a, G)
    _check_inputs(s)
    yp, dp = host_series(case["y"], case["diag"], s)
    xs = np.sort(np.concatenate([case["t"][0, ::13], case["t"][0, :-1:17] + 0.3 * np.diff(case["t"][0])[::17]]))
    p = _plan(case, JR, JC, case["diag"], _chunked(N))
    fresh = _plan(case, JR, JC, dp, _chunked(N), y=yp)
    try:
        p.set_amplitude_basis(G)
        p.set_amplitudes(a)
        p.log_likelihood(True)
        fresh.log_likelihood(True)
        mu, var = p.predict(xs, return_var=True)
        mu0, var0 = fresh.predict(xs, return_var=True)
    finally:
        p.close()
        fresh.close()
    assert np.array_equal(mu, mu0) and np.array_equal(var, var0)
    for b in range(B):
        co = coeffs_of(case, b)
        k0 = float(dense.kernel_value(*co, np.zeros(1))[0])
        K0 = dense.kernel_value(*co, case["t"][b][:, None] - case["t"][b][None, :])
        Ky = s[b][:, None] * K0 * s[b][None, :] + np.diag(case["diag"][b])
        ks = dense.kernel_value(*co, xs[:, None] - case["t"][b][None, :]) * s[b][None, :]      # cov(f(x*), y)
        sol = np.linalg.solve(Ky, np.column_stack([case["y"][b], ks.T]))
        within("latent posterior mean vs the dense k*^T S K_y^-1 r, of k(0)", np.max(np.abs(mu[b] - ks @ sol[:, 0])) / k0, REL, b)
        within("latent posterior variance vs the dense k** - k*^T S K_y^-1 S k*, of k(0)",
               np.max(np.abs(var[b] - (k0 - np.einsum("mn,nm->m", ks, sol[:, 1:])))) / k0, REL, b)
