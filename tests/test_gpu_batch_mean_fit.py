# -*- coding: utf-8 -*-
"""The generalised-least-squares fit of a linear mean's weights on batched plans (clr_batch_fit_mean_weights and its
sharded twin): w = w0 + G^-1 d with G = Phi^T K^-1 Phi and d = Phi^T K^-1 r from right-hand sides formed on the device, a
bordered Gram pass and one small solve per problem.  The Gram matrix is held against the binary128 solves of the oracle
(oracle.ref.quad_factor_solve) at the bar the weight gradient is held to; the small solve against a long-double Cholesky
of the device's own Gram matrix at the forward bound of a K x K Cholesky solve.  The accuracy cases use the well-conditioned
basis of _mean_fit.fit_basis and assert kappa_2(G_s) <= 2 on their truth: the tolerances are stated for that regime."""
import numpy as np
import pytest

from celerite_amd import batch
from oracle import ref
from _cases import coeffs_of, synthetic, within
from _mean_fit import LD, fit_basis, ld_fit, small_solve_bound, small_solve_errors
from test_gpu_batch_linear_mean import basis_of, host_residual

pytestmark = pytest.mark.gpu

REL = 1e-10                      # tests/test_gpu_batch_linear_mean.py: the bar of Phi_k^T K^-1 r
FIELDS = batch.MeanFit._fields


def _inputs(case, B, K, phi_kind, seed=3, zero=False):
    """``(y, Phi, w0, r)``: y per problem, the basis shared (of problem 0's times) or per problem, start weights random in
    [-1.5, 1.5] and the residual the device forms from them."""
    Phi = fit_basis(case["t"], K) if phi_kind == "per" else fit_basis(case["t"][0], K)
    w0 = np.zeros((B, K)) if zero else np.random.RandomState(seed).uniform(-1.5, 1.5, (B, K))
    return case["y"], Phi, w0, host_residual(case["y"], w0, Phi)


def _plan(case, B, N, JR, JC, y, setup=None):
    plan = batch.BatchedGP(B, N, JR, JC)
    if setup:
        setup(plan)
    plan.set_series(case["t"], case["diag"], y)
    plan.set_coefficients(*coeffs_of(case))
    return plan


def _fitted(case, B, N, JR, JC, Phi, w0, setup=None, apply=False, then=None, **kw):
    """A plan with the basis and start weights, materialised, fitted: ``(fit, evaluation, then(plan, fit))``."""
    plan = _plan(case, B, N, JR, JC, case["y"], setup)
    try:
        plan.set_mean_basis(Phi)
        plan.set_mean_weights(w0)
        ev = plan.log_likelihood(True)
        fit = plan.fit_mean_weights(apply=apply, **kw)
        return fit, ev, (then(plan, fit) if then else None)
    finally:
        plan.close()


def _same_fit(a, b, what, rows=None):
    for name in FIELDS:
        x, z = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
        if rows is not None:
            x, z = x[rows], z[rows]
        assert np.array_equal(x, z, equal_nan=(name != "status")), (what, name, x, z)


_TRUTH = {}


def _truth(case, key, Phi, w0, r):
    """Per problem ``(S, scale, fit)``: the bordered Gram matrix accumulated in long double from the binary128 solves of
    the K + 1 right-hand sides (its symmetric part), ``scale[j, k] = 1 + max |R_j| sum_n |Z_k|`` and the long-double
    Cholesky fit of it; once per (shape, input) and session."""
    if key not in _TRUTH:
        B, K = w0.shape
        P = np.broadcast_to(Phi, (B, K, r.shape[1]))
        out = []
        for b in range(B):
            R = np.concatenate([P[b], r[b][None]], axis=0)
            Z = np.stack([ref.quad_factor_solve(0.0, *coeffs_of(case, b), case["t"][b], case["diag"][b], R[j],
                                                want_factor=False)[2] for j in range(K + 1)])
            S = np.array([[np.sum(R[j].astype(LD) * Z[k].astype(LD)) for k in range(K + 1)] for j in range(K + 1)], dtype=LD)
            S = (S + S.T) / 2
            scale = 1 + np.max(np.abs(R), axis=1)[:, None] * np.sum(np.abs(Z), axis=1)[None, :]
            out.append((S, scale, ld_fit(S, w0[b])))
        _TRUTH[key] = out
    return _TRUTH[key]


def _against_truth(fit, truth, tag):
    """The bars of the issue: every Gram entry within REL of the truth relative to 1 + max |R_j| sum |Z_k|; weights,
    log det G and the profiled quadratic form within REL relative to 1 + |truth|, the covariance relative to max |cov|;
    kappa_2(G_s) <= 2 asserted first."""
    assert (fit.status == 0).all()
    for b, (S, scale, t) in enumerate(truth):
        assert t["kappa_s"] <= 2.0, t["kappa_s"]
        K = S.shape[0] - 1
        within("bordered Gram entry vs binary128 / (1 + max |R_j| sum |Z_k|): " + tag,
               np.max(np.abs(fit.gram[b] - S) / scale), REL, b)
        within("fitted weights vs truth / (1 + |w|): " + tag,
               np.max(np.abs(fit.weights[b] - t["weights"]) / (1 + np.abs(t["weights"]))), REL, b)
        within("covariance vs truth / max |cov|: " + tag,
               np.max(np.abs(fit.covariance[b] - t["covariance"])) / np.max(np.abs(t["covariance"])), REL, b)
        within("log det G vs truth / (1 + |log det G|): " + tag,
               abs(fit.logdet_gram[b] - t["logdet_gram"]) / (1 + abs(t["logdet_gram"])), REL, b)
        within("profiled quadratic form vs truth / (1 + |quad|): " + tag,
               abs(fit.quad[b] - t["quad"]) / (1 + abs(t["quad"])), REL, b)
        assert np.array_equal(fit.gram[b], fit.gram[b].T) and np.array_equal(fit.covariance[b], fit.covariance[b].T)
        assert fit.gram.shape[1:] == (K + 1, K + 1)


def _small_solve_alone(fit, w0, tag):
    """The device's small solve against the long-double Cholesky of ITS OWN Gram matrix at the forward bound of the solve,
    and against clr_gram_solve of the same matrix bit for bit."""
    B, K = w0.shape
    for b in range(B):
        t = ld_fit(fit.gram[b], w0[b])
        bound = small_solve_bound(K, t["kappa_s"])
        err = small_solve_errors(t, fit.weights[b], fit.covariance[b], fit.logdet_gram[b], fit.quad[b])
        for name, e in sorted(err.items()):
            within("small solve, %s vs long double, in units of (3 K + 1) 2^-52 kappa_2(G_s): %s" % (name, tag), e / bound, 1.0, b)
    w, cov, quad, ld, st = batch.gram_solve(fit.gram, w0)
    for name, host in (("weights", w), ("covariance", cov), ("quad", quad), ("logdet_gram", ld), ("status", st)):
        assert np.array_equal(getattr(fit, name), host), (tag, name)


def _narrow_setup(layout):
    def setup(p):
        p.set_chunks(24)
        p.set_factor_layout(layout)
    return setup


# ---- 1. / 2. narrow plans against the truth, and the small solve alone -----------------------------------------------

@pytest.mark.parametrize("phi_kind", ["shared", "per"])
@pytest.mark.parametrize("layout", ["reference", "lean"])
@pytest.mark.parametrize("JR,JC", [(2, 1), (2, 3)])
def test_fit_on_narrow_plans_against_binary128(JR, JC, layout, phi_kind):
    """B = 3, N = 3000 in 24 chunks (a ragged last chunk, one ragged slab of the Gram pass), K = 4, both factor layouts,
    the basis shared and per problem.  Largest deviations seen on an MI355X over the eight cases, against the binary128
    truth: a Gram entry 3.6e-15 (1 + max |R_j| sum |Z_k|), the weights 1.1e-14 (1 + |w|), the covariance 1.5e-15 max |cov|,
    log det G 6.1e-15, the profiled quadratic form 1.0e-14 (1 + |quad|).  The small solve alone, against the long-double
    Cholesky of the device's own Gram matrix: 0.13 of its forward bound (the covariance), and the bits of
    clr_gram_solve."""
    B, N, K = 3, 3000, 4
    case = synthetic(B, N, JR, JC, "bench", seed=91)
    y, Phi, w0, r = _inputs(case, B, K, phi_kind)
    fit, ev, chunks = _fitted(case, B, N, JR, JC, Phi, w0, _narrow_setup(layout), then=lambda p, f: p.chunks)
    nchunk, L = chunks
    assert N % L != 0 and nchunk > 1 and N % 4096 != 0 and (ev[3] == 0).all()
    _against_truth(fit, _truth(case, (JR, JC, N, K, phi_kind), Phi, w0, r), "narrow")
    _small_solve_alone(fit, w0, "narrow")
    # the likelihoods are the formulas of the header on the evaluation's log det K
    ll = -0.5 * (fit.quad + ev[1] + N * np.log(2 * np.pi))
    assert np.array_equal(fit.loglike, ll)
    assert np.array_equal(fit.loglike_marginal, ll - 0.5 * fit.logdet_gram + 0.5 * K * np.log(2 * np.pi))


# ---- 3. wide plans ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("phi_kind", ["shared", "per"])
@pytest.mark.parametrize("N", [2047, 6000])
def test_fit_on_a_wide_plan_against_binary128(N, phi_kind):
    """Width 12: the wave-per-chunk sweeps on the reference's storage, K = 3; N = 6000 is two slabs of the Gram pass, the
    second ragged.  Largest deviations seen on an MI355X over the four cases: a Gram entry 2.1e-15, the weights 1.6e-14, the
    covariance 3.1e-15, log det G 7.2e-15, the profiled quadratic form 1.1e-14 (scales as above); the small solve alone
    0.24 of its forward bound (the weights)."""
    B, JR, JC, K = 3, 4, 4, 3
    case = synthetic(B, N, JR, JC, "bench", seed=91)
    y, Phi, w0, r = _inputs(case, B, K, phi_kind)
    fit, ev, _ = _fitted(case, B, N, JR, JC, Phi, w0)
    assert N % 4096 != 0 and (ev[3] == 0).all()
    _against_truth(fit, _truth(case, (JR, JC, N, K, phi_kind), Phi, w0, r), "wide")
    _small_solve_alone(fit, w0, "wide")


# ---- 4. it is the optimum ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC", [(2, 3), (4, 4)])
def test_the_fit_is_the_optimum(JR, JC):
    """After fit_mean_weights(apply=True): the weight gradient vanishes, the evaluation returns MeanFit.loglike, every
    perturbation of the weights lowers the log-likelihood, and a second fit stays put.  Seen on an MI355X (narrow, wide):
    the gradient 9.9e-16, 5.3e-16 (1 + sum |K^-1 r|); quad 1.1e-15, 1.1e-15 (1 + |quad|), loglike the same bits; the
    second fit moves the weights by 0.86, 0.44 of the small solve's forward bound."""
    B, N, K = 3, 3000, 4
    case = synthetic(B, N, JR, JC, "bench", seed=93)
    y, Phi, w0, _ = _inputs(case, B, K, "per", seed=9)
    tag = "narrow" if JR + 2 * JC <= 8 else "wide"
    rng = np.random.RandomState(17)

    def then(plan, fit):
        dw, gst = plan.grad_mean_weights()
        x = plan.solve()
        ev = plan.log_likelihood(True)
        worse = []
        for _ in range(3):
            plan.set_mean_weights(fit.weights + 1e-3 * rng.uniform(-1, 1, (B, K)))
            worse.append(plan.log_likelihood(True)[0])
        plan.set_mean_weights(fit.weights)
        plan.log_likelihood(True)
        return dw, gst, x, ev, worse, plan.fit_mean_weights()

    fit, _, (dw, gst, x, ev, worse, again) = _fitted(case, B, N, JR, JC, Phi, w0, apply=True, then=then)
    assert (fit.status == 0).all() and (gst == 0).all() and (again.status == 0).all()
    for b in range(B):
        within("weight gradient at the fitted weights / (1 + sum |K^-1 r|): " + tag,
               np.max(np.abs(dw[b])) / (1 + np.sum(np.abs(x[b]))), REL, b)
        within("quad of the evaluation at the fitted weights vs the profiled one / (1 + |quad|): " + tag,
               abs(ev[2][b] - fit.quad[b]) / (1 + abs(fit.quad[b])), REL, b)
        within("loglike of the evaluation at the fitted weights vs MeanFit.loglike / (1 + |quad|): " + tag,
               abs(ev[0][b] - fit.loglike[b]) / (1 + abs(fit.quad[b])), REL, b)
        for ll in worse:
            assert ll[b] < ev[0][b], (b, ll[b], ev[0][b])
        kappa = ld_fit(again.gram[b], fit.weights[b])["kappa_s"]
        within("a second fit from the fitted weights moves them, in units of (3 K + 1) 2^-52 kappa_2(G_s): " + tag,
               np.max(np.abs(again.weights[b] - fit.weights[b]) / (1 + np.abs(fit.weights[b]))) / small_solve_bound(K, kappa),
               1.0, b)


# ---- 5. start weights -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC", [(2, 3), (4, 4)])
def test_the_fit_does_not_depend_on_the_start_weights(JR, JC):
    """From zero and from random start weights: 5.0e-15 (1 + |w|) apart at most on an MI355X."""
    B, N, K = 3, 3000, 4
    case = synthetic(B, N, JR, JC, "bench", seed=95)
    y, Phi, w0, _ = _inputs(case, B, K, "shared", seed=11)
    a, _, _ = _fitted(case, B, N, JR, JC, Phi, w0)
    z, _, _ = _fitted(case, B, N, JR, JC, Phi, np.zeros((B, K)))
    assert (a.status == 0).all() and (z.status == 0).all()
    for b in range(B):
        within("fitted weights from random vs from zero start weights / (1 + |w|)",
               np.max(np.abs(a.weights[b] - z.weights[b]) / (1 + np.abs(z.weights[b]))), REL, (JR, JC, b))
    assert np.array_equal(a.gram[:, :K, :K], z.gram[:, :K, :K])       # (G does not depend on the residual)


# ---- 6. K = 1, Phi = 1: the generalised weighted mean -----------------------------------------------------------------

@pytest.mark.parametrize("phi_kind", ["shared", "per"])
def test_one_basis_function_of_ones_gives_the_generalised_mean(phi_kind):
    """w = 1^T K^-1 y / 1^T K^-1 1 from the batched solve of a plan without a mean: 2.5e-16 (1 + |w|) apart at most on an
    MI355X."""
    B, N, JR, JC = 3, 3000, 2, 3
    case = synthetic(B, N, JR, JC, "bench", seed=97)
    ones = np.ones((1, N)) if phi_kind == "shared" else np.ones((B, 1, N))
    fit, _, _ = _fitted(case, B, N, JR, JC, ones, np.zeros((B, 1)))
    plain = _plan(case, B, N, JR, JC, case["y"])
    try:
        plain.log_likelihood(True)
        x = plain.solve(np.stack([np.ones((B, N)), case["y"]], axis=1))     # K^-1 1, K^-1 y
    finally:
        plain.close()
    assert (fit.status == 0).all() and fit.weights.shape == (B, 1)
    for b in range(B):
        mean = np.sum(x[b, 1].astype(LD)) / np.sum(x[b, 0].astype(LD))
        within("K = 1, Phi = 1: the weight vs 1^T K^-1 y / 1^T K^-1 1 / (1 + |w|)",
               abs(fit.weights[b, 0] - mean) / (1 + abs(mean)), REL, b)


# ---- 7. the tile ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC", [(2, 3), (4, 4)])
def test_results_do_not_depend_on_the_tile(JR, JC):
    """K = 4: five right-hand sides, in tiles of 1, of 2 (a ragged last tile) and all at once."""
    B, N, K = 3, 3000, 4
    case = synthetic(B, N, JR, JC, "bench", seed=99)
    y, Phi, w0, _ = _inputs(case, B, K, "per", seed=13)
    fits = [_fitted(case, B, N, JR, JC, Phi, w0, setup=lambda p, t=tile: p.set_mean_fit_tile(t),
                    then=lambda p, f: p.mean_fit_ms())[::2] for tile in (0, 1, 2)]
    assert (fits[0][0].status == 0).all()
    for (f, ms), tile in zip(fits[1:], (1, 2)):
        _same_fit(f, fits[0][0], ("tile", tile))
        assert len(ms) == 3 and all(m >= 0.0 for m in ms) and ms[0] > 0.0


# ---- 8. K = 16 -------------------------------------------------------------------------------------------------------

def test_sixteen_basis_functions():
    """K = 16 on width 4: the widest instantiation of the Gram pass, 17 right-hand sides.  No binary128 truth here (the
    small solve alone, and the gradient at the fit).  Seen on an MI355X: the small solve 0.045 of its forward bound (the
    weights), the gradient at the fitted weights 1.3e-13 (1 + sum |K^-1 r|)."""
    B, N, JR, JC, K = 2, 3000, 2, 1, 16
    case = synthetic(B, N, JR, JC, "bench", seed=101)
    y, Phi, w0, _ = _inputs(case, B, K, "per", seed=15)

    def then(plan, fit):
        dw, gst = plan.grad_mean_weights()
        return dw, gst, plan.solve()

    fit, _, (dw, gst, x) = _fitted(case, B, N, JR, JC, Phi, w0, apply=True, then=then)
    assert (fit.status == 0).all() and (gst == 0).all()
    _small_solve_alone(fit, w0, "K = 16")
    for b in range(B):
        assert ld_fit(fit.gram[b], w0[b])["kappa_s"] <= 2.0
        within("weight gradient at the fitted weights / (1 + sum |K^-1 r|): K = 16",
               np.max(np.abs(dw[b])) / (1 + np.sum(np.abs(x[b]))), REL, b)


# ---- 9. rank deficiency ------------------------------------------------------------------------------------------------

def test_a_rank_deficient_basis_is_refused_per_problem():
    B, N, JR, JC = 3, 3000, 2, 1
    case = synthetic(B, N, JR, JC, "bench", seed=103)
    # sin 0.3 t = 0.3 t on [0, 1] to 5e-3, and 16 functions of it: the Gram matrix is numerically singular
    K = 16
    w0 = np.random.RandomState(19).uniform(-1.5, 1.5, (B, K))
    fit, _, _ = _fitted(case, B, N, JR, JC, basis_of(case["t"], K), w0)
    assert (fit.status == batch.CLR_NOT_POSITIVE_DEFINITE).all()
    assert np.isfinite(fit.gram).all() and np.isnan(fit.covariance).all() and np.isnan(fit.quad).all()
    assert np.isnan(fit.logdet_gram).all() and np.isnan(fit.loglike).all() and np.isnan(fit.loglike_marginal).all()
    assert np.array_equal(fit.weights, w0)
    # only problem 1 has a duplicated row
    K = 4
    y, Phi, w0, _ = _inputs(case, B, K, "per", seed=21)
    dup = Phi.copy()
    dup[1, 2] = dup[1, 0]
    weights_after = lambda p, f: p._mean_w.copy()
    clean, _, w_clean = _fitted(case, B, N, JR, JC, Phi, w0, apply=True, then=weights_after)
    bad, _, w_bad = _fitted(case, B, N, JR, JC, dup, w0, apply=True, then=weights_after)
    assert clean.status.tolist() == [0, 0, 0] and bad.status.tolist() == [0, batch.CLR_NOT_POSITIVE_DEFINITE, 0]
    _same_fit(bad, clean, "a refused neighbour", rows=[0, 2])
    assert np.isfinite(bad.gram[1]).all() and np.isnan(bad.covariance[1]).all() and np.isnan(bad.quad[1])
    assert np.array_equal(w_bad[1], w0[1]) and np.array_equal(w_bad[[0, 2]], clean.weights[[0, 2]])
    assert np.array_equal(w_clean, clean.weights)


# ---- 10. a problem without a factor ---------------------------------------------------------------------------------

def test_an_indefinite_problem_keeps_its_status_and_disturbs_no_other():
    B, N, JR, JC, K = 5, 4000, 2, 3, 3
    good = synthetic(B, N, JR, JC, "bench", seed=111)
    bad = dict(good, a_real=good["a_real"].copy())
    bad["a_real"][2] *= -40.0                        # not positive definite
    y, Phi, w0, _ = _inputs(good, B, K, "per", seed=4)
    f0, ev0, _ = _fitted(good, B, N, JR, JC, Phi, w0)
    f1, ev1, _ = _fitted(bad, B, N, JR, JC, Phi, w0)
    assert (f0.status == 0).all() and np.array_equal(f1.status, ev1[3])
    assert f1.status[2] == batch.CLR_NOT_POSITIVE_DEFINITE and (np.delete(f1.status, 2) == 0).all()
    assert np.array_equal(f1.weights[2], w0[2])
    for name in ("covariance", "gram", "quad", "logdet_gram", "loglike", "loglike_marginal"):
        assert np.isnan(getattr(f1, name)[2]).all(), name
    _same_fit(f1, f0, "an indefinite neighbour", rows=[0, 1, 3, 4])


# ---- 11. new weights, the same factor ----------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC", [(2, 3), (4, 4)])
def test_new_weights_need_no_new_materialising_run(JR, JC):
    B, N, K = 3, 3000, 3
    case = synthetic(B, N, JR, JC, "bench", seed=113)
    y, Phi, w1, _ = _inputs(case, B, K, "shared", seed=1)
    w2 = np.random.RandomState(8).uniform(-1.5, 1.5, (B, K))

    def then(plan, fit):
        plan.set_mean_weights(w2)                    # the factor does not depend on y
        return plan.fit_mean_weights()

    first, _, second = _fitted(case, B, N, JR, JC, Phi, w1, then=then)
    fresh, _, _ = _fitted(case, B, N, JR, JC, Phi, w2)
    assert not np.array_equal(first.gram, second.gram)
    _same_fit(second, fresh, "new weights on the old factor")


# ---- 12. sharding ------------------------------------------------------------------------------------------------------

def test_sharded_fit_matches_the_single_plan():
    """Two shards on one device (one chunk count for both, as bit identity under sharding asks)."""
    B, N, JR, JC, K = 5, 5000, 2, 1, 3
    case = synthetic(B, N, JR, JC, "bench", seed=141)
    y, Phi, w0, _ = _inputs(case, B, K, "per", seed=7)
    single = _plan(case, B, N, JR, JC, y, setup=lambda p: p.set_chunks(40))
    sh = batch.ShardedBatchedGP(B, N, JR, JC, devices=[0, 0])
    try:
        sh.set_chunks(40)
        sh.set_series(case["t"], case["diag"], y)
        sh.set_coefficients(*coeffs_of(case))
        for plan in (single, sh):
            plan.set_mean_basis(Phi)
            plan.set_mean_weights(w0)
        single.log_likelihood(True)
        sh.materialize()
        a = single.fit_mean_weights(apply=True)
        b = sh.fit_mean_weights(apply=True)
        _same_fit(b, a, "sharded")
        assert (a.status == 0).all() and np.isfinite(a.loglike_marginal).all()
        for x, z in zip(sh.log_likelihood(), single.log_likelihood()):
            assert np.array_equal(x, z)
    finally:
        sh.close()
        single.close()


# ---- 13. refusals --------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_plan_as_it_was():
    B, N, JR, JC, K = 3, 3000, 2, 3, 3
    case = synthetic(B, N, JR, JC, "bench", seed=131)
    y, Phi, w0, _ = _inputs(case, B, K, "shared", seed=6)
    lib = batch._load()
    plan = _plan(case, B, N, JR, JC, y)

    def same(base, what):
        for x, z in zip(plan.log_likelihood(True), base):
            assert np.array_equal(x, z), what

    def raw(min_pivot=1e-10):
        return lib.clr_batch_fit_mean_weights(plan._h, min_pivot, None, None, None, None, None, None)

    try:
        base = plan.log_likelihood(True)
        with pytest.raises(RuntimeError, match="no basis"):                 # no basis
            plan.fit_mean_weights()
        assert raw() == batch.CLR_INVALID_ARGUMENT
        same(base, "no basis")
        plan.set_mean(0.3)                                                  # a constant mean in force
        kept = plan.log_likelihood(True)
        with pytest.raises(RuntimeError, match="no basis"):
            plan.fit_mean_weights()
        assert raw() == batch.CLR_INVALID_ARGUMENT and b"constant mean" in lib.clr_last_error()
        same(kept, "constant mean")
        plan.set_mean(None)
        plan.set_mean_basis(Phi)
        plan.set_mean_weights(w0)
        fresh = _plan(case, B, N, JR, JC, y)                                # a plan that never materialised
        try:
            fresh.set_mean_basis(Phi)
            fresh.set_mean_weights(w0)
            kept_fresh = fresh.log_likelihood()
            with pytest.raises(RuntimeError, match="materialising"):
                fresh.fit_mean_weights()
            for x, z in zip(fresh.log_likelihood(), kept_fresh):
                assert np.array_equal(x, z)
        finally:
            fresh.close()
        kept = plan.log_likelihood(True)
        for bad in (np.nan, -1.0, 1.0):
            with pytest.raises(ValueError, match="min_pivot"):
                plan.fit_mean_weights(min_pivot=bad)
            assert raw(bad) == batch.CLR_INVALID_ARGUMENT
            same(kept, ("min_pivot", bad))
        # all outputs null is a valid call, and the weights in force stay
        assert raw() == batch.CLR_OK
        same(kept, "after a fit")
        fit = plan.fit_mean_weights()
        assert (fit.status == 0).all() and not np.array_equal(fit.weights, w0)
        same(kept, "the C call does not change the weights in force")
    finally:
        plan.close()
