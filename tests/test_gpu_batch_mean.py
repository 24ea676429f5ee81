# -*- coding: utf-8 -*-
"""A constant mean per problem on batched plans (clr_batch_set_mean / _evaluate_mean / _grad_mean and their sharded
twins).  The residual y - mu is formed on the device by the same IEEE subtraction a caller would do on the host, so
every route must give the SAME BITS as a plan whose series was host-subtracted; the mean's partial 1^T K^-1 r is held
against the binary128 solve of the oracle (oracle.ref.quad_factor_solve)."""
import numpy as np
import pytest

from celerite_amd import batch
from oracle import ref
from _cases import adversarial, coeffs_of, general_terms, synthetic, within

pytestmark = pytest.mark.gpu

REL = 1e-10
Y_MU = [("shared", "scalar"), ("shared", "per"), ("per", "scalar"), ("per", "per")]


def _series_and_mean(case, B, y_kind, mu_kind, seed=0):
    rng = np.random.RandomState(seed)
    y = case["y"] if y_kind == "per" else case["y"][0]
    mu = 0.37 if mu_kind == "scalar" else rng.uniform(-1.0, 1.0, B)
    m = np.asarray(mu, dtype=np.float64)
    if m.ndim == 0:
        r = y - m
    elif y.ndim == 1:
        r = y[None, :] - m[:, None]
    else:
        r = y - m[:, None]
    return y, mu, r


def _plan(case, B, N, JR, JC, y, setup=None, general=None):
    plan = batch.BatchedGP(B, N, JR, JC)
    if setup:
        setup(plan)
    if general is not None:
        plan.set_general(*general)
    plan.set_series(case["t"], case["diag"], y)
    plan.set_coefficients(*coeffs_of(case))
    return plan


def _same(a, b, what):
    for x, z, name in zip(a, b, ("loglike", "logdet", "quad", "status")):
        assert np.array_equal(np.asarray(x), np.asarray(z), equal_nan=(name != "status")), (what, name, x, z)


def _bit_identity(case, B, N, JR, JC, y_kind, mu_kind, setup=None, general=None, materialize=False, mean_first=False,
                  check=None):
    """set_mean(mu) on the uploaded y against set_series(y - mu) on the host: loglike, logdet, quad and status equal."""
    y, mu, r = _series_and_mean(case, B, y_kind, mu_kind)
    a = batch.BatchedGP(B, N, JR, JC)
    b = _plan(case, B, N, JR, JC, r, setup, general)
    try:
        if setup:
            setup(a)
        if general is not None:
            a.set_general(*general)
        if mean_first:              # the mean set before the series: set_series applies it
            a.set_mean(mu)
            a.set_series(case["t"], case["diag"], y)
        else:
            a.set_series(case["t"], case["diag"], y)
            a.set_mean(mu)
        a.set_coefficients(*coeffs_of(case))
        ra = a.log_likelihood(materialize)
        rb = b.log_likelihood(materialize)
        _same(ra, rb, (JR, JC, y_kind, mu_kind))
        if check:
            check(a, b, mu)
        return ra
    finally:
        a.close()
        b.close()


NARROW = [(1, 0), (0, 1), (2, 1), (3, 1), (2, 2), (1, 3), (0, 4), (2, 3)]


@pytest.mark.parametrize("y_kind,mu_kind", Y_MU)
@pytest.mark.parametrize("JR,JC", NARROW)
def test_narrow_plan_mean_is_bit_identical_to_host_subtraction(JR, JC, y_kind, mu_kind):
    B, N = 8, 4000
    case = synthetic(B, N, JR, JC, "bench", seed=11 + JR + 7 * JC)
    _bit_identity(case, B, N, JR, JC, y_kind, mu_kind, mean_first=(JR + JC) % 2 == 0)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("JR,JC", [(1, 3), (2, 3), (0, 4)])
def test_split_summarize_widths_7_8_with_a_mean(JR, JC, mode):
    """Widths 7 / 8: the single-wave kernel (0) and the role split reading the chunk-interleaved copy (1, 2): a new
    mean on an unchanged series rebuilds the copy of y alone."""
    B, N = 16, 20000
    case = synthetic(B, N, JR, JC, "bench", seed=31)
    for y_kind, mu_kind in Y_MU:
        _bit_identity(case, B, N, JR, JC, y_kind, mu_kind, setup=lambda p: p.set_summarize_mode(mode))
    # a second mean on the same plan: the interleaved copy follows
    y, mu, r = _series_and_mean(case, B, "shared", "per", seed=5)
    a = _plan(case, B, N, JR, JC, y, setup=lambda p: p.set_summarize_mode(mode))
    b = _plan(case, B, N, JR, JC, r, setup=lambda p: p.set_summarize_mode(mode))
    try:
        a.set_mean(0.5)
        a.log_likelihood()
        a.set_mean(mu)
        _same(a.log_likelihood(), b.log_likelihood(), mode)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("JR,JC", [(1, 0), (2, 1), (0, 2)])
def test_one_launch_small_mode_with_a_mean(JR, JC):
    B, N = 4, 2000
    case = synthetic(B, N, JR, JC, "bench", seed=41)

    def setup(p):
        p.set_small_mode(1)

    for y_kind, mu_kind in Y_MU:
        _bit_identity(case, B, N, JR, JC, y_kind, mu_kind, setup=setup,
                      check=lambda a, b, mu: a.small_mode_active() or pytest.fail("one-launch mode not taken"))


def test_warm_start_with_a_mean():
    B, N, JR, JC = 9, 12000, 2, 3
    case = synthetic(B, N, JR, JC, "accuracy", seed=77)

    def check(a, b, mu):
        assert a.warm_start()["active"] == 1 and b.warm_start()["active"] == 1

    for y_kind, mu_kind in Y_MU:
        _bit_identity(case, B, N, JR, JC, y_kind, mu_kind, setup=lambda p: p.set_warm_start(1, 128), check=check)


@pytest.mark.parametrize("JR,JC", [(4, 4), (1, 10), (0, 20), (1, 31)])
def test_wide_plans_with_a_mean(JR, JC):
    B, N = 4, 6000
    case = synthetic(B, N, JR, JC, "bench", seed=51)
    for y_kind, mu_kind in Y_MU:
        _bit_identity(case, B, N, JR, JC, y_kind, mu_kind)


@pytest.mark.parametrize("JR,JC,N", [(2, 3, 3000), (1, 30, 600)])
def test_general_term_plans_with_a_mean(JR, JC, N):
    """General terms through the wide kernels (total width 12) and through the any-width kernel (total width 65)."""
    B = 3
    case = synthetic(B, N, JR, JC, "bench", seed=61)
    t = case["t"][0]
    case["t"] = t
    A, U, V = general_terms(t, np.random.RandomState(3).rand)
    for y_kind, mu_kind in Y_MU:
        _bit_identity(case, B, N, JR, JC, y_kind, mu_kind, general=(A, U, V))


def test_route1_problems_on_the_side_plan_see_the_residual():
    """Problems re-planned on a side plan (clr_batch_set_rescue) copy the plan's series: the residual."""
    B, N, JR, JC = 24, 40000, 2, 3
    case = synthetic(B, N, JR, JC, "bench", seed=515)
    for y_kind, mu_kind in (("per", "per"), ("shared", "per")):
        y, mu, r = _series_and_mean(case, B, y_kind, mu_kind)
        a = _plan(case, B, N, JR, JC, y, setup=lambda p: p.set_chunks(32))
        b = _plan(case, B, N, JR, JC, r, setup=lambda p: p.set_chunks(32))
        try:
            a.set_mean(mu)
            b.log_likelihood()
            gamma, _ = b.conditioning()
            order = np.argsort(gamma)[::-1]
            bound = 0.5 * (gamma[order[1]] + gamma[order[2]])
            for p in (a, b):
                p.set_certificate(max_gamma=bound)
                p.set_coefficients(*coeffs_of(case))
            ra, rb = a.log_likelihood(), b.log_likelihood()
            assert a.rescue()["last"] == 2 and b.rescue()["last"] == 2, (a.rescue(), b.rescue())
            _same(ra, rb, y_kind)
        finally:
            a.close()
            b.close()


@pytest.mark.parametrize("JR,JC", [(2, 3), (4, 4)])
def test_materialising_run_solve_and_predict_with_a_mean(JR, JC):
    """A materialising run gives the same bits; solve(None) solves the residual; predict is mu_b + the prediction of
    the residual (GP.predict, celerite.py:279)."""
    B, N = 6, 4000
    case = synthetic(B, N, JR, JC, "bench", seed=71)
    xs = np.linspace(0.05, 0.95, 37)

    def check(a, b, mu):
        assert np.array_equal(a.solve(), b.solve())
        m = np.broadcast_to(np.asarray(mu, dtype=np.float64), (B,))
        assert np.array_equal(a.predict(xs), m[:, None] + b.predict(xs))

    for y_kind, mu_kind in Y_MU:
        _bit_identity(case, B, N, JR, JC, y_kind, mu_kind, materialize=True, check=check)


def test_neutral_settings_and_the_one_call_evaluation():
    B, N, JR, JC = 8, 5000, 2, 3
    case = synthetic(B, N, JR, JC, "bench", seed=81)
    mu = np.random.RandomState(2).uniform(-1, 1, B)
    plan = _plan(case, B, N, JR, JC, case["y"][0])
    try:
        base = plan.log_likelihood()
        plan.set_mean(0.0)
        _same(plan.log_likelihood(), base, "mean 0")
        plan.set_mean(mu)
        with_mean = plan.log_likelihood()
        assert not np.array_equal(with_mean[2], base[2])
        plan.set_mean(None)
        _same(plan.log_likelihood(), base, "mean removed")
        # the one-call form equals set_mean + enqueue, and leaves the mean in force
        one = plan.evaluate(*coeffs_of(case), mean=mu)
        _same(one, with_mean, "evaluate(mean=)")
        _same(plan.evaluate(*coeffs_of(case)), with_mean, "mean kept")
        # set_series after set_mean keeps the mean and applies it to the new series
        y2 = case["y"] * 0.5
        plan.set_series(case["t"], case["diag"], y2)
        ref_plan = _plan(case, B, N, JR, JC, y2 - mu[:, None])
        try:
            _same(plan.log_likelihood(), ref_plan.log_likelihood(), "new series")
        finally:
            ref_plan.close()
        # a non-finite mean is refused and the plan keeps the mean it had
        kept = plan.log_likelihood()
        bad = mu.copy()
        bad[3] = np.nan
        with pytest.raises(Exception):
            plan.set_mean(bad)
        with pytest.raises(Exception):
            plan.set_mean(np.inf)
        _same(plan.log_likelihood(), kept, "after a refused mean")
    finally:
        plan.close()


def _kernel_draws(B, seed):
    from celerite_amd import terms

    kernel = terms.RealTerm(0.1, 0.5) + terms.ComplexTerm(0.6, 0.2, 1.0, 1.2)
    rng = np.random.RandomState(seed)
    draws = kernel.get_parameter_vector()[None, :] + 0.05 * rng.randn(B, kernel.vector_size)
    return kernel, draws


def test_against_the_object_api_and_the_oracle():
    """16 problems against GP(kernel, mean=mu_b, fit_mean=True): log-likelihood and the full chained gradient
    (kernel parameters, then the mean); and against the CPU oracle on y - mu_b."""
    from celerite_amd import GP

    B, N = 16, 3000
    kernel, draws = _kernel_draws(B, 4)
    rng = np.random.RandomState(9)
    t = np.sort(rng.uniform(0, 100, N))
    yerr = rng.uniform(0.1, 0.3, N)
    y = np.sin(t) + 0.4 + yerr * rng.randn(N)
    mu = rng.uniform(0.0, 0.8, B)
    tab = batch.kernel_coefficient_table(kernel, draws)
    plan = batch.BatchedGP(B, N, 1, 1)
    try:
        plan.set_series(t, yerr ** 2, y)
        plan.set_mean(mu)
        plan.set_coefficients(*tab[:6], jitter=tab[6])
        ll, ld, q, st = plan.log_likelihood()
        value, grad, dmean, gst = plan.grad_log_likelihood(mean_partial=True)
    finally:
        plan.close()
    assert (st == 0).all() and (gst == 0).all()
    g = batch.chain_gradient(grad, *batch.kernel_coefficient_jacobian_table(kernel, draws), dmean=dmean)
    r = y[None, :] - mu[:, None]
    l0, d0, q0, s0 = ref.batch_log_likelihood(tab[6], *tab[:6], t, yerr ** 2, r)
    assert np.array_equal(st, s0)
    within("batched mean: log det vs oracle on y - mu", np.max(np.abs(ld - d0) / np.abs(d0)), REL)
    within("batched mean: quadratic form vs oracle on y - mu", np.max(np.abs(q - q0) / np.abs(q0)), REL)
    for b in range(B):
        kernel.set_parameter_vector(draws[b])
        gp = GP(kernel, mean=mu[b], fit_mean=True)
        gp.compute(t, yerr)
        l_obj = gp.log_likelihood(y)
        within("batched mean: log-likelihood vs GP(mean=mu_b, fit_mean=True)", abs(ll[b] - l_obj) / abs(l_obj), REL, b)
        v_obj, g_obj = gp.grad_log_likelihood(y)
        assert g.shape[1] == len(g_obj)
        within("batched mean: chained gradient vs GP(...fit_mean=True).grad_log_likelihood (of the largest)",
               np.max(np.abs(g[b] - g_obj)) / np.max(np.abs(g_obj)), 1e-9, b)
        within("batched mean: gradient value vs GP(...fit_mean=True)", abs(value[b] - v_obj) / abs(v_obj), REL, b)


def _mean_partial_truth(case, b, r_b):
    co = tuple(c[b] for c in coeffs_of(case))
    t = case["t"][b] if case["t"].ndim == 2 else case["t"]
    diag = case["diag"][b] if case["diag"].ndim == 2 else case["diag"]
    x = ref.quad_factor_solve(0.0, *co, t, diag, r_b, want_factor=False)[2]
    s = ref.RefSolver()
    s.compute(0.0, *co, np.empty(0), np.empty((0, 0)), np.empty((0, 0)), t, diag)
    xd = np.asarray(s.solve(r_b)).ravel()
    return float(np.sum(x)), float(np.sum(np.abs(x))), float(np.sum(xd))


ROUTES = {
    "narrow reverse": dict(JR=2, JC=3, B=6, N=6000, setup=None),
    "narrow reverse, long series": dict(JR=2, JC=3, B=2, N=100000, setup=None),
    "narrow reverse, every problem redone forwards": dict(
        JR=2, JC=3, B=6, N=6000, setup=lambda p: p.set_grad_mode("reverse", 0, 1e-300)),
    "narrow forward": dict(JR=2, JC=3, B=6, N=6000, setup=lambda p: p.set_grad_mode("forward")),
    "wide 9..32": dict(JR=4, JC=4, B=3, N=6000, setup=None),
    "wide 33..64 chunked": dict(JR=0, JC=20, B=2, N=8000, setup=None),
    "wide 33..64 one chunk": dict(JR=0, JC=20, B=2, N=3000, setup=lambda p: p.set_chunks(1)),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_mean_partial_on_every_gradient_route_against_binary128(route):
    """dmean = 1^T K^-1 r against the binary128 solve; the coefficient partials of clr_batch_grad_mean equal those of
    clr_batch_grad on the host-subtracted series, bit for bit.  On the narrow reverse route the partial is half the sum
    of the sweep's adjoint of y; forward mode, the wide routes and problems the sweep hands to forward mode take the
    sequential recurrence with the substitution of the ones."""
    cfg = ROUTES[route]
    JR, JC, B, N = cfg["JR"], cfg["JC"], cfg["B"], cfg["N"]
    case = synthetic(B, N, JR, JC, "bench", seed=91)
    y, mu, r = _series_and_mean(case, B, "per", "per", seed=3)
    a = _plan(case, B, N, JR, JC, y, cfg["setup"])
    b = _plan(case, B, N, JR, JC, r, cfg["setup"])
    try:
        a.set_mean(mu)
        va, ga, dm, sa = a.grad_log_likelihood(mean_partial=True)
        info = a.grad_info()
        vb, gb, sb = b.grad_log_likelihood()
    finally:
        a.close()
        b.close()
    assert np.array_equal(sa, sb) and (sa == 0).all()
    assert np.array_equal(va, vb) and np.array_equal(ga, gb)
    if route.startswith("narrow reverse"):
        assert info["reverse"]
        assert (info["forward_reruns"] >= 1) == route.endswith("forwards"), info
    for p in range(B):
        truth, scale, twin = _mean_partial_truth(case, p, r[p])
        within("mean partial vs binary128 / (1 + sum |K^-1 r|): " + route, abs(dm[p] - truth) / (1 + scale), 1e-10, p)
        within("mean partial, double oracle vs binary128 / (1 + sum |K^-1 r|)", abs(twin - truth) / (1 + scale), 1e-8, p)


def test_mean_partial_on_level2_problems_against_binary128():
    """Problems the evaluation settles sequentially (level 2; ill-conditioned): bar 1e-10 (1 + sum |K^-1 r|) or 100 x
    the double oracle's distance from the truth, whichever is larger (test_gpu_grad_truth.py's rule)."""
    JR, JC = 2, 3
    seen = 0
    for trial in range(6):
        B, N = 6, 3000
        case = adversarial(B, N, JR, JC, seed=4000 + trial)
        mu = np.random.RandomState(trial).uniform(-1, 1, B)
        plan = batch.BatchedGP(B, N, JR, JC)
        try:
            plan.set_series(case["t"], case["diag"], case["y"])
            plan.set_mean(mu)
            plan.set_coefficients(*coeffs_of(case))
            v, g, dm, st = plan.grad_log_likelihood(mean_partial=True)
            levels = plan.exact_levels()
        finally:
            plan.close()
        assert (dm[st != 0] == 0).all()
        for b in np.nonzero((st == 0) & (levels >= 2))[0]:
            try:
                truth, scale, twin = _mean_partial_truth(case, b, case["y"][b] - mu[b])
            except ref.RefLinAlgError:
                continue
            bar = max(1e-10 * (1 + scale), 100 * abs(twin - truth))
            within("mean partial, level-2 problems: vs binary128 / max(1e-10 (1 + sum |K^-1 r|), 100 x double oracle)",
                   abs(dm[b] - truth) / bar, 1.0, (trial, b))
            seen += 1
    assert seen >= 1


def test_sharded_plan_with_a_mean_matches_the_single_plan():
    """Two shards (on the same device when there is one): set_mean, evaluate(mean=) and the gradient with the mean's
    partial give the same bits as the unsharded plan."""
    B, N, JR, JC = 10, 5000, 2, 3
    case = synthetic(B, N, JR, JC, "bench", seed=101)
    mu = np.random.RandomState(6).uniform(-1, 1, B)
    ndev = batch.device_count()
    single = _plan(case, B, N, JR, JC, case["y"][0])
    sh = batch.ShardedBatchedGP(B, N, JR, JC, devices=[s % ndev for s in range(2)])
    try:
        sh.set_series(case["t"], case["diag"], case["y"][0])
        sh.set_coefficients(*coeffs_of(case))
        for m in (mu, 0.25):
            single.set_mean(m)
            sh.set_mean(m)
            _same(sh.log_likelihood(), single.log_likelihood(), "sharded set_mean")
            _same(sh.evaluate(*coeffs_of(case), mean=m), single.evaluate(*coeffs_of(case), mean=m), "sharded evaluate")
            g1 = single.grad_log_likelihood(mean_partial=True)
            g2 = sh.grad_log_likelihood(mean_partial=True)
            for x, z in zip(g1, g2):
                assert np.array_equal(x, z)
        sh.set_mean(None)
        single.set_mean(None)
        _same(sh.log_likelihood(), single.log_likelihood(), "sharded, mean removed")
    finally:
        sh.close()
        single.close()


def test_mean_partial_reverse_sweep_against_the_sequential_recurrence():
    """The two layers of the partial on the same problems: half the sum of the reverse sweep's adjoint of y (default
    mode) against the recurrence carrying the substitution of the ones (forward mode) -- over all widths 1..8."""
    for JR, JC in NARROW:
        B, N = 6, 5000
        case = synthetic(B, N, JR, JC, "bench", seed=17 + JR + 5 * JC)
        mu = np.random.RandomState(JR + JC).uniform(-1, 1, B)
        plan = _plan(case, B, N, JR, JC, case["y"])
        try:
            plan.set_mean(mu)
            _, _, d_rev, st = plan.grad_log_likelihood(mean_partial=True)
            assert plan.grad_info()["reverse"] and plan.grad_fallbacks() == 0
            plan.set_grad_mode("forward")
            _, _, d_seq, st2 = plan.grad_log_likelihood(mean_partial=True)
        finally:
            plan.close()
        assert (st == 0).all() and (st2 == 0).all()
        within("mean partial: reverse sweep vs sequential recurrence (relative)",
               np.max(np.abs(d_rev - d_seq) / np.maximum(np.abs(d_seq), 1e-300)), 1e-10, (JR, JC))


@pytest.mark.parametrize("JR,JC", [(2, 3), (4, 4)])
def test_mean_partial_with_general_terms(JR, JC):
    """A plan with general terms (A, U, V read by the recurrence of the partial) against the CPU oracle's solve."""
    B, N = 3, 4000
    case = synthetic(B, N, JR, JC, "bench", seed=121)
    t = case["t"][0]
    case["t"] = t
    A, U, V = general_terms(t, np.random.RandomState(8).rand)
    mu = np.array([0.3, -0.2, 0.7])
    r = case["y"] - mu[:, None]
    a = _plan(case, B, N, JR, JC, case["y"], general=(A, U, V))
    b = _plan(case, B, N, JR, JC, r, general=(A, U, V))
    try:
        a.set_mean(mu)
        va, ga, dm, sa = a.grad_log_likelihood(mean_partial=True)
        vb, gb, sb = b.grad_log_likelihood()
    finally:
        a.close()
        b.close()
    assert (sa == 0).all() and np.array_equal(sa, sb) and np.array_equal(va, vb) and np.array_equal(ga, gb)
    for p in range(B):
        s = ref.RefSolver()
        s.compute(0.0, *(c[p] for c in coeffs_of(case)), A, U, V, t, case["diag"][p])
        x = np.asarray(s.solve(r[p])).ravel()
        within("mean partial, general terms: vs the oracle's solve / (1 + sum |K^-1 r|)",
               abs(dm[p] - np.sum(x)) / (1 + np.sum(np.abs(x))), 1e-10, p)
