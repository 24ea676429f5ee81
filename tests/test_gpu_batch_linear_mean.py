# -*- coding: utf-8 -*-
"""A mean that is linear in its parameters on batched plans (clr_batch_set_mean_basis / _set_mean_weights /
_grad_mean_weights and their sharded twins).  The residual y - sum_k w_k Phi_k is formed on the device in a fixed order
with every product and sum rounded on its own, so every route must give the SAME BITS as a plan whose series was
subtracted on the host by the same NumPy expression; the weight gradient Phi_k^T K^-1 r is held against the binary128
solve of the oracle (oracle.ref.quad_factor_solve) at the bar the constant mean's partial is held to."""
import numpy as np
import pytest

from celerite_amd import batch
from oracle import ref
from _cases import coeffs_of, synthetic, within

pytestmark = pytest.mark.gpu

REL = 1e-10                      # tests/test_gpu_batch_mean.py: |dmean - truth| / (1 + sum |K^-1 r|)
Y_PHI = [("shared", "shared"), ("shared", "per"), ("per", "shared"), ("per", "per")]


def basis_of(t, K):
    """``[1, t - mean(t), sin(0.3 t), cos(0.3 t), sin(0.6 t), ...]`` at the times ``t`` (..., N) -> (..., K, N); every
    entry but the trend's is at most 1 in magnitude, the trend is scaled to [-1, 1]."""
    t = np.asarray(t, dtype=np.float64)
    c = t - t.mean(axis=-1, keepdims=True)
    rows = [np.ones_like(t), c / np.max(np.abs(c)), np.sin(0.3 * t)]
    j = 1
    while len(rows) < K:
        rows.append(np.cos(0.3 * j * t))
        j += 1
        rows.append(np.sin(0.3 * j * t))
    return np.stack(rows[:K], axis=-2)


def host_model(w, Phi):
    B, K = w.shape
    P = np.broadcast_to(Phi, (B, K, Phi.shape[-1]))
    m = w[:, 0, None] * P[:, 0]
    for k in range(1, K):
        m = m + w[:, k, None] * P[:, k]
    return m


def host_residual(y, w, Phi):
    """The expression the device's residual is the bits of."""
    return y - host_model(w, Phi)


def _inputs(case, B, K, y_kind, phi_kind, seed=0):
    y = case["y"] if y_kind == "per" else case["y"][0]
    Phi = basis_of(case["t"], K) if phi_kind == "per" else basis_of(case["t"][0], K)
    w = np.random.RandomState(seed).uniform(-1.5, 1.5, (B, K))
    return y, Phi, w, host_residual(y, w, Phi)


def _plan(case, B, N, JR, JC, y, setup=None):
    plan = batch.BatchedGP(B, N, JR, JC)
    if setup:
        setup(plan)
    plan.set_series(case["t"], case["diag"], y)
    plan.set_coefficients(*coeffs_of(case))
    return plan


def _same(a, b, what):
    for x, z, name in zip(a, b, ("loglike", "logdet", "quad", "status")):
        assert np.array_equal(np.asarray(x), np.asarray(z), equal_nan=(name != "status")), (what, name, x, z)


def _bit_identity(case, B, N, JR, JC, K, y_kind, phi_kind, setup=None, materialize=False, basis_first=False, check=None):
    """set_mean_basis + set_mean_weights on the uploaded y against set_series(r) with r subtracted on the host."""
    y, Phi, w, r = _inputs(case, B, K, y_kind, phi_kind)
    a = batch.BatchedGP(B, N, JR, JC)
    b = _plan(case, B, N, JR, JC, r, setup)
    try:
        if setup:
            setup(a)
        if basis_first:             # basis and weights before the series: set_series applies them
            a.set_mean_basis(Phi)
            a.set_mean_weights(w)
            a.set_series(case["t"], case["diag"], y)
        else:
            a.set_series(case["t"], case["diag"], y)
            a.set_mean_basis(Phi)
            a.set_mean_weights(w)
        a.set_coefficients(*coeffs_of(case))
        ra = a.log_likelihood(materialize)
        rb = b.log_likelihood(materialize)
        _same(ra, rb, (JR, JC, K, y_kind, phi_kind))
        assert (ra[3] == 0).all()
        if check:
            check(a, b)
    finally:
        a.close()
        b.close()


# ---- 1. bit identity with the host's subtraction, on every route that reads y or a copy of it ----------------------

@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("JR,JC", [(1, 0), (2, 1), (2, 3)])
def test_narrow_plan_linear_mean_is_bit_identical_to_host_subtraction(JR, JC, K):
    B, N = 5, 4000
    case = synthetic(B, N, JR, JC, "bench", seed=11 + JR + 7 * JC)
    for i, (y_kind, phi_kind) in enumerate(Y_PHI):
        _bit_identity(case, B, N, JR, JC, K, y_kind, phi_kind, basis_first=(i + K) % 2 == 0)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("JR,JC", [(1, 3), (2, 3)])
def test_split_summarize_widths_7_8_with_a_linear_mean(JR, JC, mode):
    """The role split reads the chunk-interleaved copy of y: new weights on an unchanged series rebuild it."""
    B, N, K = 16, 20000, 3
    case = synthetic(B, N, JR, JC, "bench", seed=31)
    setup = lambda p: p.set_summarize_mode(mode)
    for y_kind, phi_kind in Y_PHI:
        _bit_identity(case, B, N, JR, JC, K, y_kind, phi_kind, setup=setup)
    # a second weight vector on the same plan: the interleaved copy follows
    y, Phi, w2, r2 = _inputs(case, B, K, "shared", "shared", seed=5)
    a = _plan(case, B, N, JR, JC, y, setup=setup)
    b = _plan(case, B, N, JR, JC, r2, setup=setup)
    try:
        a.set_mean_basis(Phi)
        a.set_mean_weights(np.full(K, 0.5))
        first = a.log_likelihood()
        a.set_mean_weights(w2)
        second = a.log_likelihood()
        _same(second, b.log_likelihood(), mode)
        assert not np.array_equal(first[2], second[2])
    finally:
        a.close()
        b.close()


def test_one_launch_small_mode_with_a_linear_mean():
    B, N, JR, JC = 4, 2000, 2, 1
    case = synthetic(B, N, JR, JC, "bench", seed=41)
    for y_kind, phi_kind in Y_PHI:
        _bit_identity(case, B, N, JR, JC, 3, y_kind, phi_kind, setup=lambda p: p.set_small_mode(1),
                      check=lambda a, b: a.small_mode_active() or pytest.fail("one-launch mode not taken"))


def test_warm_start_with_a_linear_mean():
    B, N, JR, JC = 9, 12000, 2, 3
    case = synthetic(B, N, JR, JC, "accuracy", seed=77)

    def check(a, b):
        assert a.warm_start()["active"] == 1 and b.warm_start()["active"] == 1

    for y_kind, phi_kind in Y_PHI:
        _bit_identity(case, B, N, JR, JC, 3, y_kind, phi_kind, setup=lambda p: p.set_warm_start(1, 128), check=check)


def test_wide_plan_with_a_linear_mean():
    B, N, JR, JC = 4, 6000, 4, 4
    case = synthetic(B, N, JR, JC, "bench", seed=51)
    for i, (y_kind, phi_kind) in enumerate(Y_PHI):
        _bit_identity(case, B, N, JR, JC, 3, y_kind, phi_kind, basis_first=i % 2 == 1)


@pytest.mark.parametrize("JR,JC", [(2, 3), (4, 4)])
def test_materialising_run_and_solve_with_a_linear_mean(JR, JC):
    B, N = 5, 4000
    case = synthetic(B, N, JR, JC, "bench", seed=71)

    def check(a, b):
        assert np.array_equal(a.solve(), b.solve())

    for y_kind, phi_kind in Y_PHI:
        _bit_identity(case, B, N, JR, JC, 3, y_kind, phi_kind, materialize=True, check=check)


# ---- 2. K = 1, Phi = ones is the constant mean ----------------------------------------------------------------------

@pytest.mark.parametrize("phi_kind", ["shared", "per"])
def test_one_basis_function_of_ones_is_the_constant_mean(phi_kind):
    """The evaluation's bits are the constant mean's; the weight gradient (solve + projection) against the constant
    mean's partial from the reverse gradient sweep: 6.9e-14 (1 + sum |K^-1 r|) seen on an MI355X."""
    B, N, JR, JC = 5, 4000, 2, 3
    case = synthetic(B, N, JR, JC, "bench", seed=83)
    w = np.random.RandomState(2).uniform(-1, 1, (B, 1))
    ones = np.ones((1, N)) if phi_kind == "shared" else np.ones((B, 1, N))
    a = _plan(case, B, N, JR, JC, case["y"])
    b = _plan(case, B, N, JR, JC, case["y"])
    try:
        a.set_mean_basis(ones)
        a.set_mean_weights(w)
        b.set_mean(w[:, 0])
        _same(a.log_likelihood(True), b.log_likelihood(True), "K = 1, ones")       # (1 x w is exact)
        dw, st = a.grad_mean_weights()
        x = b.solve()
        _, _, dmean, st2 = b.grad_log_likelihood(mean_partial=True)
    finally:
        a.close()
        b.close()
    assert (st == 0).all() and (st2 == 0).all() and dw.shape == (B, 1)
    for p in range(B):
        within("weight gradient of the basis function 1 vs the constant mean's partial / (1 + sum |K^-1 r|)",
               abs(dw[p, 0] - dmean[p]) / (1 + np.sum(np.abs(x[p]))), REL, p)


# ---- 3. the weight gradient against binary128 -----------------------------------------------------------------------

_TRUTH = {}


def _truth(case, key, r, Phi):
    """``(g[B, K], scale[B])``: Phi_b x_b with x_b = K_b^-1 r_b from the binary128 recurrence, and sum |x_b|; once per
    (shape, residual) and session."""
    if key not in _TRUTH:
        B, K = r.shape[0], Phi.shape[-2]
        P = np.broadcast_to(Phi, (B, K, r.shape[1]))
        g, scale = np.empty((B, K)), np.empty(B)
        for b in range(B):
            x = ref.quad_factor_solve(0.0, *coeffs_of(case, b), case["t"][b], case["diag"][b], r[b], want_factor=False)[2]
            xl = x.astype(np.longdouble)
            g[b] = [float(np.sum(P[b, k].astype(np.longdouble) * xl)) for k in range(K)]
            scale[b] = np.sum(np.abs(x))
        _TRUTH[key] = (g, scale)
    return _TRUTH[key]


def _gradient_against_truth(JR, JC, B, N, phi_kind, setup, tag):
    K = 3
    case = synthetic(B, N, JR, JC, "bench", seed=91)
    y, Phi, w, r = _inputs(case, B, K, "per", phi_kind, seed=3)
    plan = _plan(case, B, N, JR, JC, y, setup)
    try:
        plan.set_mean_basis(Phi)
        plan.set_mean_weights(w)
        _, _, _, st = plan.log_likelihood(True)
        dw, gst = plan.grad_mean_weights()
        chunks = plan.chunks
    finally:
        plan.close()
    assert (st == 0).all() and (gst == 0).all()
    g, scale = _truth(case, (JR, JC, N, phi_kind), r, Phi)
    for p in range(B):
        for k in range(K):
            within("weight gradient vs Phi_k . (binary128 K^-1 r) / (1 + sum |K^-1 r|): " + tag,
                   abs(dw[p, k] - g[p, k]) / (1 + scale[p]), REL, (p, k, phi_kind))
    return chunks


@pytest.mark.parametrize("phi_kind", ["shared", "per"])
@pytest.mark.parametrize("layout", ["reference", "lean"])
@pytest.mark.parametrize("JR,JC", [(2, 1), (2, 3)])
def test_weight_gradient_on_narrow_plans_against_binary128(JR, JC, layout, phi_kind):
    """d loglike / d w = Phi_k^T K^-1 r from the batched solve and the projection, both factor layouts; 24 chunks of 128
    samples over N = 3000 (a ragged last chunk), one ragged slab of the projection.  Largest deviation seen on an
    MI355X: 9.7e-16 (1 + sum |K^-1 r|), over the 120 partials of the eight cases."""
    B, N = 5, 3000

    def setup(p):
        p.set_chunks(24)
        p.set_factor_layout(layout)

    nchunk, L = _gradient_against_truth(JR, JC, B, N, phi_kind, setup, "narrow")
    assert N % L != 0 and nchunk > 1 and N % batch_slab() != 0


@pytest.mark.parametrize("phi_kind", ["shared", "per"])
@pytest.mark.parametrize("N", [2047, 6000])
def test_weight_gradient_on_a_wide_plan_against_binary128(N, phi_kind):
    """Width 12: the wave-per-chunk sweeps on the reference's storage; N = 6000 is two slabs of the projection, the
    second ragged.  Largest deviation seen on an MI355X: 7.7e-16 (1 + sum |K^-1 r|), over the 36 partials of the four
    cases."""
    _gradient_against_truth(4, 4, 3, N, phi_kind, None, "wide")
    assert N % batch_slab() != 0


def batch_slab():
    return 4096                  # clr::CLR_MEAN_SLAB (csrc/clr_bmean_kernels.h)


# ---- 4. new weights, the same factor -------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC", [(2, 3), (4, 4)])
def test_new_weights_need_no_new_materialising_run(JR, JC):
    B, N, K = 5, 5000, 3
    case = synthetic(B, N, JR, JC, "bench", seed=101)
    y, Phi, w1, _ = _inputs(case, B, K, "per", "shared", seed=1)
    w2 = np.random.RandomState(8).uniform(-1.5, 1.5, (B, K))
    xs = np.linspace(0.05, 0.95, 23)
    Phi_xs = np.stack([np.ones_like(xs), xs - 0.5, np.sin(0.3 * xs)])
    a = _plan(case, B, N, JR, JC, y)
    fresh = _plan(case, B, N, JR, JC, y)
    try:
        a.set_mean_basis(Phi)
        a.set_mean_weights(w1)
        a.log_likelihood(True)
        g1, _ = a.grad_mean_weights()
        a.set_mean_weights(w2)                       # the factor does not depend on y: no second materialising run
        g2, st = a.grad_mean_weights()
        p2 = a.predict(xs, mean_basis=Phi_xs)
        fresh.set_mean_basis(Phi)
        fresh.set_mean_weights(w2)
        fresh.log_likelihood(True)
        gf, stf = fresh.grad_mean_weights()
        pf = fresh.predict(xs, mean_basis=Phi_xs)
        with pytest.raises(ValueError, match="mean_basis"):
            a.predict(xs)
        # the prediction is the model at xs plus the conditional mean of the residual
        fresh.set_mean_basis(None)
        fresh.set_series(case["t"], case["diag"], host_residual(y, w2, Phi))
        resid = fresh.predict(xs)
    finally:
        a.close()
        fresh.close()
    assert (st == 0).all() and (stf == 0).all()
    assert not np.array_equal(g1, g2)
    assert np.array_equal(g2, gf) and np.array_equal(p2, pf)
    assert np.array_equal(p2, host_model(w2, Phi_xs) + resid)


# ---- 5. a problem without a factor ---------------------------------------------------------------------------------

def test_an_indefinite_problem_gets_a_row_of_zeros_and_disturbs_no_other():
    B, N, JR, JC, K = 5, 4000, 2, 3, 3
    good = synthetic(B, N, JR, JC, "bench", seed=111)
    bad = dict(good, a_real=good["a_real"].copy())
    bad["a_real"][2] *= -40.0                        # not positive definite
    y, Phi, w, _ = _inputs(good, B, K, "per", "per", seed=4)
    out = []
    for case in (good, bad):
        plan = _plan(case, B, N, JR, JC, y)
        try:
            plan.set_mean_basis(Phi)
            plan.set_mean_weights(w)
            st = plan.log_likelihood(True)[3]
            dw, gst = plan.grad_mean_weights()
        finally:
            plan.close()
        assert np.array_equal(st, gst)
        out.append((dw, gst))
    (dw0, st0), (dw1, st1) = out
    assert (st0 == 0).all()
    assert st1[2] == batch.CLR_NOT_POSITIVE_DEFINITE and (np.delete(st1, 2) == 0).all()
    assert (dw1[2] == 0.0).all()
    keep = [0, 1, 3, 4]
    assert np.array_equal(dw1[keep], dw0[keep]) and np.isfinite(dw0).all()


# ---- 6. limits and refusals ---------------------------------------------------------------------------------------

def test_sixteen_basis_functions_work_and_seventeen_are_refused():
    B, N, JR, JC = 3, 4000, 2, 1
    case = synthetic(B, N, JR, JC, "bench", seed=121)
    _bit_identity(case, B, N, JR, JC, 16, "per", "per", materialize=True,
                  check=lambda a, b: a.grad_mean_weights()[0].shape == (B, 16) or pytest.fail("shape"))
    _bit_identity(case, B, N, JR, JC, 16, "shared", "shared")
    plan = _plan(case, B, N, JR, JC, case["y"])
    try:
        with pytest.raises(ValueError):
            plan.set_mean_basis(np.ones((17, N)))
        seventeen = np.ones((17, N))                  # the library's own check, past the Python layer's
        lib = batch._load()
        assert lib.clr_batch_set_mean_basis(plan._h, 17, batch._ptr(seventeen), 0) == batch.CLR_INVALID_ARGUMENT
        assert lib.clr_batch_set_mean_weights(plan._h, batch._ptr(seventeen)) == batch.CLR_INVALID_ARGUMENT   # no basis
    finally:
        plan.close()


def test_refusals_leave_the_plan_as_it_was():
    B, N, JR, JC, K = 4, 4000, 2, 3, 3
    case = synthetic(B, N, JR, JC, "bench", seed=131)
    y, Phi, w, _ = _inputs(case, B, K, "per", "shared", seed=6)
    plan = _plan(case, B, N, JR, JC, y)
    try:
        base = plan.log_likelihood()
        with pytest.raises(ValueError):                    # no basis yet
            plan.set_mean_weights(w)
        nan_basis = Phi.copy()
        nan_basis[1, 17] = np.nan
        with pytest.raises(RuntimeError, match="non-finite"):
            plan.set_mean_basis(nan_basis)
        _same(plan.log_likelihood(), base, "after a refused basis")
        plan.set_mean_basis(Phi)
        _same(plan.log_likelihood(), base, "zero weights: the residual is y")
        plan.set_mean_weights(w)
        kept = plan.log_likelihood()
        assert not np.array_equal(kept[2], base[2])
        nan_w = w.copy()
        nan_w[2, 1] = np.inf
        with pytest.raises(RuntimeError, match="non-finite"):
            plan.set_mean_weights(nan_w)
        with pytest.raises(RuntimeError, match="mutually exclusive"):
            plan.set_mean(0.3)
        with pytest.raises(RuntimeError, match="mutually exclusive"):
            plan.evaluate(*coeffs_of(case), mean=0.3)
        with pytest.raises(RuntimeError, match="grad_mean_weights"):
            plan.grad_log_likelihood(mean_partial=True)
        with pytest.raises(RuntimeError, match="materialising"):
            plan.grad_mean_weights()                       # not computed: no materialising run yet
        _same(plan.log_likelihood(), kept, "after the refusals")
        _same(plan.evaluate(*coeffs_of(case), mean_weights=w), kept, "evaluate(mean_weights=)")
        plan.set_mean_basis(None)
        _same(plan.log_likelihood(), base, "basis removed")
        plan.set_mean(0.3)                                 # and the reverse: a basis while a constant mean is in force
        with pytest.raises(RuntimeError, match="mutually exclusive"):
            plan.set_mean_basis(Phi)
        plan.set_mean(None)
        _same(plan.log_likelihood(), base, "mean removed")
    finally:
        plan.close()


# ---- 7. reproducibility and sharding ---------------------------------------------------------------------------------

def test_sharded_plan_with_a_linear_mean_matches_the_single_plan():
    """Two shards on one device: evaluation, weight gradient and predict give the unsharded plan's bits (one chunk count
    for both, as bit identity under sharding asks); two calls of the gradient give the same bits."""
    B, N, JR, JC, K = 5, 5000, 2, 1, 3
    case = synthetic(B, N, JR, JC, "bench", seed=141)
    y, Phi, w, _ = _inputs(case, B, K, "shared", "per", seed=7)
    xs = np.linspace(0.1, 0.9, 19)
    Phi_xs = np.stack([np.ones_like(xs), xs - 0.5, np.sin(0.3 * xs)])
    single = _plan(case, B, N, JR, JC, y, setup=lambda p: p.set_chunks(40))
    sh = batch.ShardedBatchedGP(B, N, JR, JC, devices=[0, 0])
    try:
        sh.set_chunks(40)
        sh.set_series(case["t"], case["diag"], y)
        sh.set_coefficients(*coeffs_of(case))
        for plan in (single, sh):
            plan.set_mean_basis(Phi)
            plan.set_mean_weights(w)
        _same(sh.log_likelihood(), single.log_likelihood(), "sharded evaluation")
        _same(sh.evaluate(*coeffs_of(case), mean_weights=w[0]), single.evaluate(*coeffs_of(case), mean_weights=w[0]),
              "sharded evaluate(mean_weights=), one row for all")
        for plan in (single, sh):
            plan.set_mean_weights(w)
        _same(sh.materialize(), single.log_likelihood(True), "sharded materialising run")
        g1, s1 = single.grad_mean_weights()
        g1b, _ = single.grad_mean_weights()
        g2, s2 = sh.grad_mean_weights()
        assert np.array_equal(g1, g1b) and np.array_equal(g1, g2) and np.array_equal(s1, s2) and (s1 == 0).all()
        assert np.isfinite(g1).all() and np.abs(g1).max() > 0
        assert np.array_equal(sh.predict(xs, mean_basis=Phi_xs), single.predict(xs, mean_basis=Phi_xs))
        with pytest.raises(ValueError, match="mean_basis"):
            sh.predict(xs)
        sh.set_mean_basis(None)
        single.set_mean_basis(None)
        _same(sh.log_likelihood(), single.log_likelihood(), "sharded, basis removed")
    finally:
        sh.close()
        single.close()
