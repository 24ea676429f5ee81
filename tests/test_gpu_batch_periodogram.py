# -*- coding: utf-8 -*-
"""`-m gpu`: ``BatchedGP.periodogram`` (``clr_batch_periodogram``) -- the generalised-least-squares fit of a sinusoid under
the plan's covariance at every trial frequency -- at every narrow kernel shape in both factor layouts against the dense
reference of tests/_periodogram_ref.py, the small solve apart from the sums, bit-identity across everything but the plan's
chunking, under the mean and noise models, against ``fit_mean_weights`` on the device, on an injected signal, and where it
refuses.

Bars (the issue's): ``gram`` entrywise 1e-10 of ``sqrt(G_ii G_jj)`` (border: ``sqrt(G_ii q)``, corner: ``q``); ``power``
``1e-10 kappa q / 2``; ``coef_i sqrt(G_ii)`` ``1e-10 kappa sqrt(q)``, ``kappa`` the condition number of the unit-diagonal
``G`` of the reference, asserted <= 100 (largest met: 1.7).

The two results whose difference the constant-shift test looks at are each within their bar, their difference within two.

Largest deviations seen on the MI355X, in units of the bars' scales:
    all 24 shapes, both layouts, N = 130 and 1000, both families: gram 4.5e-13 (bench family, N = 1000; accuracy 3.1e-15),
        cov 4.2e-13, coef 1.3e-14, power 3.7e-16
    under a constant mean, a linear mean, a noise model                  gram 2.4e-15, coef 6.3e-16, power 2.6e-16
    a constant added to y, with the offset                               coef 3.4e-16, power 2.8e-16
    power against fit_mean_weights' gain in profiled log-likelihood      4.6e-15; coef against its weights 4.9e-17"""
import numpy as np
import pytest

from celerite_amd import batch
from _cases import ALL_WIDTH_SHAPES, synthetic, coeffs_of, within
import _periodogram_ref as pref

pytestmark = pytest.mark.gpu

BAR = 1e-10
CLR_OK, CLR_INVALID_ARGUMENT, CLR_NOT_POSITIVE_DEFINITE = batch.CLR_OK, batch.CLR_INVALID_ARGUMENT, batch.CLR_NOT_POSITIVE_DEFINITE
CLR_NOT_COMPUTED, CLR_UNSUPPORTED = 3, 7                           # include/celerite_hip.h
B_ALL = 5
SHAPES_N = ((130, 2, (2, 72)), (1000, 24, (21, 48)))     # N, set_chunks, the chunking it gives: ragged last chunks of 58 / 40

_REF = {}


def reference(case, key, omega=None, resid=None, diag=None, t_ref=None):
    """``(omega[B, F], grams[B][F, 4, 4])`` of a case by the dense reference, once per session and ``key``."""
    if key not in _REF:
        B = case["t"].shape[0]
        om, grams = [], []
        for p in range(B):
            t = case["t"][p]
            w = pref.scan_frequencies(t) if omega is None else (omega[p] if np.ndim(omega) == 2 else omega)
            K = pref.dense_K(coeffs_of(case, p), t, case["diag"][p] if diag is None else diag[p])
            r = case["y"][p] if resid is None else resid[p]
            grams.append(pref.dense_grams(K, t, r, w, t[0] if t_ref is None else t_ref))
            om.append(w)
        _REF[key] = (np.stack(om), grams)
    return _REF[key]


def check(tag, pg, grams, offset, skip=()):
    """A device result against the reference's bordered matrices, problem by problem; returns the worst (gram, power, coef)."""
    worst = [0.0, 0.0, 0.0]
    K = 3 if offset else 2
    for p, g4 in enumerate(grams):
        if p in skip:
            continue
        fit = pref.fit_from_grams(g4, offset)
        assert np.max(fit.kappa) <= 100.0, (tag, p, fit.kappa)
        assert (pg.status[p] == CLR_OK).all(), (tag, p, pg.status[p])
        gd = np.sqrt(np.stack([np.diag(S)[:K] for S in fit.gram]))          # [F, K] sqrt(G_ii)
        q = fit.gram[:, K, K]
        scale = np.empty_like(fit.gram)
        full = np.concatenate([gd, np.sqrt(q)[:, None]], axis=1)             # sqrt(G_ii) ..., sqrt(q)
        scale = full[:, :, None] * full[:, None, :]
        dev = float(np.max(np.abs(pg.gram[p] - fit.gram) / scale))
        within(tag + ": gram vs dense reference, of sqrt(G_ii G_jj)", dev, BAR, p)
        assert np.array_equal(pg.gram[p], np.swapaxes(pg.gram[p], -1, -2)), (tag, p)
        dp = float(np.max(np.abs(pg.power[p] - fit.power) / (fit.kappa * 0.5 * q)))
        within(tag + ": power vs dense reference, of kappa q / 2", dp, BAR, p)
        dc = float(np.max(np.abs(pg.coef[p] - fit.coef) * gd / (fit.kappa * np.sqrt(q))[:, None]))
        within(tag + ": coef sqrt(G_ii) vs dense reference, of kappa sqrt(q)", dc, BAR, p)
        dv = float(np.max(np.abs(pg.cov[p] - fit.cov) * gd[:, :, None] * gd[:, None, :] / fit.kappa[:, None, None]))
        within(tag + ": cov sqrt(G_ii G_jj) vs dense reference, of kappa", dv, BAR, p)
        worst = [max(a, b) if b == b else float("nan") for a, b in zip(worst, (dev, dp, dc))]
    print("%s: gram %.3e, power %.3e kappa q / 2, coef %.3e kappa sqrt(q)" % (tag, *worst))
    return worst


def make_plan(case, JR, JC, layout="reference", chunks=24, cls=batch.BatchedGP, **kw):
    B, N = case["t"].shape
    plan = cls(B, N, JR, JC, **kw)
    if chunks:
        plan.set_chunks(chunks)
    if layout != "reference":
        plan.set_factor_layout(layout)
    plan.set_series(case["t"], case["diag"], case["y"])
    plan.set_coefficients(*coeffs_of(case), **({"jitter": case["jitter"]} if "jitter" in case else {}))
    return plan


def materialised(case, JR, JC, layout="reference", chunks=24, **kw):
    plan = make_plan(case, JR, JC, layout, chunks, **kw)
    st = plan.log_likelihood(materialize=True)[3] if isinstance(plan, batch.BatchedGP) else plan.materialize()[3]
    assert (st == 0).all()
    return plan


def same(a, b, what=("power", "coef", "cov", "status", "gram")):
    for k in what:
        x, y = getattr(a, k), getattr(b, k)
        assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), k


def cut(pg, rows=slice(None), cols=slice(None)):
    return batch.Periodogram(*[None if a is None else a[rows][:, cols] for a in pg])


# ---------------------------------------------------------------------------------------------------------------------
# 1. every narrow shape, both layouts, both families, with and without the offset; 2. the small solve apart from the sums
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["reference", "lean"])
@pytest.mark.parametrize("JR,JC", ALL_WIDTH_SHAPES)
def test_periodogram_at_every_narrow_shape(JR, JC, layout):
    """The walks are compiled per (J_real, J_comp), factor layout and trig flavour (csrc/clr_bperiodogram_kernels.h): all 24
    shapes, both layouts, N = 130 in two chunks of 72 (the last one 58) and N = 1000 in 21 of 48 (the last one 40), both
    families, 7 frequencies between 4 pi / T and pi / median(dt) per problem, t_ref = t[0] of problem 0.  ``coef``, ``cov``
    and ``power`` are also the host's ``gram_solve`` on the device's own ``gram``, bit for bit."""
    for N, chunks, expect in SHAPES_N:
        for family in ("bench", "accuracy"):
            case = synthetic(B_ALL, N, JR, JC, family, seed=700 + 9 * JC + JR)
            t_ref = float(case["t"][0, 0])
            omega, grams = reference(case, (JR, JC, N, family), t_ref=t_ref)
            plan = materialised(case, JR, JC, layout, chunks)
            try:
                assert plan.chunks == expect
                res = {off: plan.periodogram(omega, offset=off, t_ref=t_ref, return_gram=True) for off in (False, True)}
            finally:
                plan.close()
            for off, pg in res.items():
                K = 3 if off else 2
                assert pg.power.shape == (B_ALL, 7) and pg.coef.shape == (B_ALL, 7, K) and pg.cov.shape == (B_ALL, 7, K, K)
                assert pg.gram.shape == (B_ALL, 7, K + 1, K + 1) and pg.status.shape == (B_ALL, 7) and pg.status.dtype == np.int32
                check("periodogram (%s layout, %s family, N = %d, offset %s)" % (layout, family, N, off), pg, grams, off)
                small_solve_is_the_hosts(pg, off)


def small_solve_is_the_hosts(pg, offset, min_pivot=1e-10):
    K = 3 if offset else 2
    g = pg.gram.reshape(-1, K + 1, K + 1)
    ok = np.isfinite(g).all(axis=(1, 2))
    w, cov, quad, ld, st = batch.gram_solve(g[ok], min_pivot=min_pivot)
    assert np.array_equal(pg.status.reshape(-1)[ok], st)
    good = st == 0
    w[~good] = np.nan                                                  # (gram_solve leaves w0 where it refuses)
    assert np.array_equal(pg.coef.reshape(-1, K)[ok], w, equal_nan=True)
    assert np.array_equal(pg.cov.reshape(-1, K, K)[ok], cov, equal_nan=True)
    d = g[ok][:, :K, K]
    power = d[:, 0] * w[:, 0] + d[:, 1] * w[:, 1]
    if offset:
        power = (power + d[:, 2] * w[:, 2]) - (d[:, 0] * d[:, 0]) / g[ok][:, 0, 0]
    power = 0.5 * power
    assert np.array_equal(pg.power.reshape(-1)[ok], power, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------
# 3. nothing but the plan's chunking matters
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("JR,JC,layout", [(2, 3, "lean"), (1, 1, "reference"), (2, 0, "lean"), (0, 1, "reference")])
def test_results_depend_on_the_chunking_alone(JR, JC, layout):
    """Widths 8, 3, 2, 2 (frequency blocks of 2, 4, 8, 8).  One list of 3 FB + 2 per-problem frequencies is the yardstick:
    its leading 1, FB and FB + 1 frequencies alone, tiles of 1 and 2, a frequency alone, shared against tiled rows, B plans of
    one problem, B = 1, after a solve(), and 2 and 3 shards all give its bits."""
    N = 700
    case = synthetic(B_ALL, N, JR, JC, "accuracy", seed=31 + JR)
    rng = np.random.RandomState(5)
    plan = materialised(case, JR, JC, layout)
    try:
        FB = plan.periodogram_block()
        assert FB == {8: 2, 3: 4, 2: 8}[JR + 2 * JC]
        F = 3 * FB + 2
        T = case["t"][:, -1] - case["t"][:, 0]
        omega = np.stack([np.sort(rng.uniform(4 * np.pi / T[p], np.pi / np.median(np.diff(case["t"][p])), F)) for p in range(B_ALL)])
        t_ref = float(case["t"][0, 0])
        kw = dict(t_ref=t_ref, return_gram=True)
        for off in (False, True):
            full = plan.periodogram(omega, offset=off, **kw)             # the first consumer after the materialising run
            assert (full.status == CLR_OK).all()
            for n in (1, FB, FB + 1):
                same(plan.periodogram(omega[:, :n], offset=off, **kw), cut(full, cols=slice(0, n)))
            same(plan.periodogram(omega[:, F - 1:], offset=off, **kw), cut(full, cols=slice(F - 1, F)))   # a frequency alone
            for tile in (1, 2, 0):
                plan.set_periodogram_tile(tile)
                same(plan.periodogram(omega, offset=off, **kw), full)
            # shared (F,) against the same values tiled to (B, F)
            shared = plan.periodogram(omega[2], offset=off, **kw)
            same(plan.periodogram(np.tile(omega[2], (B_ALL, 1)), offset=off, **kw), shared)
            same(cut(shared, rows=slice(2, 3)), cut(full, rows=slice(2, 3)))
            plan.solve()                                                 # ... now the chunk maps are the solve's
            same(plan.periodogram(omega, offset=off, **kw), full)
            plan.log_likelihood(materialize=True)                        # (the maps are dropped again for the other offset)
            without_gram = plan.periodogram(omega, offset=off, t_ref=t_ref)
            assert without_gram.gram is None
            same(without_gram, full, what=("power", "coef", "cov", "status"))
        results = {off: plan.periodogram(omega, offset=off, **kw) for off in (False, True)}
    finally:
        plan.close()
    for p in (0, B_ALL - 1):                                             # B = 1 against the same problem inside B = 5
        one = {k: (v[p:p + 1] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B_ALL else v) for k, v in case.items()}
        single = materialised(one, JR, JC, layout)
        try:
            for off in (False, True):
                same(single.periodogram(omega[p:p + 1], offset=off, **kw), cut(results[off], rows=slice(p, p + 1)))
                same(single.periodogram(omega[p], offset=off, **kw), cut(results[off], rows=slice(p, p + 1)))
        finally:
            single.close()
    if layout != "reference":                                            # (a sharded plan keeps the reference layout)
        base = materialised(case, JR, JC, "reference")
        try:
            results = {off: base.periodogram(omega, offset=off, **kw) for off in (False, True)}
        finally:
            base.close()
    for nshards in (2, 3):
        sh = materialised(case, JR, JC, "reference", cls=batch.ShardedBatchedGP, devices=[0] * nshards)
        try:
            for off in (False, True):
                same(sh.periodogram(omega, offset=off, **kw), results[off])
                same(sh.periodogram(omega[1], offset=off, **kw), sh.periodogram(np.tile(omega[1], (B_ALL, 1)), offset=off, **kw))
            sh.set_periodogram_tile(1)
            same(sh.periodogram(omega, **kw), results[False])
            assert sh.periodogram_ms() > 0.0
        finally:
            sh.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. means and noise
# ---------------------------------------------------------------------------------------------------------------------

def test_the_residual_and_the_diagonal_in_force():
    JR, JC, N = 2, 1, 700
    case = synthetic(B_ALL, N, JR, JC, "accuracy", seed=12)
    t_ref = float(case["t"][0, 0])
    rng = np.random.RandomState(8)
    omega, _ = reference(case, ("means", "plain"), t_ref=t_ref)
    kw = dict(t_ref=t_ref, return_gram=True)
    # a constant mean
    mu = rng.randn(B_ALL)
    plan = make_plan(case, JR, JC, "lean")
    try:
        plan.set_mean(mu)
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        res = {off: plan.periodogram(omega, offset=off, **kw) for off in (False, True)}
    finally:
        plan.close()
    _, grams = reference(case, ("means", "constant"), omega=omega, resid=case["y"] - mu[:, None], t_ref=t_ref)
    for off in (False, True):
        check("periodogram under a constant mean (offset %s)" % off, res[off], grams, off)
    # a linear mean
    Phi = np.stack([np.ones((B_ALL, N)), case["t"] - case["t"].mean(axis=1, keepdims=True)], axis=1)
    w = rng.randn(B_ALL, 2) * np.array([1.0, 0.01])
    plan = make_plan(case, JR, JC, "reference")
    try:
        plan.set_mean_basis(Phi)
        plan.set_mean_weights(w)
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        res = {off: plan.periodogram(omega, offset=off, **kw) for off in (False, True)}
    finally:
        plan.close()
    resid = case["y"] - np.einsum("bk,bkn->bn", w, Phi)
    _, grams = reference(case, ("means", "linear"), omega=omega, resid=resid, t_ref=t_ref)
    for off in (False, True):
        check("periodogram under a linear mean (offset %s)" % off, res[off], grams, off)
    # a noise model: the effective diagonal is part of the factor
    Psi = np.stack([np.ones((B_ALL, N)), rng.uniform(0.0, 1.0, (B_ALL, N))], axis=1)
    s = rng.uniform(0.1, 0.5, (B_ALL, 2))
    plan = make_plan(case, JR, JC, "lean")
    try:
        plan.set_noise_basis(Psi)
        plan.set_noise_weights(s)
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        res = {off: plan.periodogram(omega, offset=off, **kw) for off in (False, True)}
    finally:
        plan.close()
    diag_eff = case["diag"] + np.einsum("bk,bkn->bn", s, Psi)
    _, grams = reference(case, ("means", "noise"), omega=omega, diag=diag_eff, t_ref=t_ref)
    for off in (False, True):
        check("periodogram under a noise model (offset %s)" % off, res[off], grams, off)
    # with the offset a constant added to y moves coef[..., 0] by that constant and nothing else beyond the bars
    shift = 3.25
    moved = dict(case, y=case["y"] + shift)
    out = []
    for c in (case, moved):
        plan = materialised(c, JR, JC, "reference")
        try:
            out.append(plan.periodogram(omega, offset=True, **kw))
        finally:
            plan.close()
    a, b = out
    _, grams = reference(case, ("means", "plain"), t_ref=t_ref)
    for p in range(B_ALL):
        fit = pref.fit_from_grams(grams[p], True)
        _, gm = reference(moved, ("means", "moved"), omega=omega, t_ref=t_ref)
        fm = pref.fit_from_grams(gm[p], True)
        gd, q = np.sqrt(np.stack([np.diag(S)[:3] for S in fit.gram])), np.maximum(fit.gram[:, 3, 3], fm.gram[:, 3, 3])
        delta = (b.coef[p] - a.coef[p]) - np.array([shift, 0.0, 0.0])
        within("offset: coef moves by the constant added to y, of kappa sqrt(q)",
               np.max(np.abs(delta) * gd / (fit.kappa * np.sqrt(q))[:, None]), 2 * BAR, p)
        within("offset: power unmoved by a constant added to y, of kappa q / 2",
               np.max(np.abs(b.power[p] - a.power[p]) / (fit.kappa * 0.5 * q)), 2 * BAR, p)
        assert np.array_equal(a.cov[p], b.cov[p])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the cross-check on the device: fit_mean_weights with (cos, sin) uploaded
# ---------------------------------------------------------------------------------------------------------------------

def test_power_is_the_gain_in_profiled_log_likelihood_of_fit_mean_weights():
    JR, JC, N = 1, 2, 700
    case = synthetic(B_ALL, N, JR, JC, "accuracy", seed=77)
    t_ref = float(case["t"][0, 0])
    omega, grams = reference(case, ("cross",), t_ref=t_ref)
    pick = [0, 3, 6]
    plan = materialised(case, JR, JC, "lean")
    try:
        pg = plan.periodogram(omega, t_ref=t_ref)
        ll0 = plan.log_likelihood(materialize=True)[0]
    finally:
        plan.close()
    for f in pick:
        Phi = np.stack([np.cos(omega[:, f, None] * (case["t"] - t_ref)), np.sin(omega[:, f, None] * (case["t"] - t_ref))], axis=1)
        plan = make_plan(case, JR, JC, "lean")
        try:
            plan.set_mean_basis(Phi)
            plan.set_mean_weights(np.zeros((B_ALL, 2)))
            assert (plan.log_likelihood(materialize=True)[3] == 0).all()
            fit = plan.fit_mean_weights()
        finally:
            plan.close()
        assert (fit.status == 0).all()
        for p in range(B_ALL):
            ref_fit = pref.fit_from_grams(grams[p], False)
            q, kappa = ref_fit.gram[f, 2, 2], ref_fit.kappa[f]
            within("power vs fit_mean_weights' gain in profiled log-likelihood, of kappa q / 2",
                   abs(pg.power[p, f] - (fit.loglike[p] - ll0[p])) / (kappa * 0.5 * q), BAR, (p, f))
            within("coef vs fit_mean_weights' weights, of kappa sqrt(q)",
                   np.max(np.abs(pg.coef[p, f] - fit.weights[p]) * np.sqrt(np.diag(ref_fit.gram[f])[:2])) / (kappa * np.sqrt(q)), BAR, (p, f))


# ---------------------------------------------------------------------------------------------------------------------
# 6. a known answer
# ---------------------------------------------------------------------------------------------------------------------

def injected_case(seed=4):
    """Draws of the GP (dense Cholesky; the accuracy family at a twentieth of its variances, white noise of 0.3 .. 0.45) plus
    0.5 cos(w0 t + 0.3), N = 1000; a grid of 64 frequencies that contains w0."""
    JR, JC, N, B = 1, 1, 1000, 3
    case = synthetic(B, N, JR, JC, "accuracy", seed=seed)
    case = dict(case, a_real=0.05 * case["a_real"], a_comp=0.05 * case["a_comp"], b_comp=0.05 * case["b_comp"], diag=0.09 * case["diag"])
    rng = np.random.RandomState(seed + 1)
    grid = np.linspace(0.05, 0.68, 64)
    w0 = grid[23]
    y = np.empty((B, N))
    for p in range(B):
        K = pref.dense_K(coeffs_of(case, p), case["t"][p], case["diag"][p])
        y[p] = np.linalg.cholesky(K) @ rng.randn(N) + 0.5 * np.cos(w0 * case["t"][p] + 0.3)
    return dict(case, y=y), grid, 23


def amplitude_phase_within(pg_amp, pg_phase, coef, cov, a=0.5, phi=0.3, sigmas=3.0):
    """amplitude and phase against the injected ones in units of their own standard deviations (first-order propagation of
    ``cov`` through hypot and arctan2(-B, A))."""
    A, Bc = coef[-2], coef[-1]
    c = cov[-2:, -2:]
    amp = np.hypot(A, Bc)
    ja = np.array([A, Bc]) / amp
    jp = np.array([Bc, -A]) / (amp * amp)
    assert abs(pg_amp - a) <= sigmas * np.sqrt(ja @ c @ ja), (pg_amp, np.sqrt(ja @ c @ ja))
    assert abs(pg_phase - phi) <= sigmas * np.sqrt(jp @ c @ jp), (pg_phase, np.sqrt(jp @ c @ jp))


def test_an_injected_sinusoid_is_found_at_its_frequency():
    case, grid, at = injected_case()
    B = case["t"].shape[0]
    _, grams = reference(case, ("injected",), omega=grid, t_ref=0.0)
    for p in range(B):                                                    # the reference itself satisfies the claim
        for off in (False, True):
            fit = pref.fit_from_grams(grams[p], off)
            assert int(np.argmax(fit.power)) == at
            A, Bc = fit.coef[at, -2], fit.coef[at, -1]
            amplitude_phase_within(np.hypot(A, Bc), np.arctan2(-Bc, A), fit.coef[at], fit.cov[at])
    plan = materialised(case, 1, 1, "lean")
    try:
        res = {off: plan.periodogram(grid, offset=off) for off in (False, True)}
    finally:
        plan.close()
    for off, pg in res.items():
        assert (pg.status == CLR_OK).all()
        assert (np.argmax(pg.power, axis=1) == at).all()
        for p in range(B):
            amplitude_phase_within(pg.amplitude[p, at], pg.phase[p, at], pg.coef[p, at], pg.cov[p, at])


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals and statuses
# ---------------------------------------------------------------------------------------------------------------------

def test_a_zero_frequency_is_refused_alone():
    JR, JC, N = 2, 1, 700
    case = synthetic(B_ALL, N, JR, JC, "accuracy", seed=19)
    omega = np.array([0.3, 0.0, 0.7, 1.1, 0.9])
    plan = materialised(case, JR, JC, "reference")
    try:
        for off in (True, False):
            pg = plan.periodogram(omega, offset=off, return_gram=True)
            rest = plan.periodogram(np.delete(omega, 1), offset=off, return_gram=True)
            assert (pg.status[:, 1] == CLR_NOT_POSITIVE_DEFINITE).all() and (np.delete(pg.status, 1, axis=1) == CLR_OK).all()
            assert np.isnan(pg.power[:, 1]).all() and np.isnan(pg.coef[:, 1]).all() and np.isnan(pg.cov[:, 1]).all()
            assert np.isfinite(pg.gram[:, 1]).all()
            K = 3 if off else 2
            assert (pg.gram[:, 1, K - 1, K - 1] == 0.0).all()             # sin(0) = 0: a zero on the diagonal of G
            same(batch.Periodogram(*[np.delete(a, 1, axis=1) for a in pg]), rest)
            small_solve_is_the_hosts(pg, off)
        # a frequency far below 1 / T with the offset: cos is the constant column again
        T = case["t"].max() - case["t"].min()
        pg = plan.periodogram(np.array([1e-9 / T, 0.5]), offset=True, return_gram=True)
        assert (pg.status[:, 0] == CLR_NOT_POSITIVE_DEFINITE).all() and (pg.status[:, 1] == CLR_OK).all()
        assert np.isnan(pg.power[:, 0]).all() and np.isfinite(pg.gram).all()
    finally:
        plan.close()


def test_a_failed_evaluation_is_nan_with_its_status_at_every_frequency():
    JR, JC, N = 2, 1, 700
    case = synthetic(B_ALL, N, JR, JC, "accuracy", seed=19)
    bad = {k: v.copy() for k, v in case.items()}
    bad["a_real"][2] = -50.0                                              # not positive definite
    bad["diag"][2] = 1e-3
    plan = make_plan(bad, JR, JC, "reference")
    try:
        st = plan.log_likelihood(materialize=True)[3]
        assert st[2] != CLR_OK and (np.delete(st, 2) == CLR_OK).all()
        pg = plan.periodogram(np.array([0.3, 0.7, 1.1]), offset=True, return_gram=True)
    finally:
        plan.close()
    assert (pg.status[2] == st[2]).all() and (np.delete(pg.status, 2, axis=0) == CLR_OK).all()
    for a in (pg.power, pg.coef, pg.cov, pg.gram):
        assert np.isnan(a[2]).all() and np.isfinite(np.delete(a, 2, axis=0)).all()


def raw_call(plan, omega, stride=0, t_ref=0.0, offset=0, min_pivot=1e-10, outputs=True, F=None):
    """``clr_batch_periodogram`` itself: (status, the output arrays as they came back)."""
    import ctypes as C
    lib = batch._load()
    omega = np.ascontiguousarray(omega, dtype=np.float64)
    F = omega.shape[-1] if F is None else F
    K = 3 if offset else 2
    n = max(F, 1)
    outs = [np.full((plan.B, n), -7.0), np.full((plan.B, n, K), -7.0), np.full((plan.B, n, K, K), -7.0), np.full((plan.B, n, K + 1, K + 1), -7.0)]
    st = np.full((plan.B, n), -7, dtype=np.int32)
    dp = C.POINTER(C.c_double)
    ptrs = [a.ctypes.data_as(dp) for a in outs] if outputs else [None] * 4
    rc = lib.clr_batch_periodogram(plan._h, int(F), omega.ctypes.data_as(dp), stride, float(t_ref), int(offset), float(min_pivot),
                                   *ptrs, st.ctypes.data_as(C.POINTER(C.c_int)) if outputs else None)
    return rc, outs + [st]


def untouched(outs):
    return all((a == -7).all() for a in outs)


def test_bad_arguments_and_a_plan_without_a_factor():
    JR, JC, N = 2, 1, 700
    case = synthetic(2, N, JR, JC, "accuracy", seed=19)
    plan = make_plan(case, JR, JC, "reference")
    try:
        ll = plan.log_likelihood()[0]
        rc, outs = raw_call(plan, np.array([0.3, 0.5]))
        assert rc == CLR_NOT_COMPUTED and untouched(outs)                 # no materialising run
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        w = np.array([0.3, 0.5])
        for kwargs in (dict(F=-1), dict(stride=1), dict(t_ref=np.nan), dict(t_ref=np.inf), dict(min_pivot=-1e-3), dict(min_pivot=1.0),
                       dict(min_pivot=np.nan), dict(outputs=False)):
            rc, outs = raw_call(plan, w, **kwargs)
            assert rc == CLR_INVALID_ARGUMENT and untouched(outs), kwargs
        for badw in (np.array([0.3, np.nan]), np.array([np.inf, 0.3])):
            rc, outs = raw_call(plan, badw)
            assert rc == CLR_INVALID_ARGUMENT and untouched(outs)
        rc, outs = raw_call(plan, w, F=0)
        assert rc == CLR_OK and untouched(outs)                           # F = 0: nothing to do, as M = 0 of the point consumers
        pg = plan.periodogram(w)
        assert (pg.status == CLR_OK).all() and np.isfinite(pg.power).all()
        assert plan.periodogram_ms() > 0.0
        assert np.array_equal(plan.log_likelihood()[0], ll)
    finally:
        plan.close()


def expect_unsupported(plan, message):
    rc, outs = raw_call(plan, np.array([0.3, 0.5]))
    assert rc == CLR_UNSUPPORTED and untouched(outs)
    text = batch._load().clr_last_error().decode()
    assert message in text, text
    with pytest.raises(Exception):
        plan.periodogram(np.array([0.3, 0.5]))


def test_what_the_periodogram_refuses():
    N = 700
    # a wide plan
    case = synthetic(2, N, 1, 4, "accuracy", seed=3)
    plan = make_plan(case, 1, 4, "reference", chunks=0)
    try:
        before = plan.log_likelihood(materialize=True)
        expect_unsupported(plan, "clr_batch_fit_mean_weights")
        assert all(np.array_equal(a, b) for a, b in zip(before, plan.log_likelihood(materialize=True)))
    finally:
        plan.close()
    case = synthetic(2, N, 2, 1, "accuracy", seed=3)
    # general terms
    plan = make_plan(case, 2, 1, "reference", chunks=0)
    try:
        rng = np.random.RandomState(1)
        U = 1e-2 * rng.rand(2, 2, N)
        plan.set_general(1e-3 + np.sum(U * U, axis=1), U, U)
        before = plan.log_likelihood()
        expect_unsupported(plan, "general terms")
        assert all(np.array_equal(a, b) for a, b in zip(before, plan.log_likelihood()))
    finally:
        plan.close()
    # per-problem lengths
    plan = batch.BatchedGP(2, N, 2, 1)
    try:
        plan.set_series(case["t"], case["diag"], case["y"], lengths=[N, N - 100])
        plan.set_coefficients(*coeffs_of(case))
        before = plan.log_likelihood()
        expect_unsupported(plan, "per-problem lengths")
        assert all(np.array_equal(a, b) for a, b in zip(before, plan.log_likelihood()))
    finally:
        plan.close()
    # amplitudes in force
    plan = make_plan(case, 2, 1, "reference")
    try:
        plan.set_amplitude_basis(np.ones((2, 1, N)))
        plan.set_amplitudes(np.full((2, 1), 2.0))
        before = plan.log_likelihood(materialize=True)
        expect_unsupported(plan, "amplitudes are in force")
        assert all(np.array_equal(a, b) for a, b in zip(before, plan.log_likelihood(materialize=True)))
    finally:
        plan.close()
    # an unchunked plan
    short = synthetic(2, 100, 2, 1, "accuracy", seed=3)
    plan = make_plan(short, 2, 1, "reference", chunks=0)
    try:
        before = plan.log_likelihood(materialize=True)
        expect_unsupported(plan, "needs a chunked plan")
        assert all(np.array_equal(a, b) for a, b in zip(before, plan.log_likelihood(materialize=True)))
    finally:
        plan.close()
