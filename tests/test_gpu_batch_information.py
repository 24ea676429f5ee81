# -*- coding: utf-8 -*-
"""``BatchedGP.information`` / ``ShardedBatchedGP.information`` on the device against the dense reference of
tests/_information_ref.py (Cholesky factor and analytic d K / d coefficient; its own error is below 1e-13).

Bar: 1e-10 of sqrt(I_ii I_jj), the project's bar for the gradient on these plans.

Measured on an MI355X (max over the cases of each test, of sqrt(I_ii I_jj)):
    parity, own series, the seven term shapes, both ways of the mean   N = 63: 3.2e-14, 64: 8.4e-14, 65: 4.9e-14,
                                                                       130: 4.6e-14, 700 (22 chunks): 1.1e-13
    parity, shared series (stride 0)                                   2.5e-14
    sequential form (set_exact) at N = 700                             2.6e-14 of the reference, 3.7e-14 of the chunked route
    lengths [700, 1, 2, 64, 130, 389], NaN and unsorted tails          2.3e-14
    linear mean, noise weights and amplitudes in force                 2.5e-14
    I[mean][mean] against 1^T K^-1 1 of fit_mean_weights               8.6e-16 relative
    smallest eigenvalue at unit diagonal, rank-deficient problem       -3.7e-16
"""
import functools

import numpy as np
import pytest

from celerite_amd import batch

import _information_ref as iref

pytestmark = pytest.mark.gpu

BAR = 1e-10
SHAPES = [(1, 0), (0, 1), (2, 3), (1, 3), (0, 4), (8, 0), (3, 2)]
CHUNKS = {63: 0, 64: 2, 65: 2, 130: 2, 700: 22}     # 130: two chunks, ragged last; 700: 22 chunks of 32
B0 = 4


@functools.lru_cache(maxsize=None)
def problems(N, JR, JC, B=B0):
    """B problems with their own series and coefficients, and their dense references WITH the mean's direction (the
    matrix without it is the leading block: the rows of the Gram matrix are independent).  Computed once, never changed."""
    cs = [iref.case(N, JR, JC, 1000 * b + 10 + N + JR) for b in range(B)]
    refs = [iref.dense_information(*c, mean=True) for c in cs]
    for r in refs:
        r.flags.writeable = False
    return cs, refs


def stack(cs, k):
    return np.array([c[k] for c in cs])


def make_plan(cs, nchunk=0, shared=False, lengths=None, cls=None, **kw):
    B, N = len(cs), len(cs[0][0])
    JR, JC = len(cs[0][3]), len(cs[0][5])
    plan = (cls or batch.BatchedGP)(B, N, JR, JC, **kw)
    if nchunk:
        plan.set_chunks(nchunk)
    if shared:
        plan.set_series(cs[0][0], cs[0][1], cs[0][2])
    else:
        plan.set_series(stack(cs, 0), stack(cs, 1), stack(cs, 2), lengths=lengths)
    plan.set_coefficients(*[stack(cs, k) for k in range(3, 9)], jitter=stack(cs, 9))
    return plan


def worst(info, refs, mean):
    dev = 0.0
    for b, r in enumerate(refs):
        want = r if mean else r[:-1, :-1]
        dev = max(dev, iref.scaled_dev(info[b], want))
    return dev


# ---- 1. parity with the dense reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", sorted(CHUNKS))
@pytest.mark.parametrize("JR,JC", SHAPES)
def test_parity_with_dense_reference(JR, JC, N):
    cs, refs = problems(N, JR, JC)
    plan = make_plan(cs, CHUNKS[N])
    try:
        for mean in (False, True):
            info, st = plan.information(mean_partial=mean)
            assert (st == 0).all(), st
            M = 1 + 2 * JR + 4 * JC + (1 if mean else 0)
            assert info.shape == (B0, M, M)
            dev = worst(info, refs, mean)
            print("parity JR %d JC %d N %d mean %d chunks %s: %.2e" % (JR, JC, N, mean, plan.chunks, dev))
            assert dev < BAR
    finally:
        plan.close()


def test_parity_shared_series():
    N, JR, JC = 130, 2, 3
    cs, _ = problems(N, JR, JC)
    shared = [(cs[0][0], cs[0][1], cs[0][2]) + c[3:] for c in cs]
    refs = [iref.dense_information(*c, mean=True) for c in shared]
    plan = make_plan(shared, CHUNKS[N], shared=True)
    try:
        for mean in (False, True):
            info, st = plan.information(mean_partial=mean)
            assert (st == 0).all()
            dev = worst(info, refs, mean)
            print("parity, shared series (stride 0), mean %d: %.2e" % (mean, dev))
            assert dev < BAR
    finally:
        plan.close()


# ---- 2. routes ----------------------------------------------------------------------------------------------------
def test_sequential_form_against_chunked_route():
    N, JR, JC = 700, 2, 3
    cs, refs = problems(N, JR, JC)
    plan = make_plan(cs, CHUNKS[N])
    try:
        chunked, st0 = plan.information(mean_partial=True)
        plan.set_exact(True)
        seq, st1 = plan.information(mean_partial=True)
        assert (st0 == 0).all() and (st1 == 0).all()
        d_ref, d_routes = worst(seq, refs, True), max(iref.scaled_dev(seq[b], chunked[b]) for b in range(B0))
        print("sequential form: vs reference %.2e, vs chunked route %.2e" % (d_ref, d_routes))
        assert d_ref < BAR and d_routes < BAR
    finally:
        plan.close()


# ---- 3. lengths ---------------------------------------------------------------------------------------------------
LENS = np.array([700, 1, 2, 64, 130, 389], dtype=np.int32)


def test_per_problem_lengths():
    N, JR, JC = 700, 1, 3
    cs, _ = problems(N, JR, JC, B=6)
    refs = [iref.dense_information(*([a[:n] for a in c[:3]] + list(c[3:])), mean=True) for c, n in zip(cs, LENS)]
    rng = np.random.default_rng(5)
    outs = []
    for tail in ("nan", "unsorted"):
        arrs = [stack(cs, k).copy() for k in range(3)]
        for b, n in enumerate(LENS):
            for a in arrs:
                a[b, n:] = np.nan if tail == "nan" else rng.uniform(-5, 5, N - n)
        plan = batch.BatchedGP(6, N, JR, JC)
        try:
            plan.set_chunks(CHUNKS[N])
            plan.set_series(*arrs, lengths=LENS)
            plan.set_coefficients(*[stack(cs, k) for k in range(3, 9)], jitter=stack(cs, 9))
            info, st = plan.information(mean_partial=True)
            assert (st == 0).all(), st
            dev = worst(info, refs, True)
            print("lengths %s, %s tails: %.2e" % (LENS.tolist(), tail, dev))
            assert dev < BAR
            outs.append(info)
        finally:
            plan.close()
    assert np.array_equal(outs[0], outs[1])                 # inputs that differ only in the tails: the same bits


# ---- 4. bits ------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_tile_or_sharding():
    N, JR, JC = 700, 2, 3
    cs, refs = problems(N, JR, JC, B=5)
    plan = make_plan(cs, CHUNKS[N])
    try:
        want, st = plan.information(mean_partial=True)
        assert (st == 0).all() and worst(want, refs, True) < BAR
        plan.set_information_tile(2)
        tiled, _ = plan.information(mean_partial=True)
        assert np.array_equal(tiled, want)
        plan.set_information_tile(0)
    finally:
        plan.close()
    for nshards in (2, 3):
        sh = make_plan(cs, CHUNKS[N], cls=batch.ShardedBatchedGP, devices=[0] * nshards)
        try:
            got, st = sh.information(mean_partial=True)
            assert (st == 0).all()
            assert np.array_equal(got, want), nshards
            sh.set_information_tile(1)
            assert np.array_equal(sh.information(mean_partial=True)[0], want)
        finally:
            sh.close()


# ---- 5. structure -------------------------------------------------------------------------------------------------
def test_structure_symmetric_psd_and_mean_entry():
    N, JR, JC = 700, 1, 3
    cs, _ = problems(N, JR, JC)
    # one rank-deficient problem: two identical complex terms
    twin = list(cs[1])
    for k in (5, 6, 7, 8):
        twin[k] = twin[k].copy()
        twin[k][1] = twin[k][0]
    cs = [cs[0], tuple(twin), cs[2], cs[3]]
    plan = make_plan(cs, CHUNKS[N])
    try:
        info, st = plan.information(mean_partial=True)
        assert (st == 0).all()
        for b in range(B0):
            assert np.array_equal(info[b], info[b].T)
            d = np.sqrt(np.diag(info[b]))
            lo = np.linalg.eigvalsh(info[b] / np.outer(d, d)).min()
            print("problem %d: smallest eigenvalue at unit diagonal %.2e" % (b, lo))
            assert lo >= -1e-12
        # I[mean][mean] = 1^T K^-1 1: the linear mean's Gram matrix with Phi = 1, an independent device route
        plan.set_mean_basis(np.ones((1, N)))
        plan.log_likelihood(materialize=True)
        fit = plan.fit_mean_weights()
        assert (fit.status == 0).all()
        rel = np.max(np.abs(info[:, -1, -1] - fit.gram[:, 0, 0]) / fit.gram[:, 0, 0])
        print("I[mean][mean] against 1^T K^-1 1 of fit_mean_weights: %.2e" % rel)
        assert rel < 1e-10
    finally:
        plan.close()


# ---- 6. models in force -------------------------------------------------------------------------------------------
def test_models_in_force():
    N, JR, JC = 130, 2, 3
    cs, _ = problems(N, JR, JC)
    rng = np.random.default_rng(8)
    t = stack(cs, 0)
    Phi = np.stack([np.ones_like(t), t / t.max()], axis=1)                     # (B, 2, N)
    Psi = np.stack([stack(cs, 1), (t > 0.5 * t.max()).astype(float)], axis=1)  # error-bar inflation, a season's jitter
    Gam = np.stack([(np.arange(N) % 2 == 0).astype(float) * np.ones_like(t), (np.arange(N) % 2 == 1) * np.ones_like(t)], axis=1)
    w, s, a = rng.normal(0, 0.3, (B0, 2)), rng.uniform(0.1, 0.5, (B0, 2)), rng.uniform(0.7, 1.4, (B0, 2))
    plan = batch.BatchedGP(B0, N, JR, JC)
    try:
        plan.set_chunks(CHUNKS[N])
        plan.set_mean_basis(Phi)
        plan.set_noise_basis(Psi)
        plan.set_amplitude_basis(Gam)
        plan.set_series(t, stack(cs, 1), stack(cs, 2))
        plan.set_coefficients(*[stack(cs, k) for k in range(3, 9)], jitter=stack(cs, 9))
        plan.set_mean_weights(w)
        plan.set_noise_weights(s)
        plan.set_amplitudes(a)
        info, st = plan.information()
        assert (st == 0).all(), st
        # the effective series on the host: r = y - w Phi, d = diag + s Psi, scale = a Gamma; y' = r / scale, d' = d / scale^2
        r = stack(cs, 2) - np.einsum("bk,bkn->bn", w, Phi)
        d = stack(cs, 1) + np.einsum("bk,bkn->bn", s, Psi)
        sc = np.einsum("bk,bkn->bn", a, Gam)
        refs = [iref.dense_information(t[b], d[b] / sc[b] ** 2, r[b] / sc[b], *cs[b][3:], mean=False) for b in range(B0)]
        dev = max(iref.scaled_dev(info[b], refs[b]) for b in range(B0))
        print("linear mean, noise weights and amplitudes in force: %.2e" % dev)
        assert dev < BAR
        with pytest.raises(RuntimeError, match="clr_batch_information"):
            plan.information(mean_partial=True)
    finally:
        plan.close()


# ---- 7. conventions -----------------------------------------------------------------------------------------------
def test_conventions_bad_problem_and_zero_jitter():
    N, JR, JC = 130, 2, 3
    cs, refs = problems(N, JR, JC)
    bad = list(cs[1])
    bad[1] = -np.abs(bad[1]) - 5.0                         # negative variances: not positive definite
    zero = cs[2][:9] + (0.0,)
    cases = [cs[0], tuple(bad), zero, cs[3]]
    plan = make_plan(cases, CHUNKS[N])
    try:
        info, st = plan.information(mean_partial=True)
        assert st[1] != 0 and st[0] == 0 and st[2] == 0 and st[3] == 0, st
        assert np.isnan(info[1]).all()
        for b in (0, 3):                                   # the neighbours are unaffected
            assert iref.scaled_dev(info[b], refs[b]) < BAR
        assert (info[2][0, :] == 0.0).all() and (info[2][:, 0] == 0.0).all()
        want = iref.dense_information(*zero, mean=True)
        assert iref.scaled_dev(info[2][1:, 1:], want[1:, 1:]) < BAR
    finally:
        plan.close()


def test_information_parameters_is_the_chain():
    from celerite_amd import terms
    N = 130
    kernel = terms.RealTerm(log_a=0.1, log_c=-0.5) + terms.SHOTerm(log_S0=0.2, log_Q=1.0, log_omega0=0.7) + terms.JitterTerm(log_sigma=-2.0)
    prog = batch.compile_kernel(kernel)
    cs, _ = problems(N, 1, 1)
    rng = np.random.default_rng(4)
    params = kernel.get_parameter_vector()[None, :] + 0.05 * rng.standard_normal((B0, prog.n_params))
    plan = batch.BatchedGP(B0, N, prog.J_real, prog.J_comp)
    try:
        plan.set_chunks(CHUNKS[N])
        plan.set_series(stack(cs, 0), stack(cs, 1), stack(cs, 2))
        plan.set_kernel(prog)
        plan.evaluate_parameters(params)
        for mean in (False, True):
            got, st = plan.information_parameters(mean_partial=mean)
            info, _ = plan.information(mean_partial=mean)
            want = batch.chain_information(info, *prog.jacobian(params), mean_partial=mean)
            assert (st == 0).all() and np.array_equal(got, want)
            Q = prog.n_params + (1 if mean else 0)
            assert got.shape == (B0, Q, Q)
            # the chained matrix is the dense reference's in the same parameters
            co = prog.coefficients(params)
            for b in range(B0):
                dense = iref.dense_information(cs[b][0], cs[b][1], cs[b][2], *[c[b] for c in co[:6]], co[6][b], mean=mean)
                ref = batch.chain_information(dense[None], *[x[b:b + 1] for x in prog.jacobian(params)], mean_partial=mean)[0]
                assert iref.scaled_dev(got[b], ref) < BAR
    finally:
        plan.close()


# ---- 8. refusals and non-interference -----------------------------------------------------------------------------
def test_refusals_name_the_entry():
    rng = np.random.default_rng(2)
    N = 1200
    t = np.sort(rng.uniform(0, 10, N))
    wide = batch.BatchedGP(2, N, 21, 0)
    try:
        wide.set_series(t, np.full(N, 0.1), np.sin(t))
        wide.set_coefficients(rng.uniform(0.5, 1, (2, 21)), rng.uniform(0.1, 2, (2, 21)), *[np.zeros((2, 0))] * 4)
        want = wide.log_likelihood()
        with pytest.raises(RuntimeError, match="clr_batch_information"):
            wide.information()
        assert all(np.array_equal(a, b) for a, b in zip(wide.log_likelihood(), want))
    finally:
        wide.close()
    gen = batch.BatchedGP(2, N, 1, 1)
    try:
        gen.set_series(t, np.full(N, 0.1), np.sin(t))
        gen.set_coefficients(np.full((2, 1), 1.0), np.full((2, 1), 0.5), np.full((2, 1), 0.8), np.zeros((2, 1)),
                             np.full((2, 1), 0.3), np.full((2, 1), 2.0))
        gen.set_general(np.full(N, 0.05), 0.1 * np.ones((1, N)), 0.1 * np.ones((1, N)))
        want = gen.log_likelihood()
        with pytest.raises(RuntimeError, match="clr_batch_information"):
            gen.information()
        assert all(np.array_equal(a, b) for a, b in zip(gen.log_likelihood(), want))
    finally:
        gen.close()


def test_information_leaves_the_plan_as_it_was():
    N, JR, JC = 700, 2, 3
    cs, _ = problems(N, JR, JC)
    plan = make_plan(cs, CHUNKS[N])
    try:
        plan.log_likelihood(materialize=True)
        x = plan.solve()
        ll = plan.log_likelihood()
        g = plan.grad_log_likelihood()
        gi, gf = plan.grad_info(), plan.grad_fallbacks()
        plan.information(mean_partial=True)
        assert plan.grad_info() == gi and plan.grad_fallbacks() == gf
        assert np.array_equal(plan.solve(), x)              # the materialised factor
        assert all(np.array_equal(a, b) for a, b in zip(plan.grad_log_likelihood(), g))
        assert all(np.array_equal(a, b) for a, b in zip(plan.log_likelihood(), ll))
    finally:
        plan.close()
