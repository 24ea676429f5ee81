# -*- coding: utf-8 -*-
"""Batched plans evaluated straight from ``terms`` kernel parameters (BatchedGP.set_kernel / evaluate_parameters /
grad_parameters / coefficients and the sharded twins): the coefficients are formed on the device by the compiled
program, so the results must be the SAME BITS as ``evaluate`` on the coefficients read back, the coefficients within
the derived ulp bound of the host evaluator's, and everything within the oracle tolerance of test_gpu_batch.py."""
import os
import re

import numpy as np
import pytest

from celerite_amd import batch, terms
from oracle import ref
from _cases import within
from test_kernel_program_cpu import ULP, LEAF_ULP, _bound, _envelopes

pytestmark = pytest.mark.gpu

REL = 1e-10     # tests/test_gpu_batch.py: log det, quadratic form and log-likelihood against the oracle
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _complex_sum(n):
    k = None
    for j in range(n):
        t = terms.ComplexTerm(0.1 - 0.02 * j, 2.0 + 0.05 * j, 1.6 - 0.06 * j)
        k = t if k is None else k + t
    return k


def _bench():
    return terms.RealTerm(1.0, 0.1) + terms.RealTerm(0.9, 0.3) + _complex_sum(3)


# (name, kernel, J_real, J_comp, levels of products, B, N)
CASES = [
    ("width 3: real + sho", lambda: terms.RealTerm(1.0, 0.1) + terms.SHOTerm(0.1, 1.0, 1.5), 1, 1, 0, 64, 4096),
    ("width 8: bench kernel", _bench, 2, 3, 0, 64, 4096),
    ("width 8: bench kernel + jitter", lambda: _bench() + terms.JitterTerm(-2.0), 2, 3, 0, 64, 4096),
    ("width 3: product", lambda: terms.RealTerm(0.5, 0.1) * terms.ComplexTerm(0.1, -1.5, 1.0, 1.6) + terms.RealTerm(1.0, 0.3),
     1, 1, 1, 64, 4096),
    ("width 16", lambda: _complex_sum(8), 0, 8, 0, 64, 4096),
    ("width 32 (chunked wide plan)", lambda: _complex_sum(16), 0, 16, 0, 64, 8192),
    ("launch-latency shape: configs[1] 256 x 1e4 x width 4", lambda: _complex_sum(2), 0, 2, 0, 256, 10000),
]
IDS = [c[0] for c in CASES]


def _setup(make, JR, JC, B, N, seed=0, cls=batch.BatchedGP, **kw):
    rng = np.random.RandomState(seed)
    kernel = make()
    p0 = kernel.get_parameter_vector()
    draws = p0[None, :] + 0.1 * np.clip(rng.randn(B, len(p0)), -3, 3)
    t = np.sort(rng.rand(B, N), axis=1)
    diag = rng.uniform(0.1, 0.2, (B, N)) ** 2
    y = np.sin(t) + 0.3
    mean = rng.uniform(0.0, 0.6, B)
    plan = cls(B, N, JR, JC, **kw)
    plan.set_series(t, diag, y)
    prog = plan.set_kernel(kernel)
    assert (prog.J_real, prog.J_comp) == (JR, JC)
    return kernel, draws, t, diag, y, mean, plan


def _same(a, b, what):
    for x, z, name in zip(a, b, ("loglike", "logdet", "quad", "status")):
        assert np.array_equal(np.asarray(x), np.asarray(z), equal_nan=(name != "status")), (what, name, x, z)


@pytest.mark.parametrize("name,make,JR,JC,depth,B,N", CASES, ids=IDS)
def test_same_bits_as_evaluate_on_the_coefficients_read_back(name, make, JR, JC, depth, B, N):
    kernel, draws, t, diag, y, mean, plan = _setup(make, JR, JC, B, N)
    saved = kernel.get_parameter_vector().copy()
    try:
        for m in (None, mean):
            got = plan.evaluate_parameters(draws, mean=m)
            flags = plan.exact_flags()
            co = plan.coefficients()
            want = plan.evaluate(*co[:6], jitter=co[6], mean=m)
            _same(got, want, (name, "mean" if m is not None else "no mean"))
            assert np.array_equal(flags, plan.exact_flags()), name
            assert (got[3] == 0).all()
        # 6: the device's coefficients against the host evaluator's table -- the derived bound of
        # test_kernel_program_cpu.py (device exp within 1 ulp, sqrt and / correctly rounded: see the flags test below)
        host = plan.kernel_program.coefficients(draws)
        env = _envelopes(kernel, draws) + [np.abs(host[6])]
        for d, h, s, block in zip(co, host, env, ("a_real", "c_real", "a_comp", "b_comp", "c_comp", "d_comp", "jitter")):
            assert d.shape == h.shape
            if d.size:
                dev = np.max(np.abs(d - h) / np.maximum(s, 1e-300)) / ULP
                within("device coefficients vs host evaluator, ulp of the envelope / allowed", dev / (2 * _bound(depth)), 1.0, (name, block))
        # 7: end to end against the oracle at the Python table's coefficients
        plan.evaluate_parameters(draws, mean=mean)
        ll, ld, q, st = plan.evaluate_parameters(draws, mean=mean)
        tab = batch.kernel_coefficient_table(kernel, draws, compiled=False)
        l0, d0, q0, s0 = ref.batch_log_likelihood(tab[6], *tab[:6], t, diag, y - mean[:, None])
        assert np.array_equal(st, s0)
        within("from parameters: log det vs oracle", np.max(np.abs(ld - d0) / np.abs(d0)), REL, name)
        within("from parameters: quadratic form vs oracle", np.max(np.abs(q - q0) / np.abs(q0)), REL, name)
        within("from parameters: log-likelihood vs oracle", np.max(np.abs(ll - l0) / np.abs(l0)), REL, name)
        assert np.array_equal(saved, kernel.get_parameter_vector())
    finally:
        plan.close()


@pytest.mark.parametrize("name,make,JR,JC,depth,B,N", CASES, ids=IDS)
def test_gradient_chain_on_the_device(name, make, JR, JC, depth, B, N):
    """grad_parameters against chain_gradient(grad_log_likelihood(), host Jacobian at p): the same products summed in
    another order -- a P-term dot product, P 2^-52 sum |terms| -- for both forms (with and without the mean)."""
    kernel, draws, t, diag, y, mean, plan = _setup(make, JR, JC, B, N)
    try:
        P = draws.shape[1]
        jac, jj = plan.kernel_program.jacobian(draws)
        for with_mean in (False, True):
            ll, ld, q, st = plan.evaluate_parameters(draws, mean=mean)
            value, g, gst = plan.grad_parameters(mean_partial=with_mean)
            assert g.shape == (B, P + (1 if with_mean else 0)) and (gst == 0).all()
            if with_mean:
                v2, cg, dm, st2 = plan.grad_log_likelihood(mean_partial=True)
                want = batch.chain_gradient(cg, jac, jj, dmean=dm)
                assert np.array_equal(g[:, P], dm)
            else:
                v2, cg, st2 = plan.grad_log_likelihood()
                want = batch.chain_gradient(cg, jac, jj)
            assert np.array_equal(value, v2) and np.array_equal(gst, st2)
            terms_abs = np.einsum("bpc,bc->bp", np.abs(jac), np.abs(cg[:, 1:])) + np.abs(jj * cg[:, :1])
            dev = np.abs(g[:, :P] - want[:, :P])
            bar = P * ULP * terms_abs
            worst = float(np.max(dev / np.maximum(bar, 1e-300)))
            print("%s: chain rule on the device vs host, worst deviation / (P 2^-52 sum |terms|) = %.3f" % (name, worst))
            within("grad_parameters vs chain_gradient(host Jacobian) / (P 2^-52 sum |terms|)", worst, 1.0, name)
    finally:
        plan.close()


@pytest.mark.parametrize("name,make,JR,JC,depth,B,N", CASES, ids=IDS)
def test_gradient_against_central_differences(name, make, JR, JC, depth, B, N):
    """grad_parameters(mean_partial=True) against central differences of evaluate_parameters in every parameter and
    the mean.  test_gpu_batch_mean.py's chain-rule test holds the chained gradient to 1e-9 of the problem's largest
    partial against the object API and uses no step; for differences the bar is derived: step h = 1e-4, rounding of
    the two values N 2^-53 (|log det| + |quad|) each over 2 h, truncation h^2 f''' / 6 with |f'''| <= 60 x the largest
    partial (the parameters are logarithms: every derivative of exp(p) is exp(p); 60 covers the curvature of the
    solve in c and d) -- and 1e-9 of the largest partial on top, the chain-rule test's own bar."""
    kernel, draws, t, diag, y, mean, plan = _setup(make, JR, JC, min(B, 64), N)
    B = min(B, 64)
    try:
        P, h = draws.shape[1], 1e-4
        ll, ld, q, st = plan.evaluate_parameters(draws, mean=mean)
        value, g, gst = plan.grad_parameters(mean_partial=True)
        assert (st == 0).all() and (gst == 0).all()
        fd = np.empty((B, P + 1))
        for p in range(P + 1):
            up, dn, mu, md = draws.copy(), draws.copy(), mean.copy(), mean.copy()
            if p < P:
                up[:, p] += h
                dn[:, p] -= h
            else:
                mu += h
                md -= h
            fd[:, p] = (plan.evaluate_parameters(up, mean=mu)[0] - plan.evaluate_parameters(dn, mean=md)[0]) / (2 * h)
        gmax = np.max(np.abs(g), axis=1, keepdims=True)
        bar = 2 * N * 2.0 ** -53 * (np.abs(ld) + np.abs(q))[:, None] / (2 * h) + 10 * h * h * gmax + 1e-9 * gmax
        worst = float(np.max(np.abs(g - fd) / bar))
        print("%s: gradient vs central differences, worst deviation / bar = %.3f (largest relative to the largest partial %.2e)"
              % (name, worst, float(np.max(np.abs(g - fd) / gmax))))
        within("grad_parameters vs central differences / derived bar", worst, 1.0, name)
    finally:
        plan.close()


def test_refused_draws_do_not_disturb_the_batch():
    """One draw across an SHO regime, one with a NaN parameter: CLR_INVALID_ARGUMENT and NaN for those two; every other
    problem -- the stand-in rows included -- bitwise what evaluate(*plan.coefficients()) gives on the same plan."""
    make = lambda: terms.RealTerm(1.0, 0.1) + terms.SHOTerm(0.1, 1.0, 1.5) + _complex_sum(2)
    kernel, draws, t, diag, y, mean, plan = _setup(make, 1, 3, 64, 4096)
    try:
        bad = [7, 33]
        draws[7, 3] = np.log(0.2)       # log_Q of the SHO term: the other regime
        draws[33, 0] = np.nan
        got = plan.evaluate_parameters(draws, mean=mean)
        flags = plan.exact_flags()
        co = plan.coefficients()
        assert all(np.isfinite(c).all() for c in co)        # (the stand-ins: nothing non-finite reaches the scan)
        want = plan.evaluate(*co[:6], jitter=co[6], mean=mean)
        assert np.array_equal(flags, plan.exact_flags())
        good = np.delete(np.arange(64), bad)
        for x, z in zip(got, want):
            assert np.array_equal(x[good], z[good])
        assert (got[3][bad] == batch.CLR_INVALID_ARGUMENT).all() and (got[3][good] == 0).all()
        for x in got[:3]:
            assert np.isnan(x[bad]).all()
        assert np.isfinite(want[0][bad]).all()
        tab = batch.kernel_coefficient_table(kernel, draws[good], compiled=False)
        l0, d0, q0, s0 = ref.batch_log_likelihood(tab[6], *tab[:6], t[good], diag[good], (y - mean[:, None])[good])
        within("refused draws: the others' log det vs oracle", np.max(np.abs(got[1][good] - d0) / np.abs(d0)), REL)
        within("refused draws: the others' quadratic form vs oracle", np.max(np.abs(got[2][good] - q0) / np.abs(q0)), REL)
        within("refused draws: the others' log-likelihood vs oracle", np.max(np.abs(got[0][good] - l0) / np.abs(l0)), REL)
        plan.evaluate_parameters(draws, mean=mean)
        value, g, gst = plan.grad_parameters(mean_partial=True)
        assert (gst[bad] == batch.CLR_INVALID_ARGUMENT).all() and np.isnan(g[bad]).all() and np.isnan(value[bad]).all()
        assert np.isfinite(g[good]).all() and (gst[good] == 0).all()
    finally:
        plan.close()


def test_kernel_and_plan_shapes_must_agree():
    plan = batch.BatchedGP(4, 600, 1, 1)
    prog = batch.compile_kernel(_bench())
    try:
        lib = batch._load()
        assert lib.clr_batch_set_kernel(plan._h, prog._k) == batch.CLR_DIMENSION_MISMATCH
        with pytest.raises(ValueError):
            plan.set_kernel(_bench())
        with pytest.raises(RuntimeError):       # no kernel set: nothing to evaluate
            plan.evaluate_parameters(np.zeros((4, 5)))
    finally:
        plan.close()


def test_the_unit_is_compiled_with_ieee_arithmetic():
    """sqrt and / are correctly rounded and no FMA is formed only without fast-math and contraction: the Makefile gives
    kernel_program.hip and the host evaluator -ffp-contract=off and no fast-math flag."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    flags = re.search(r"^KP_FPFLAGS\s*:=\s*(.*)$", mk, re.M).group(1)
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags
    for rule in ("kernel_program.o", "kernel_program_host.o"):
        body = re.search(r"\$\(BUILD\)/%s:.*\n\t(.*)" % re.escape(rule), mk).group(1)
        assert "$(KP_FPFLAGS)" in body and "-ffast-math" not in body and "-Ofast" not in body
    assert "-ffast-math" not in mk.replace("-fno-fast-math", "") and "-Ofast" not in mk


def _device_lists():
    n = batch.device_count()
    lists = [[0, 0, 0]]
    if n > 1:
        lists.append(list(range(n)))
    return lists


@pytest.mark.parametrize("name,make,JR,JC,depth,B,N", [CASES[1], CASES[2], CASES[5]], ids=[IDS[1], IDS[2], IDS[5]])
def test_sharded_same_bits_as_the_unsharded_plan(name, make, JR, JC, depth, B, N):
    kernel, draws, t, diag, y, mean, plan = _setup(make, JR, JC, B, N)
    try:
        nchunk = plan.chunks[0]
        want = plan.evaluate_parameters(draws, mean=mean)
        wco = plan.coefficients()
        wg = plan.grad_parameters(mean_partial=True)
    finally:
        plan.close()
    for devices in _device_lists():
        sh = batch.ShardedBatchedGP(B, N, JR, JC, devices=devices)
        try:
            sh.set_chunks(nchunk)
            sh.set_series(t, diag, y)
            sh.set_kernel(make())
            got = sh.evaluate_parameters(draws, mean=mean)
            _same(got, want, (name, devices))
            for a, b in zip(sh.coefficients(), wco):
                assert np.array_equal(a, b)
            g = sh.grad_parameters(mean_partial=True)
            for a, b in zip(g, wg):
                assert np.array_equal(a, b), (name, devices)
        finally:
            sh.close()
