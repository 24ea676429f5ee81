# -*- coding: utf-8 -*-
"""The device evaluator (kernel_program_eval_kernel) and its vector-Jacobian kernel (kernel_program_vjp_kernel) on
every opcode and edge shape, against the 60-digit oracle of oracle/kernel_terms.py and its running bound -- one side
at a time, the bars of tests/_kernel_families.py (no constant per kernel, no factor 2; bound / envelope <= 1e-10
asserted for every draw used).

Where each opcode and edge is reached (CASES by name):

  REAL, COMPLEX_B0          "16 temporaries", "all leaves, width 12", "frozen: none left"
  COMPLEX                   "depth 3", "all leaves, width 12", "complex x same"
  SHO_OVER                  "sho over ..." (negative second amplitude), "sho below 1/2 ...", "real + sho over, B = 1000"
  SHO_UNDER                 "sho above 1/2 ...", "all leaves, width 12"
  MATERN32 (reads consts)   "all leaves, width 12", "width 32: products with matern"
  JITTER                    "long program", "all leaves, width 12"
  MUL_RR                    "long program", "depth 3", "16 temporaries", "all leaves, width 12"
  MUL_RC                    "depth 3", "16 temporaries"
  MUL_CC, d1 - d2 <= 0      "complex x same" (= 0), "width 32: products with matern" (d - eps, eps - d < 0), "depth 3"
  frozen parameters         "frozen: none left" (P = 0), "frozen: one left", "long program" (256 constants)
  product of products       "depth 3"
  16 temporaries of a kind  "16 temporaries" (16 real and 16 complex)
  staging loop > once/lane  every program above 64 words: "16 temporaries", "long program" (1088 words: 17 rounds)
  J_comp == 0               "sho over ...", "real + sho over, B = 1000", "long program"
  J_real == 0               "sho above 1/2 ...", "complex x same", "depth 3", "width 32: products with matern"
  narrow / wide plans       widths 2, 3, 4, 8 / 12, 16 ("long program"), 32, 47 ("16 temporaries")
  B in {1, 63, 64, 65, 1000} the SHO cases; B x P not a multiple of 64 with a workgroup over several draws: "16
                            temporaries" (33 x 80), every SHO case with B = 63 or 65 (P = 3)
  P == 0, mean_partial      "frozen: none left": the gradient has shape (B, 1) and is d loglike / d mean
"""
import numpy as np
import pytest

from celerite_amd import batch, terms
from oracle import ref
from _cases import within
import _kernel_families as fam

pytestmark = pytest.mark.gpu

REL = 1e-10     # tests/test_gpu_batch.py: log det, quadratic form and log-likelihood against the oracle
FAMILY = {n: (m, d) for n, m, d in fam.FAMILIES}


def _all_leaves():
    return fam._sum([terms.RealTerm(1.0, 0.1), terms.ComplexTerm(0.1, -1.5, 1.0, 1.6), terms.ComplexTerm(0.2, 1.5, 1.2),
                     terms.SHOTerm(0.1, 1.0, 1.5), terms.Matern32Term(0.1, 0.3), terms.JitterTerm(-2.0),
                     terms.RealTerm(0.2, -0.3) * terms.RealTerm(-0.1, 0.2), terms.SHOTerm(0.1, -2.0, 0.3)])


def _width32():
    """(C + C0) x (C0 + Matern32) + the same the other way round: 16 complex terms; d1 - d2 is positive in the first
    product (d - eps among them) and negative in the second (eps - d); one log_a per product is frozen"""
    def left(s):
        return terms.ComplexTerm(0.1 + s, -1.5, 1.0, 1.6 - s) + terms.ComplexTerm(0.2 - s, 1.5, 1.2 + s)
    def right(s):
        k = terms.ComplexTerm(0.3, 0.4 + s, 0.9) + terms.Matern32Term(0.1 + s, 0.3)
        k.freeze_parameter("terms[0]:log_a")
        return k
    return left(0.0) * right(0.0) + right(0.05) * left(0.05)


def _real_sho_over():
    return terms.RealTerm(1.0, 0.1) + terms.SHOTerm(0.1, -2.0, 0.3)


# (name, kernel factory, draws, J_real, J_comp, B, N)
CASES = []
for (q, B) in ((-1.0, 1), (-2.0, 63), (-3.0, 64), (-5.0, 65)):
    n = "sho over-damped, log Q = %g" % q
    CASES.append(("sho over, log Q = %g, B = %d" % (q, B),) + FAMILY[n] + (2, 0, B, 1024))
for dist, Bb, Ba in ((1e-1, 63, 65), (1e-2, 65, 64), (1e-3, 64, 63)):
    CASES.append(("sho below 1/2 by %g, B = %d" % (dist, Bb),) + FAMILY["sho below Q = 1/2 by %g" % dist] + (2, 0, Bb, 1024))
    CASES.append(("sho above 1/2 by %g, B = %d" % (dist, Ba),) + FAMILY["sho above Q = 1/2 by %g" % dist] + (0, 1, Ba, 1024))
CASES += [
    ("real + sho over, B = 1000", _real_sho_over, fam.spread_draws(), 3, 0, 1000, 1024),
    ("complex x same",) + FAMILY["complex x the same complex (d1 - d2 = 0)"] + (0, 2, 65, 2048),
    ("depth 3",) + FAMILY["product of products, depth 3"] + (0, 2, 63, 2048),
    ("16 temporaries",) + FAMILY["16 real and 16 complex temporaries"] + (15, 16, 33, 1024),
    ("long program",) + FAMILY["sum of more than 1024 words"] + (16, 0, 5, 2048),
    ("frozen: none left",) + FAMILY["every parameter frozen"] + (2, 3, 65, 4096),
    ("frozen: one left",) + FAMILY["every parameter but one frozen"] + (2, 3, 64, 4096),
    ("all leaves, width 12", _all_leaves, fam.spread_draws(), 4, 4, 64, 2048),
    ("width 32: products with matern", _width32, fam.spread_draws(), 0, 16, 17, 2048),
]
IDS = [c[0] for c in CASES]


def _setup(make, draw, JR, JC, B, N, seed=0, cls=batch.BatchedGP, **kw):
    """the series of test_gpu_kernel_params._setup; the draws of the case's own family"""
    rng = np.random.RandomState(seed)
    kernel = make()
    draws = draw(kernel, B)
    t = np.sort(rng.rand(B, N), axis=1)
    diag = rng.uniform(0.1, 0.2, (B, N)) ** 2
    y = np.sin(t) + 0.3
    mean = rng.uniform(0.0, 0.6, B)
    plan = cls(B, N, JR, JC, **kw)
    try:
        plan.set_series(t, diag, y)
        prog = plan.set_kernel(kernel)
        assert (prog.J_real, prog.J_comp) == (JR, JC)
    except BaseException:
        plan.close()
        raise
    return kernel, draws, t, diag, y, mean, plan


def _same(a, b, what):
    for x, z, name in zip(a, b, ("loglike", "logdet", "quad", "status")):
        assert np.array_equal(np.asarray(x), np.asarray(z), equal_nan=(name != "status")), (what, name, x, z)


def test_the_cases_reach_all_ten_opcodes():
    seen = set()
    for name, make, draw, JR, JC, B, N in CASES:
        ops, pc = batch.compile_kernel(make()).ops, 0
        lengths = {1: 4, 2: 6, 3: 5, 4: 6, 5: 5, 6: 5, 7: 2, 8: 4, 9: 4, 10: 5}
        while pc < len(ops):
            seen.add(int(ops[pc]))
            pc += lengths[int(ops[pc])]
    assert seen == set(range(1, 11))
    assert set(c[5] for c in CASES) >= {1, 63, 64, 65, 1000}


@pytest.mark.parametrize("name,make,draw,JR,JC,B,N", CASES, ids=IDS)
def test_same_bits_as_evaluate_on_the_coefficients_read_back(name, make, draw, JR, JC, B, N):
    """The statistics the device forms per draw (smallest / largest rate, largest frequency, jitter) feed the route
    selection exactly as the host's do for tables: same results, same exact_flags -- with negative amplitudes, negative
    or zero d and near-equal rates."""
    kernel, draws, t, diag, y, mean, plan = _setup(make, draw, JR, JC, B, N)
    try:
        for m in (None, mean):
            got = plan.evaluate_parameters(draws, mean=m)
            flags = plan.exact_flags()
            co = plan.coefficients()
            want = plan.evaluate(*co[:6], jitter=co[6], mean=m)
            _same(got, want, (name, "mean" if m is not None else "no mean"))
            assert np.array_equal(flags, plan.exact_flags()), name
            assert (got[3] == 0).all(), (name, got[3])
            assert np.isfinite(got[0]).all(), name
    finally:
        plan.close()


@pytest.mark.parametrize("name,make,draw,JR,JC,B,N", CASES, ids=IDS)
def test_device_coefficients_within_the_oracle_bound(name, make, draw, JR, JC, B, N):
    kernel, draws, t, diag, y, mean, plan = _setup(make, draw, JR, JC, B, N)
    try:
        st = plan.evaluate_parameters(draws)[3]
        assert (st == 0).all()
        co = plan.coefficients()
    finally:
        plan.close()
    table = fam.oracle_table(("gpu", name), kernel, draws)
    fam.check_cap(name, kernel, draws, table)
    worst = fam.check_coefficients(name, co, table)
    print("%s: device coefficients, worst deviation / oracle bound = %.3f" % (name, worst))
    within("device coefficients / oracle bound", worst, 1.0, name)


@pytest.mark.parametrize("name,make,draw,JR,JC,B,N", CASES, ids=IDS)
def test_device_vjp_against_the_oracle_jacobian(name, make, draw, JR, JC, B, N):
    """grad_parameters, with and without the mean's partial, against the oracle Jacobian contracted in Decimal with
    the coefficient gradient the plan itself returns; the mean column is ``dm`` bit for bit (P == 0: shape (B, 1))."""
    kernel, draws, t, diag, y, mean, plan = _setup(make, draw, JR, JC, B, N)
    P = draws.shape[1]
    out = {}
    try:
        for with_mean in (False, True):
            st = plan.evaluate_parameters(draws, mean=mean)[3]
            assert (st == 0).all()
            value, g, gst = plan.grad_parameters(mean_partial=with_mean)
            assert g.shape == (B, P + (1 if with_mean else 0)) and (gst == 0).all()
            if with_mean:
                v2, cg, dm, st2 = plan.grad_log_likelihood(mean_partial=True)
                assert np.array_equal(g[:, P], dm), name
            else:
                v2, cg, st2 = plan.grad_log_likelihood()
            assert np.array_equal(value, v2) and np.array_equal(gst, st2)
            out[with_mean] = (g, cg)
    finally:
        plan.close()
    table = fam.oracle_table(("gpu", name), kernel, draws)
    fam.check_cap(name, kernel, draws, table)
    for with_mean, (g, cg) in out.items():
        worst = fam.check_vjp(name, g[:, :P], cg, table)
        print("%s: grad_parameters(mean_partial=%s), worst deviation / bar = %.3f" % (name, with_mean, worst))
        within("grad_parameters vs oracle Jacobian x plan gradient / bar", worst, 1.0, name)


# ---- refusals ------------------------------------------------------------------------------------------------------
def _refusal_kernel():
    """SHO_OVER + MATERN32 + (R x R) x C0 (a product read as a factor) + R x C with the real term's log_a frozen"""
    k = fam._sum([terms.SHOTerm(0.1, -2.0, 0.3), terms.Matern32Term(0.1, 0.3),
                  (terms.RealTerm(0.2, -0.3) * terms.RealTerm(-0.1, 0.2)) * terms.ComplexTerm(0.2, 1.5, 1.2),
                  terms.RealTerm(0.1, 0.5) * terms.ComplexTerm(0.6, 0.2, 1.0, 1.2)])
    k.freeze_parameter("terms[3]:k1:log_a")
    return k


# parameter order: sho S0 Q w0 | matern sigma rho | R a c, R a c, C0 a c d | R c (a frozen), C a b c d
REFUSED = [
    ("an over-damped SHO draw across Q = 1/2", 3, {1: float(np.log(0.6))}),
    ("a product that overflows only inside a temporary", 9, {5: 400.0, 7: 400.0}),       # exp(400)^2 = inf in the temporary
    ("an exp that underflows a rate to 0", 20, {4: 800.0}),      # matern: w0 = sqrt(3) exp(-800) = 0, S0 = x / 0
    ("a NaN in a parameter", 33, {0: float("nan")}),
    ("a NaN next to a frozen parameter of a product", 47, {12: float("nan")}),
]


@pytest.mark.parametrize("why,row,change", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_draw_is_nan_and_the_others_are_untouched(why, row, change):
    kernel, draws, t, diag, y, mean, plan = _setup(_refusal_kernel, fam.spread_draws(), 2, 3, 64, 2048)
    try:
        assert draws.shape[1] == 17
        for p, x in change.items():
            draws[row, p] = x
        got = plan.evaluate_parameters(draws, mean=mean)
        flags = plan.exact_flags()
        co = plan.coefficients()
        assert all(np.isfinite(c).all() for c in co), why
        # the stand-in of a refused draw (kernel_program.hip): every term exp(-tau), no jitter
        for block, x in zip(co, (1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0)):
            assert (block[row] == x).all(), (why, block[row], x)
        want = plan.evaluate(*co[:6], jitter=co[6], mean=mean)
        assert np.array_equal(flags, plan.exact_flags())
        good = np.delete(np.arange(64), row)
        for x, z in zip(got, want):
            assert np.array_equal(x[good], z[good]), why
        assert got[3][row] == batch.CLR_INVALID_ARGUMENT and (got[3][good] == 0).all()
        assert all(np.isnan(x[row]) for x in got[:3])
        tab = batch.kernel_coefficient_table(kernel, draws[good], compiled=False)
        l0, d0, q0, s0 = ref.batch_log_likelihood(tab[6], *tab[:6], t[good], diag[good], (y - mean[:, None])[good])
        within("refusals: the others' log det vs oracle", np.max(np.abs(got[1][good] - d0) / np.abs(d0)), REL, why)
        within("refusals: the others' quadratic form vs oracle", np.max(np.abs(got[2][good] - q0) / np.abs(q0)), REL, why)
        within("refusals: the others' log-likelihood vs oracle", np.max(np.abs(got[0][good] - l0) / np.abs(l0)), REL, why)
        plan.evaluate_parameters(draws, mean=mean)      # (evaluate() above put table coefficients in force)
        value, g, gst = plan.grad_parameters(mean_partial=True)
        assert gst[row] == batch.CLR_INVALID_ARGUMENT and np.isnan(g[row]).all() and np.isnan(value[row])
        assert np.isfinite(g[good]).all() and (gst[good] == 0).all()
        table = fam.oracle_table(("gpu refusal", why), kernel, draws[good])
        fam.check_cap(why, kernel, draws[good], table)
        fam.check_coefficients(why, [c[good] for c in co], table)
    finally:
        plan.close()


# ---- sharded -------------------------------------------------------------------------------------------------------
def _device_lists():
    n = batch.device_count()
    return [[0, 0, 0]] + ([list(range(n))] if n > 1 else [])


SHARDED = [CASES[IDS.index("complex x same")], CASES[IDS.index("real + sho over, B = 1000")]]


@pytest.mark.parametrize("name,make,draw,JR,JC,B,N", SHARDED, ids=[c[0] for c in SHARDED])
def test_sharded_same_bits_as_the_unsharded_plan(name, make, draw, JR, JC, B, N):
    kernel, draws, t, diag, y, mean, plan = _setup(make, draw, JR, JC, B, N)
    try:
        # a shard and the whole plan must take the same route to give the same bits.  The shards below are given the
        # whole plan's chunk count, and an explicit chunk count pins the pipeline (clr_batch_set_chunks), which keeps
        # the automatic one-launch route of short narrow problems out; the whole plan, which only reads its chunk count,
        # would keep that route (width 4, B = 65), so it is switched off here
        plan.set_small_mode(0)
        nchunk = plan.chunks[0]
        want = plan.evaluate_parameters(draws, mean=mean)
        assert not plan.small_mode_active()
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
                assert np.array_equal(a, b), (name, devices)
            g = sh.grad_parameters(mean_partial=True)
            for a, b in zip(g, wg):
                assert np.array_equal(a, b), (name, devices)
        finally:
            sh.close()
