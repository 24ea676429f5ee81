# -*- coding: utf-8 -*-
"""A ``terms`` kernel compiled into a program (batch.compile_kernel, clr_kernel_*): the host evaluator against the
Python formulas of celerite_amd/terms.py.  No GPU needed.

The bound is DERIVED, not measured.  Both sides evaluate the same formulas with correctly rounded + - * / sqrt and an
``exp`` within 1 ulp (numpy's there, the C library's here), so each side is within ``n`` ulp of the exact value, ``n``
the number of roundings on the longest chain to a coefficient:

  Matern32Term's ``b = w0 w0 S0 / eps``: exp(-log_rho) 1 + the constant sqrt(3) 1 + their product 1 = 3 for w0;
      exp(2 log_sigma) 1, / w0 (1 + 3 + 1) = 5 for S0; w0 w0 (3 + 3 + 1) = 7, times S0 (7 + 5 + 1) = 13, / eps 14.
  SHOTerm's ``a (1 + 1 / f)`` below Q = 1/2: Q 1, Q Q 3, 4 Q Q 3, 1 - 4 Q Q 4, sqrt 3, 1 / f 4, 1 + 1 / f 5, the
      prefactor S0 w0 Q 5, their product 11.  The differences 1 - 4 Q^2, 4 Q^2 - 1, 1 - 1 / f and 1 - f cancel, and a
      cancelling difference is bounded relative to its larger operand.  The factor 4 in LEAF_ULP = 4 x 11 is NOT such
      a bound for ``1 - 1 / f``: at KERNELS' own SHOTerm(0.1, -2.0, 0.3), 1 / f is about 1.039 and the operands are
      about 27 times the difference (a 60-digit restatement measures that amplitude up to 33 ulp of itself off there,
      and far more towards log Q = -3 or Q = 1/2).  The two-sided bar below holds at these draws with a thin margin
      and must not be extended to other regimes; the bar that follows the cancellation of the actual draw is the
      oracle's running bound (oracle/kernel_terms.py), which the one-sided tests at the end of this file use.
  a product level: a1 a2 carries the two factors' counts + 1, complex x complex one more for a1 a2 -+ b1 b2; the
      bound of a difference is relative to the sum of the magnitudes of its operands: |a1 a2| + |b1 b2|, |b1 a2| +
      |a1 b2| and |d1| + |d2| (``_envelope`` computes them with the product algebra on magnitudes).

LEAF_ULP = 44 covers every leaf, a product of two sub-kernels allows the sum of their bounds + 2, and the two sides
together differ by at most twice that."""
import ctypes as C

import numpy as np
import pytest

from celerite_amd import batch, terms
from oracle import kernel_terms
from test_terms import GOLDEN, build
import _kernel_families as fam
from _kernel_families import _envelope, _envelopes     # (test_gpu_kernel_params.py takes them from here)

ULP = 2.0 ** -52
LEAF_ULP = 44        # 4 (cancellation in the SHO formulas, see above) x 11 roundings; >= the 14 of the Matern32 chain


def _bench_kernel():
    """bench.py's kernel shape: 2 real + 3 complex terms (width 8)."""
    k = terms.RealTerm(1.0, 0.1) + terms.RealTerm(0.9, 0.2)
    for j in range(3):
        k = k + terms.ComplexTerm(0.1 + 0.05 * j, 2.0 + 0.1 * j, 1.6 - 0.1 * j)
    return k


def _frozen():
    k = terms.RealTerm(0.1, 0.5) + terms.ComplexTerm(0.6, 0.2, 1.0, 1.2)
    k.freeze_parameter("terms[1]:log_b")
    return k


# (name, kernel factory, levels of products): every built-in term alone, sums, nested products, a frozen parameter,
# eps, SHO in each regime, the bench kernel
KERNELS = [
    ("real", lambda: terms.RealTerm(0.1, 0.5), 0),
    ("complex", lambda: terms.ComplexTerm(0.6, 0.2, 1.0, 1.2), 0),
    ("complex without b", lambda: terms.ComplexTerm(0.6, 1.0, 1.2), 0),
    ("sho under-damped", lambda: terms.SHOTerm(0.1, 1.0, 0.3), 0),
    ("sho over-damped", lambda: terms.SHOTerm(0.1, -2.0, 0.3), 0),
    ("matern32", lambda: terms.Matern32Term(0.1, 0.3), 0),
    ("matern32 eps", lambda: terms.Matern32Term(0.1, 0.3, eps=0.002), 0),
    ("jitter", lambda: terms.JitterTerm(-1.0), 0),
    ("jitter + real + sho", lambda: terms.JitterTerm(-1.0) + terms.RealTerm(0.1, 0.5) + terms.SHOTerm(0.1, 1.0, 0.3), 0),
    ("real x real", lambda: terms.RealTerm(0.1, 0.5) * terms.RealTerm(0.2, 0.3), 1),
    ("real x complex", lambda: terms.RealTerm(0.1, 0.5) * terms.ComplexTerm(0.6, 0.2, 1.0, 1.2), 1),
    ("complex x real", lambda: terms.ComplexTerm(0.6, 0.2, 1.0, 1.2) * terms.RealTerm(0.1, 0.5), 1),
    ("complex x complex", lambda: terms.ComplexTerm(0.3, -1.0, 0.2, 0.7) * terms.ComplexTerm(0.6, 0.2, 1.0, 1.2), 1),
    ("product of sums", lambda: (terms.RealTerm(0.1, 0.5) + terms.SHOTerm(0.1, 1.0, 0.3)) *
     (terms.RealTerm(0.3, 0.1) + terms.ComplexTerm(0.6, 0.2, 1.0, 1.2)), 1),
    ("nested product + sum", lambda: (terms.RealTerm(0.1, 0.5) * terms.ComplexTerm(0.6, 1.0, 1.2)) *
     terms.Matern32Term(0.1, 0.3) + terms.RealTerm(0.0, 0.0) + terms.JitterTerm(-2.0), 2),
    ("frozen parameter", _frozen, 0),
    ("bench kernel", _bench_kernel, 0),
]
IDS = [k[0] for k in KERNELS]


def _bound(depth):
    """ulp per side for a kernel with `depth` levels of products: b(0) = LEAF_ULP, b(d) = 2 b(d - 1) + 2"""
    b = LEAF_ULP
    for _ in range(depth):
        b = 2 * b + 2
    return b


def _draws(kernel, B=96, seed=3, spread=0.1):
    """random draws around the kernel's parameters; 0.1, clipped at 3 sigma, keeps every SHO term of KERNELS 0.3 away
    from Q = 1/2 in log Q"""
    rng = np.random.RandomState(seed)
    p0 = kernel.get_parameter_vector()
    return p0[None, :] + spread * np.clip(rng.randn(B, len(p0)), -3, 3)


def _close(got, want, scale, nulp, what):
    """|got - want| <= 2 sides x nulp ulp x scale"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.size == 0:
        return
    dev = np.abs(got - want)
    assert (dev <= 2 * nulp * ULP * scale).all(), (what, float(np.max(dev / np.maximum(scale, 1e-300)) / ULP), 2 * nulp)


@pytest.mark.parametrize("name,make,depth", KERNELS, ids=IDS)
def test_compiled_table_equals_the_python_loop(name, make, depth):
    kernel = make()
    saved = kernel.get_parameter_vector().copy()
    draws = _draws(kernel)
    want = batch.kernel_coefficient_table(kernel, draws, compiled=False)
    got = batch.kernel_coefficient_table(kernel, draws, compiled=True)
    auto = batch.kernel_coefficient_table(kernel, draws, compiled=None)
    assert len(got) == 7
    scales = _envelopes(kernel, draws) + [np.abs(want[6])]
    for g, a, w, s, block in zip(got, auto, want, scales, ("a_real", "c_real", "a_comp", "b_comp", "c_comp", "d_comp", "jitter")):
        _close(g, w, s, _bound(depth), (name, block))
        assert np.array_equal(g, a)
    assert np.array_equal(saved, kernel.get_parameter_vector())     # the kernel's own parameters are untouched


@pytest.mark.parametrize("name,make,depth", KERNELS, ids=IDS)
def test_compiled_jacobian_equals_the_python_loop(name, make, depth):
    """The same formulas on duals, in the same order on both sides.  A derivative's chain is the value's chain with
    one more product and sum per step (the product and quotient rules): twice the value's count.  Its terms are products
    of a coefficient-sized value and a derivative of unit size (the parameters are logarithms: d exp(p) / dp = exp(p)),
    so the bound is relative to the coefficient's envelope or to the largest entry of that coefficient's column of the
    Python Jacobian, whichever is larger (the SHO derivatives carry factors 1 / f^2 > 1)."""
    kernel = make()
    saved = kernel.get_parameter_vector().copy()
    draws = _draws(kernel)
    jw, jjw = batch.kernel_coefficient_jacobian_table(kernel, draws, compiled=False)
    jg, jjg = batch.kernel_coefficient_jacobian_table(kernel, draws, compiled=True)
    assert jg.shape == jw.shape and jjg.shape == jjw.shape
    scale = np.ones_like(jw)
    if jw.size:
        env = np.concatenate(_envelopes(kernel, draws), axis=1)[:, None, :]
        scale = np.maximum(np.max(np.abs(jw), axis=1, keepdims=True), env) * np.ones_like(jw)
    _close(jg, jw, scale, 2 * _bound(depth), (name, "jac"))
    _close(jjg, jjw, np.abs(jjw), 2 * _bound(depth), (name, "jitter_jac"))
    # chain_gradient on either table: a dot product of C + 1 terms, each within the bound above, + C + 1 roundings
    rng = np.random.RandomState(11)
    grad = rng.randn(draws.shape[0], 1 + jw.shape[2])
    cw = batch.chain_gradient(grad, jw, jjw)
    cg = batch.chain_gradient(grad, jg, jjg)
    env = np.einsum("bpc,bc->bp", scale, np.abs(grad[:, 1:])) + np.abs(jjw * grad[:, :1])
    _close(cg, cw, env, 2 * _bound(depth) + grad.shape[1], (name, "chain_gradient"))
    assert np.array_equal(saved, kernel.get_parameter_vector())


@pytest.mark.parametrize("key", sorted(GOLDEN))
def test_against_the_reference_golden_values(key):
    """tests/golden/terms_golden.json: the reference's coefficients for its kernels, at the stored parameters (every
    kernel there has at most two levels of products)."""
    kernel = build(key)
    want = GOLDEN[key]
    p = kernel.get_parameter_vector()
    got = batch.kernel_coefficient_table(kernel, p[None, :], compiled=True)
    env = _envelopes(kernel, p[None, :])
    for g, w, s in zip(got[:6], want["coefficients"], env):
        _close(g, np.asarray(w, dtype=float).reshape(1, -1), s, _bound(2), key)
    _close(got[6], np.array([want["jitter"]]), np.array([abs(want["jitter"])]), _bound(0), key)
    assert np.array_equal(p, kernel.get_parameter_vector())


def test_sho_draw_across_the_regime_is_an_error_for_that_row_only():
    kernel = terms.SHOTerm(0.1, 1.0, 0.3) + terms.RealTerm(0.2, 0.1)
    prog = batch.compile_kernel(kernel)
    assert (prog.J_real, prog.J_comp) == (1, 1)
    draws = _draws(kernel, B=64)
    bad = [5, 40]
    draws[bad, 1] = np.log(0.3)         # Q < 1/2: two real terms, another shape
    out = prog.coefficients(draws, status=True)
    st = out[7]
    assert (st[bad] == batch.CLR_INVALID_ARGUMENT).all() and (np.delete(st, bad) == 0).all()
    good = np.delete(np.arange(64), bad)
    want = batch.kernel_coefficient_table(kernel, draws[good], compiled=False)
    for g, w in zip(out[:7], want):
        _close(g[good], w, np.abs(w), _bound(0), "good rows")
        assert np.isnan(g[bad]).all()
    jac, jj, jst = prog.jacobian(draws, status=True)
    assert np.array_equal(jst, st) and np.isnan(jac[bad]).all() and np.isfinite(jac[good]).all()
    with pytest.raises(ValueError):     # as the Python loop does when draws disagree on the shape
        batch.kernel_coefficient_table(kernel, draws, compiled=True)
    with pytest.raises(ValueError):
        batch.kernel_coefficient_table(kernel, draws, compiled=False)
    nan = _draws(kernel, B=4)
    nan[2, 0] = np.nan
    assert list(prog.coefficients(nan, status=True)[7]) == [0, 0, batch.CLR_INVALID_ARGUMENT, 0]
    # the other regime compiles to the other shape
    kernel.set_parameter_vector(draws[5])
    assert (batch.compile_kernel(kernel).J_real, batch.compile_kernel(kernel).J_comp) == (3, 0)


def test_overridden_formulas_cannot_be_compiled():
    class Scaled(terms.RealTerm):
        def get_real_coefficients(self, params):
            return 2.0 * np.exp(params[0]), np.exp(params[1])

    class Custom(terms.Term):
        parameter_names = ("log_a", )

        def get_real_coefficients(self, params):
            return np.exp(params[0]), 1.0

    for bad, cls in ((Scaled(0.1, 0.2), "RealTerm"), (Custom(0.3), "Custom"),
                     (terms.RealTerm(0.0, 0.1) + Scaled(0.1, 0.2), "RealTerm"),
                     (terms.ComplexTerm(0.1, 0.2, 0.3) * Custom(0.3), "Custom")):
        with pytest.raises(ValueError) as err:
            batch.compile_kernel(bad)
        assert cls in str(err.value)    # (the term is named by its repr)
        p = bad.get_parameter_vector()[None, :]
        with pytest.raises(ValueError):
            batch.kernel_coefficient_table(bad, p, compiled=True)
        # compiled=None keeps the Python tables for such a kernel
        auto = batch.kernel_coefficient_table(bad, p, compiled=None)
        assert all(np.array_equal(a, w) for a, w in zip(auto, batch.kernel_coefficient_table(bad, p)))


MALFORMED = [
    ("unknown opcode", [99, 0, 0, 0], 2, 1, 0),
    ("truncated instruction", [1, 0, 0], 2, 1, 0),
    ("parameter index out of range", [1, 0, 0, 2], 2, 1, 0),
    ("constant index out of range", [1, 0, 0, -1], 2, 1, 0),
    ("output term out of range", [1, 1, 0, 1], 2, 1, 0),
    ("output term written twice", [1, 0, 0, 1, 1, 0, 0, 1], 2, 1, 0),
    ("output term never written", [1, 0, 0, 1], 2, 2, 0),
    ("temporary read before it is written", [8, 0, 0, 1, 1, -1, 0, 1, 1, -2, 0, 1], 2, 1, 0),
    ("temporary out of range", [1, -17, 0, 1, 1, 0, 0, 1], 2, 1, 0),
    ("complex output missing", [1, 0, 0, 1], 2, 1, 1),
]


@pytest.mark.parametrize("why,ops,n_params,J_real,J_comp", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_program_is_refused(why, ops, n_params, J_real, J_comp):
    lib = batch._load()
    ops = np.asarray(ops, dtype=np.int32)
    k = C.c_void_p()
    st = lib.clr_kernel_create(len(ops), ops.ctypes.data_as(C.POINTER(C.c_int)), 0, None, n_params, J_real, J_comp, C.byref(k))
    assert st == batch.CLR_INVALID_ARGUMENT and not k.value, why


def test_a_well_formed_program_by_hand():
    """real x real through two temporaries, written by hand in the documented encoding"""
    lib = batch._load()
    ops = np.asarray([1, -1, 0, 1, 1, -2, 2, 3, 8, 0, 0, 1], dtype=np.int32)
    k = C.c_void_p()
    assert lib.clr_kernel_create(len(ops), ops.ctypes.data_as(C.POINTER(C.c_int)), 0, None, 4, 1, 0, C.byref(k)) == 0
    p = np.array([[0.1, 0.2, 0.3, 0.4]])
    a, c, jit = np.empty((1, 1)), np.empty((1, 1)), np.empty(1)
    st = np.empty(1, dtype=np.int32)
    dp = C.POINTER(C.c_double)
    assert lib.clr_kernel_coefficients(k, 1, p.ctypes.data_as(dp), a.ctypes.data_as(dp), c.ctypes.data_as(dp), None, None,
                                       None, None, jit.ctypes.data_as(dp), st.ctypes.data_as(C.POINTER(C.c_int))) == 0
    lib.clr_kernel_destroy(k)
    assert st[0] == 0 and jit[0] == 0.0
    assert abs(a[0, 0] - np.exp(0.1) * np.exp(0.3)) <= 3 * ULP * a[0, 0]
    assert abs(c[0, 0] - (np.exp(0.2) + np.exp(0.4))) <= 3 * ULP * c[0, 0]


# ---- one side at a time against the 60-digit oracle and its running bound (oracle/kernel_terms.py) ------------------
ORACLE_CASES = [(n, m, fam.spread_draws()) for n, m, _ in KERNELS] + fam.FAMILIES
ORACLE_IDS = [c[0] for c in ORACLE_CASES]
ORACLE_B = {"sum of more than 1024 words": 6, "16 real and 16 complex temporaries": 24}     # (default 96)


def _oracle_case(name, make, draw):
    kernel = make()
    draws = draw(kernel, ORACLE_B.get(name, 96))
    return kernel, draws, fam.oracle_table(("cpu", name), kernel, draws)


@pytest.mark.parametrize("key", sorted(GOLDEN))
def test_oracle_against_the_reference_golden_values(key):
    """Pins the oracle: the stored values are doubles a double evaluation of these formulas produced (the file keeps
    17 significant digits, which round-trip a double exactly), so each lies within the oracle's bound of the oracle's
    value -- no further allowance."""
    kernel = build(key)
    want = GOLDEN[key]
    r = kernel_terms.evaluate(kernel)
    flat = np.concatenate([np.asarray(w, dtype=float).reshape(-1) for w in want["coefficients"]])
    assert len(flat) == len(r.value)
    for c, (w, v, e) in enumerate(zip(flat, r.value, r.bound)):
        assert kernel_terms.deviation(w, v) <= e, (key, c, w, v, e)
    assert kernel_terms.deviation(want["jitter"], r.jitter) <= r.jitter_bound


@pytest.mark.parametrize("name,make,draw", ORACLE_CASES, ids=ORACLE_IDS)
def test_oracle_bounds_the_python_loop_and_stays_below_the_cap(name, make, draw):
    """Pins the oracle from the other side: numpy's evaluation of terms.py (values and dual-number Jacobian) is a
    double evaluation of the same operation sequence, so it must lie within the bound -- for every KERNELS entry and
    every new family; and the bound itself is at most CAP = 1e-10 of the column's envelope for every draw."""
    kernel, draws, table = _oracle_case(name, make, draw)
    cap = fam.check_cap(name, kernel, draws, table)
    want = batch.kernel_coefficient_table(kernel, draws, compiled=False)
    jw, jjw = batch.kernel_coefficient_jacobian_table(kernel, draws, compiled=False)
    w = fam.check_coefficients(name, want, table)
    wj = fam.check_jacobian(name, jw.reshape(len(draws), draws.shape[1], len(table[0].value)), jjw, table)
    print("%s: python loop / oracle bound: coefficients %.3f, Jacobian %.3f; bound / envelope %.2e" % (name, w, wj, cap))


@pytest.mark.parametrize("name,make,draw", ORACLE_CASES, ids=ORACLE_IDS)
def test_host_evaluator_within_the_oracle_bound(name, make, draw):
    """clr_kernel_coefficients and clr_kernel_jacobian against the oracle alone: draw by draw, column by column,
    |computed - oracle| <= the oracle's bound for that draw (u per + - * / sqrt, 1 ulp per exp)."""
    kernel, draws, table = _oracle_case(name, make, draw)
    saved = kernel.get_parameter_vector().copy()
    fam.check_cap(name, kernel, draws, table)
    prog = batch.compile_kernel(kernel)
    assert prog.n_params == draws.shape[1] and (prog.J_real, prog.J_comp) == table[0].shape
    w = fam.check_coefficients(name, prog.coefficients(draws), table)
    jac, jj = prog.jacobian(draws)
    wj = fam.check_jacobian(name, jac, jj, table)
    # the chain rule on the host Jacobian against the oracle Jacobian contracted in Decimal: the bar of check_vjp
    grad = np.random.RandomState(11).randn(draws.shape[0], 1 + jac.shape[2])
    wc = fam.check_vjp(name, batch.chain_gradient(grad, jac, jj), grad, table)
    print("%s: host evaluator / oracle bound: coefficients %.3f, Jacobian %.3f, chain_gradient / bar %.3f" % (name, w, wj, wc))
    assert np.array_equal(saved, kernel.get_parameter_vector())


def test_the_new_families_reach_the_program_limits():
    progs = {n: batch.compile_kernel(m()) for n, m, _ in fam.FAMILIES}
    ops = lambda n: list(progs[n].ops)
    count = lambda n, op: sum(1 for w in _instructions(ops(n)) if w[0] == op)
    assert all(count(n, 4) == 1 for n in progs if n.startswith("sho over") or n.startswith("sho below"))
    assert all(count(n, 5) == 1 for n in progs if n.startswith("sho above"))
    assert count("complex x the same complex (d1 - d2 = 0)", 10) == 1
    deep = _instructions(ops("product of products, depth 3"))
    assert [w[0] for w in deep if w[0] >= 8] == [9, 9, 10, 8, 9, 9]
    assert any(w[0] == 10 and w[1] < 0 and w[2] < 0 for w in deep)           # a product written to temporaries ...
    assert any(w[0] == 9 and w[1] >= 0 and w[3] >= 2 for w in deep)          # ... and read as a factor
    t16 = _instructions(ops("16 real and 16 complex temporaries"))
    assert sorted(-w[1] for w in t16 if w[0] == 1) == list(range(1, 17))
    assert sorted(-w[1] for w in t16 if w[0] == 3) == list(range(1, 17))
    long = progs["sum of more than 1024 words"]
    assert 1024 < len(long.ops) <= 2048 and long.n_params == 256 and len(long.consts) == 256
    assert (long.J_real, long.J_comp) == (16, 0)
    assert progs["every parameter frozen"].n_params == 0 and progs["every parameter but one frozen"].n_params == 1
    assert min(progs["every parameter frozen"].ops) < 0


def _instructions(ops):
    lengths = {1: 4, 2: 6, 3: 5, 4: 6, 5: 5, 6: 5, 7: 2, 8: 4, 9: 4, 10: 5}
    out, pc = [], 0
    while pc < len(ops):
        out.append([int(w) for w in ops[pc:pc + lengths[int(ops[pc])]]])
        pc += lengths[int(ops[pc])]
    return out


@pytest.mark.parametrize("n_real,n_comp", [(17, 16), (16, 17)])
def test_seventeen_temporaries_of_one_kind_cannot_be_compiled(n_real, n_comp):
    with pytest.raises(ValueError):
        batch.compile_kernel(fam.temporaries(n_real, n_comp)())


def test_the_first_program_past_the_length_limit_is_refused_not_truncated():
    """CLR_KP_MAX_OPS = 2048 words: 1024 jitter instructions on one parameter are accepted and ALL of them run
    (jitter = 1024 exp(2 p): 1023 additions of one value, each within u of a partial sum <= 1024 exp(2 p), + the
    exp's 1 ulp); one instruction more is refused by clr_kernel_create.  A ``terms`` kernel past a limit raises too."""
    prog = batch.CompiledKernel(None, [7, 0] * 1024, [], 1, 0, 0)
    p = 0.3
    jit = prog.coefficients(np.array([[p]]))[6][0]
    want = 1024 * np.exp(2 * p)
    assert abs(jit - want) <= (1023 * 2.0 ** -53 + 2.0 ** -52) * want * (1 + 2.0 ** -40)
    with pytest.raises(RuntimeError):
        batch.CompiledKernel(None, [7, 0] * 1025, [], 1, 0, 0)
    lib = batch._load()
    ops = np.asarray([7, 0] * 1025, dtype=np.int32)
    k = C.c_void_p()
    st = lib.clr_kernel_create(len(ops), ops.ctypes.data_as(C.POINTER(C.c_int)), 0, None, 1, 0, 0, C.byref(k))
    assert st == batch.CLR_INVALID_ARGUMENT and not k.value
    too_many = fam._sum([terms.JitterTerm(-3.0) for _ in range(257)])        # 257 parameters
    with pytest.raises(RuntimeError):
        batch.compile_kernel(too_many)
