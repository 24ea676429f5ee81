# -*- coding: utf-8 -*-
"""Kernel families and the one-sided checks against oracle/kernel_terms.py that test_kernel_program_cpu.py (the host
evaluator) and test_gpu_kernel_program_device.py (the device evaluator and its vector-Jacobian kernel) share.

Every check here is ONE side against the oracle: |computed - oracle value| <= the oracle's own running bound for a
double evaluation of that draw (no constant per kernel, no factor 2).  ``CAP`` keeps the bound honest: for every draw
and column it must stay below 1e-10 of the column's envelope (``REL`` of test_gpu_batch.py against the oracle), so a
bound blown up by a cancellation cannot hide a wrong coefficient -- the draws are chosen so that this holds."""
from decimal import Decimal

import numpy as np

from celerite_amd import terms
from oracle import kernel_terms as kt

CAP = 1e-10
LOG_HALF = float(np.log(0.5))


def _sum(parts):
    k = parts[0]
    for t in parts[1:]:
        k = k + t
    return k


def spread_draws(scale=0.1, per_parameter=None, copy=None):
    """draws around the kernel's parameters: ``scale`` (or ``per_parameter[i]``) x a normal clipped at 3 sigma;
    ``copy = (dst slice, src slice)`` makes two groups of parameters identical in every draw"""
    def draw(kernel, B, seed=3):
        rng = np.random.RandomState(seed)
        p0 = kernel.get_parameter_vector()
        s = np.full(len(p0), scale)
        for i, v in (per_parameter or {}).items():
            s[i] = v
        d = p0[None, :] + s[None, :] * np.clip(rng.randn(B, len(p0)), -3, 3)
        if copy is not None:
            d[:, copy[0]] = d[:, copy[1]]
        return d
    return draw


def _cc_same():
    return terms.ComplexTerm(0.3, 0.29, 0.7, 0.2) * terms.ComplexTerm(0.3, 0.29, 0.7, 0.2)


def _depth3():
    """((R x C) x (R x C0)) x (R x R): temporaries of both kinds are read as factors at two levels"""
    a = terms.RealTerm(0.1, 0.5) * terms.ComplexTerm(0.6, 0.2, 1.0, 1.2)
    b = terms.RealTerm(-0.2, 0.1) * terms.ComplexTerm(0.3, 0.4, 0.9)
    return (a * b) * (terms.RealTerm(0.2, -0.3) * terms.RealTerm(-0.1, 0.2))


def temporaries(n_real, n_comp):
    """(n_real - 1 real + n_comp complex terms) x one real term: n_real real and n_comp complex temporaries"""
    def make():
        parts = [terms.RealTerm(0.1 - 0.03 * j, 0.5 - 0.05 * j) for j in range(n_real - 1)]
        parts += [terms.ComplexTerm(0.2 - 0.02 * j, 1.0 + 0.04 * j, 1.4 - 0.05 * j) for j in range(n_comp)]
        return _sum(parts) * terms.RealTerm(0.3, -0.2)
    return make


def _long_sum():
    """(4 real) x (4 real) + 240 jitter terms + 256 frozen jitter terms: 1088 program words, 256 parameters, 256
    constants, 16 real output terms and no complex one -- every limit of clr_kernel_create but CLR_KP_MAX_OPS reached"""
    four = lambda s: _sum([terms.RealTerm(s + 0.1 * j, 0.2 * j - s) for j in range(4)])
    k = _sum([four(0.1) * four(-0.2)] + [terms.JitterTerm(-3.0 - 0.01 * j) for j in range(496)])
    for j in range(240, 496):
        k.freeze_parameter("terms[%d]:log_sigma" % (1 + j))
    return k


def _bench():
    parts = [terms.RealTerm(1.0, 0.1), terms.RealTerm(0.9, 0.3)]
    parts += [terms.ComplexTerm(0.1 - 0.02 * j, 2.0 + 0.05 * j, 1.6 - 0.06 * j) for j in range(3)]
    return _sum(parts)


def frozen(all_but=None):
    def make():
        k = _bench()
        for i, name in enumerate(k.get_parameter_names()):
            if i != all_but:
                k.freeze_parameter(name)
        return k
    return make


# (name, kernel factory, draws)
FAMILIES = [("sho over-damped, log Q = %g" % q, (lambda q=q: terms.SHOTerm(0.1, q, 0.3)), spread_draws())
            for q in (-1.0, -2.0, -3.0, -5.0)]
for dist in (1e-1, 1e-2, 1e-3):     # both sides of Q = 1/2; log Q itself moves by at most 0.3 of the distance
    for side, sign in (("below", -1.0), ("above", 1.0)):
        FAMILIES.append(("sho %s Q = 1/2 by %g" % (side, dist),
                         (lambda x=LOG_HALF + sign * dist: terms.SHOTerm(0.1, x, 0.3)),
                         spread_draws(per_parameter={1: 0.1 * dist})))
FAMILIES += [
    ("complex x the same complex (d1 - d2 = 0)", _cc_same, spread_draws(copy=(slice(4, 8), slice(0, 4)))),
    ("product of products, depth 3", _depth3, spread_draws()),
    ("16 real and 16 complex temporaries", temporaries(16, 16), spread_draws()),
    ("sum of more than 1024 words", _long_sum, spread_draws()),
    ("every parameter frozen", frozen(), spread_draws()),
    ("every parameter but one frozen", frozen(all_but=5), spread_draws()),
]
FAMILY_IDS = [f[0] for f in FAMILIES]

_TABLES = {}


def oracle_table(key, kernel, draws):
    """oracle Results (with the Jacobian) of the draws, computed once per session and ``key``"""
    draws = np.asarray(draws, dtype=np.float64)
    hit = _TABLES.get(key)
    if hit is None or not np.array_equal(hit[0], draws, equal_nan=True):
        hit = (draws.copy(), kt.table(kernel, draws, jacobian=True))
        _TABLES[key] = hit
    return hit[1]


def _envelope(term, full):
    """The six blocks of ``term`` at the full parameter vector ``full`` with every difference of the product algebra
    replaced by the sum of its operands' magnitudes: what a rounding error of the operands is relative to."""
    if isinstance(term, terms.TermSum):
        per = [_envelope(sub, p) for sub, p in term._split(full)]
        return [np.concatenate(blocks) for blocks in zip(*per)]
    if isinstance(term, terms.TermProduct):
        k1, k2 = term.models["k1"], term.models["k2"]
        ar1, cr1, ac1, bc1, cc1, dc1 = _envelope(k1, full[:k1.full_size])
        ar2, cr2, ac2, bc2, cc2, dc2 = _envelope(k2, full[k1.full_size:])
        ar, cr, ac, bc, cc, dc = [], [], [], [], [], []
        for a1, c1 in zip(ar1, cr1):
            for a2, c2 in zip(ar2, cr2):
                ar.append(a1 * a2), cr.append(c1 + c2)
        for (ra, rc), cs in (((ar1, cr1), (ac2, bc2, cc2, dc2)), ((ar2, cr2), (ac1, bc1, cc1, dc1))):
            for a1, c1 in zip(ra, rc):
                for a2, b2, c2, d2 in zip(*cs):
                    ac.append(a1 * a2), bc.append(a1 * b2), cc.append(c1 + c2), dc.append(d2)
        for a1, b1, c1, d1 in zip(ac1, bc1, cc1, dc1):
            for a2, b2, c2, d2 in zip(ac2, bc2, cc2, dc2):
                for _ in range(2):
                    ac.append(0.5 * (a1 * a2 + b1 * b2)), bc.append(0.5 * (b1 * a2 + a1 * b2))
                    cc.append(c1 + c2), dc.append(d1 + d2)
        return [np.array(x, dtype=float) for x in (ar, cr, ac, bc, cc, dc)]
    return [np.abs(np.atleast_1d(np.asarray(b, dtype=float))) for b in term.get_all_coefficients(full)]


def _envelopes(kernel, draws):
    saved = kernel.get_parameter_vector()
    rows = []
    try:
        for p in draws:
            kernel.set_parameter_vector(p)
            rows.append(_envelope(kernel, kernel.get_parameter_vector(include_frozen=True)))
    finally:
        kernel.set_parameter_vector(saved)
    return [np.array([r[i] for r in rows]).reshape(len(rows), -1) for i in range(6)]


def envelopes(kernel, draws):
    """(B, NC) envelope of every coefficient, the six blocks side by side"""
    return np.concatenate(_envelopes(kernel, draws), axis=1).reshape(len(draws), -1)


def check_cap(name, kernel, draws, table):
    """bound / envelope <= CAP for every draw and column, the jitter included; returns the worst ratio"""
    env = envelopes(kernel, draws)
    worst = 0.0
    for b, r in enumerate(table):
        for c, e in enumerate(r.bound):
            if e != 0:
                assert env[b, c] > 0, (name, b, c)
                worst = max(worst, float(e) / env[b, c])
        if r.jitter_bound != 0:
            worst = max(worst, float(r.jitter_bound / abs(r.jitter)))
    assert worst <= CAP, (name, "oracle bound / envelope", worst, CAP)
    return worst


def _ratio(got, value, bound, where):
    dev = kt.deviation(got, value)
    if bound == 0:
        assert dev == 0, where + (got, value)
        return 0.0
    return float(dev / bound)


def check_coefficients(name, got, table):
    """the seven arrays ``got`` (a_real .. d_comp, jitter) within the oracle's bound, draw by draw and column by
    column; returns the worst deviation / bound"""
    flat = np.concatenate([np.asarray(g, dtype=np.float64).reshape(len(table), -1) for g in got[:6]], axis=1)
    jit = np.asarray(got[6], dtype=np.float64)
    worst = 0.0
    for b, r in enumerate(table):
        assert flat.shape[1] == len(r.value), (name, flat.shape, len(r.value))
        assert (got[0].shape[1], got[2].shape[1]) == r.shape, name
        for c in range(flat.shape[1]):
            worst = max(worst, _ratio(flat[b, c], r.value[c], r.bound[c], (name, "draw", b, "column", c)))
        worst = max(worst, _ratio(jit[b], r.jitter, r.jitter_bound, (name, "draw", b, "jitter")))
    assert worst <= 1.0, (name, "coefficients: deviation / oracle bound", worst)
    return worst


def check_jacobian(name, jac, jitter_jac, table):
    """``jac[B, P, NC]``, ``jitter_jac[B, P]`` within the oracle's Jacobian bound; returns the worst deviation / bound"""
    worst = 0.0
    for b, r in enumerate(table):
        assert jac.shape[1:] == (len(r.jac), len(r.value)), (name, jac.shape)
        for p in range(jac.shape[1]):
            for c in range(jac.shape[2]):
                worst = max(worst, _ratio(jac[b, p, c], r.jac[p][c], r.jac_bound[p][c], (name, "draw", b, "d", c, "/ d", p)))
            worst = max(worst, _ratio(jitter_jac[b, p], r.jitter_jac[p], r.jitter_jac_bound[p], (name, "draw", b, "d jitter / d", p)))
    assert worst <= 1.0, (name, "Jacobian: deviation / oracle bound", worst)
    return worst


def check_vjp(name, g, cg, table):
    """``g[B, P]`` (grad_parameters) against the oracle Jacobian contracted in Decimal with the coefficient gradient
    ``cg[B, 1 + NC]`` the plan returned.  Bar: sum_c jac_bound[p][c] |cg[c]| (+ the jitter's) and the dot product's own
    (C + 1) u sum |terms|, C = NC + 1 products summed one after the other.  Returns the worst deviation / bar."""
    worst = 0.0
    for b, r in enumerate(table):
        w = [Decimal(float(x)) for x in cg[b]]
        for p in range(len(r.jac)):
            want = r.jitter_jac[p] * w[0]
            mag = abs(want)
            bar = r.jitter_jac_bound[p] * abs(w[0])
            for c in range(len(r.value)):
                term = r.jac[p][c] * w[1 + c]
                want += term
                mag += abs(term)
                bar += r.jac_bound[p][c] * abs(w[1 + c])
            bar += (len(r.value) + 2) * kt.U * mag
            worst = max(worst, _ratio(g[b, p], want, bar, (name, "draw", b, "parameter", p)))
    assert worst <= 1.0, (name, "grad_parameters: deviation / bar", worst)
    return worst
