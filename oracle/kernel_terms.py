# -*- coding: utf-8 -*-
"""High-precision oracle for the coefficients of a ``terms`` kernel and their Jacobian, with a running error bound.

The formulas are the ones of celerite_amd/terms.py (and of the compiled evaluator, csrc/clr_kernel_program.h, which
writes the same operation sequence down once more): restated here on ``decimal.Decimal`` at 60 digits, so that the
result is the exact value of the formula for every practical purpose (the working precision is 44 decimal orders
below a double's).

Next to every intermediate a BOUND is carried on what an IEEE double evaluation of the same operation sequence may be
off by.  With ``u = 2^-53`` and x~ = x + dx the computed operands (|dx| <= ex):

    x + y, x - y   e = ex + ey + u (|x +- y| + ex + ey)          one correctly rounded operation
    x y            e = m + u (|x y| + m),   m = |x| ey + |y| ex + ex ey
    x / y          e = m + u (|x / y| + m), m = (ex + |x / y| ey) / (|y| - ey)
    sqrt x         e = m + u (sqrt x + m),  m = sqrt x - sqrt(x - ex)
    exp x          e = m + 2 u (exp x + m), m = exp x (exp(ex) - 1)      1 ulp <= 2 u relative: the figure the project
                                                                         states for the host's and the device's exp
                                                                         (clr_kernel_program.h, kernel_program.hip)
    a power of two times x: exact (0.5 x, 2 x, 4 x; no rounding is charged)

These are the standard first-order rules with their second-order terms kept, so the bound is a true bound and not an
estimate.  A difference that cancels keeps the absolute errors of its operands: the bound follows the cancellation of
the actual draw (SHOTerm's ``1 - 1 / f`` and ``1 - f`` near Q = 0 and near Q = 1/2, ``a1 a2 - b1 b2`` of a product)
instead of assuming one.  Parameters and ``eps`` are doubles and enter exactly; ``sqrt(3)`` of Matern32Term is exact
here and a correctly rounded constant on the double side (one u).

The Jacobian is the same tree on duals over these bounded numbers: value + derivative along every unfrozen parameter,
with the product, quotient, exp and sqrt rules written as the evaluators write them (``a.v b.d + b.v a.d``,
``(a.d - q b.d) / b.v``, ``e a.d``, ``a.d / (2 r)``), so the derivative's bound is that of the evaluators' sequence.
"""
import decimal
from decimal import Decimal

import numpy as np

from celerite_amd import terms

CTX = decimal.Context(prec=60, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
U = Decimal(2) ** -53
_ZERO, _ONE, _TWO = Decimal(0), Decimal(1), Decimal(2)
_POW2 = set(Decimal(2) ** k for k in range(-4, 5))
BLOCKS = ("a_real", "c_real", "a_comp", "b_comp", "c_comp", "d_comp")


class Num(object):
    """``v``: the value at 60 digits; ``e``: bound on |double evaluation - v|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=_ZERO):
        self.v = v if isinstance(v, Decimal) else Decimal(float(v))
        self.e = e

    @staticmethod
    def of(x):
        return x if isinstance(x, Num) else Num(x)

    def _exact_scale(self):
        return self.e == 0 and abs(self.v) in _POW2

    def __add__(self, o):
        o = Num.of(o)
        if o.e == 0 and o.v == 0:       # x + 0.0 is x
            return self
        if self.e == 0 and self.v == 0:
            return o
        v = CTX.add(self.v, o.v)
        m = self.e + o.e
        return Num(v, CTX.add(m, CTX.multiply(U, abs(v) + m)))
    __radd__ = __add__

    def __neg__(self):
        return Num(-self.v, self.e)

    def __sub__(self, o):
        return self + (-Num.of(o))

    def __rsub__(self, o):
        return Num.of(o) + (-self)

    def __mul__(self, o):
        o = Num.of(o)
        v = CTX.multiply(self.v, o.v)
        m = abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e
        if self._exact_scale() or o._exact_scale() or v == 0 and m == 0:
            return Num(v, m)
        return Num(v, CTX.add(m, CTX.multiply(U, abs(v) + m)))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Num.of(o)
        v = CTX.divide(self.v, o.v)
        if not abs(o.v) > o.e:
            raise ArithmeticError("the bound of a divisor reaches zero")
        m = CTX.divide(self.e + abs(v) * o.e, abs(o.v) - o.e)
        if o._exact_scale() or v == 0 and m == 0:
            return Num(v, m)
        return Num(v, CTX.add(m, CTX.multiply(U, abs(v) + m)))

    def __rtruediv__(self, o):
        return Num.of(o) / self

    def exp(self):
        v = CTX.exp(self.v)
        m = CTX.multiply(v, CTX.exp(self.e) - _ONE) if self.e else _ZERO
        return Num(v, CTX.add(m, CTX.multiply(_TWO * U, v + m)))

    def sqrt(self):
        if not self.v > self.e:
            raise ArithmeticError("the bound of a square root's argument reaches zero")
        v = CTX.sqrt(self.v)
        m = v - CTX.sqrt(self.v - self.e) if self.e else _ZERO
        return Num(v, CTX.add(m, CTX.multiply(U, v + m)))


class Dual(object):
    """a Num and its derivatives along the parameters, ``{index in the full vector: Num}`` (absent: exactly zero)"""
    __slots__ = ("v", "g")

    def __init__(self, v, g=None):
        self.v = Num.of(v)
        self.g = g or {}

    @staticmethod
    def of(x):
        return x if isinstance(x, Dual) else Dual(x)

    def __add__(self, o):
        o = Dual.of(o)
        g = dict(self.g)
        for k, d in o.g.items():
            g[k] = g[k] + d if k in g else d
        return Dual(self.v + o.v, g)
    __radd__ = __add__

    def __neg__(self):
        return Dual(-self.v, {k: -d for k, d in self.g.items()})

    def __sub__(self, o):
        return self + (-Dual.of(o))

    def __rsub__(self, o):
        return Dual.of(o) + (-self)

    def __mul__(self, o):
        o = Dual.of(o)
        g = {}
        for k in set(self.g) | set(o.g):        # a.v b.d + b.v a.d
            left = self.v * o.g[k] if k in o.g else None
            right = o.v * self.g[k] if k in self.g else None
            g[k] = left + right if left is not None and right is not None else (left if right is None else right)
        return Dual(self.v * o.v, g)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Dual.of(o)
        q = self.v / o.v
        g = {}
        for k in set(self.g) | set(o.g):        # (a.d - q b.d) / b.v
            num = self.g.get(k)
            if k in o.g:
                num = num - q * o.g[k] if num is not None else -(q * o.g[k])
            g[k] = num / o.v
        return Dual(q, g)

    def __rtruediv__(self, o):
        return Dual.of(o) / self

    def exp(self):
        e = self.v.exp()
        return Dual(e, {k: e * d for k, d in self.g.items()})

    def sqrt(self):
        r = self.v.sqrt()
        return Dual(r, {k: d / (2.0 * r) for k, d in self.g.items()})


_SQRT3 = Num(CTX.sqrt(Decimal(3)), CTX.multiply(U, CTX.sqrt(Decimal(3))))


def _walk(term, p):
    """the six blocks (lists) and the jitter of ``term`` at its full parameters ``p`` (a list of Num or Dual), in the
    order of ``term.coefficients``"""
    zero = type(p[0])(0.0) if p else Num(0.0)
    if isinstance(term, terms.TermSum) and term._formulas_are(terms.TermSum):
        blocks, jitter, at = [[] for _ in range(6)], zero, 0
        for sub in term.terms:
            sb, sj = _walk(sub, p[at:at + sub.full_size])
            for dst, src in zip(blocks, sb):
                dst.extend(src)
            jitter = jitter + sj
            at += sub.full_size
        return blocks, jitter
    if isinstance(term, terms.TermProduct) and term._formulas_are(terms.TermProduct):
        k1, k2 = term.models["k1"], term.models["k2"]
        (ar1, cr1, ac1, bc1, cc1, dc1), _ = _walk(k1, p[:k1.full_size])
        (ar2, cr2, ac2, bc2, cc2, dc2), _ = _walk(k2, p[k1.full_size:])
        reals1, reals2 = list(zip(ar1, cr1)), list(zip(ar2, cr2))
        comps1, comps2 = list(zip(ac1, bc1, cc1, dc1)), list(zip(ac2, bc2, cc2, dc2))
        ar, cr, ac, bc, cc, dc = [], [], [], [], [], []
        for a1, c1 in reals1:
            for a2, c2 in reals2:
                ar.append(a1 * a2), cr.append(c1 + c2)
        for rs, cs in ((reals1, comps2), (reals2, comps1)):
            for a1, c1 in rs:
                for a2, b2, c2, d2 in cs:
                    ac.append(a1 * a2), bc.append(a1 * b2), cc.append(c1 + c2), dc.append(d2)
        for a1, b1, c1, d1 in comps1:
            for a2, b2, c2, d2 in comps2:
                aa, bb, ba, ab = a1 * a2, b1 * b2, b1 * a2, a1 * b2
                ac.append(0.5 * (aa + bb)), bc.append(0.5 * (ba - ab)), cc.append(c1 + c2), dc.append(d1 - d2)
                ac.append(0.5 * (aa - bb)), bc.append(0.5 * (ba + ab)), cc.append(c1 + c2), dc.append(d1 + d2)
        return [ar, cr, ac, bc, cc, dc], zero
    if isinstance(term, terms.JitterTerm) and term._formulas_are(terms.JitterTerm):
        return [[] for _ in range(6)], (2.0 * p[0]).exp()
    if isinstance(term, terms.RealTerm) and term._formulas_are(terms.RealTerm):
        return [[p[0].exp()], [p[1].exp()], [], [], [], []], zero
    if isinstance(term, terms.ComplexTerm) and term._formulas_are(terms.ComplexTerm):
        if term.fit_b:
            return [[], [], [p[0].exp()], [p[1].exp()], [p[2].exp()], [p[3].exp()]], zero
        return [[], [], [p[0].exp()], [zero], [p[1].exp()], [p[2].exp()]], zero
    if isinstance(term, terms.SHOTerm) and term._formulas_are(terms.SHOTerm):
        S0, Q, w0 = p[0].exp(), p[1].exp(), p[2].exp()
        Qn = Q.v if isinstance(Q, Dual) else Q
        Qv = Qn.v
        # the branch is chosen from the 60-digit Q: a double evaluation takes the same one only when 1/2 lies outside
        # Q's own bound -- a draw closer to Q = 1/2 than that has no single reference and is refused here
        if not abs(Qv - Decimal("0.5")) > Qn.e:
            raise ArithmeticError("SHOTerm: Q is within its rounding bound of 1/2; the regime is not decided")
        if Qv < Decimal("0.5"):
            f = (1.0 - 4.0 * (Q * Q)).sqrt()
            pre, rate = 0.5 * (S0 * w0 * Q), 0.5 * (w0 / Q)
            return [[pre * (1.0 + 1.0 / f), pre * (1.0 - 1.0 / f)], [rate * (1.0 - f), rate * (1.0 + f)],
                    [], [], [], []], zero
        f = (4.0 * (Q * Q) - 1.0).sqrt()
        a, rate = S0 * w0 * Q, 0.5 * (w0 / Q)
        return [[], [], [a], [a / f], [rate], [rate * f]], zero
    if isinstance(term, terms.Matern32Term) and term._formulas_are(terms.Matern32Term):
        # the operation sequence of terms.py and clr_kernel_program.h: sqrt(3) exp(-log_rho), exp(2 log_sigma) / w0, then
        # w0 S0, (w0 w0) S0 / eps.  An IEEE product does not depend on the order of its two operands, so writing
        # exp(.) * sqrt(3) here charges the same roundings.
        w0 = (0.0 - p[1]).exp() * _SQRT3
        S0 = (2.0 * p[0]).exp() / w0
        return [[], [], [w0 * S0], [w0 * w0 * S0 / float(term.eps)], [w0], [type(zero)(float(term.eps))]], zero
    raise ValueError("no oracle for %s %r: only the built-in terms with their own formulas" % (type(term).__name__, term))


class Result(object):
    """``value[c]``, ``bound[c]``: the 2 J_real + 4 J_comp coefficients in the order of ``kernel.coefficients`` (blocks
    contiguous) and the bound on a double evaluation, as Decimals; ``jitter``, ``jitter_bound``; ``shape`` =
    ``(J_real, J_comp)``.  With the Jacobian: ``jac[p][c]``, ``jac_bound[p][c]``, ``jitter_jac[p]``,
    ``jitter_jac_bound[p]`` over the unfrozen parameters ``p`` in ``get_parameter_vector()`` order."""


def evaluate(kernel, full=None, jacobian=False):
    """The oracle at the full parameter vector ``full`` (default: the kernel's own), frozen parameters included."""
    if full is None:
        full = kernel.get_parameter_vector(include_frozen=True)
    full = [float(x) for x in full]
    unfrozen = [i for i, m in enumerate(kernel.unfrozen_mask) if m]
    if jacobian:
        frozen = set(range(len(full))) - set(unfrozen)
        p = [Dual(x, None if i in frozen else {i: Num(1.0)}) for i, x in enumerate(full)]
    else:
        p = [Num(x) for x in full]
    blocks, jitter = _walk(kernel, p)
    flat = [x for blk in blocks for x in blk]
    num = (lambda x: x.v) if jacobian else (lambda x: x)
    r = Result()
    r.shape = (len(blocks[0]), len(blocks[2]))
    r.value, r.bound = [num(x).v for x in flat], [num(x).e for x in flat]
    r.jitter, r.jitter_bound = num(jitter).v, num(jitter).e
    if jacobian:
        get = lambda x, i, what: getattr(x.g[i], what) if i in x.g else _ZERO
        r.jac = [[get(x, i, "v") for x in flat] for i in unfrozen]
        r.jac_bound = [[get(x, i, "e") for x in flat] for i in unfrozen]
        r.jitter_jac = [get(jitter, i, "v") for i in unfrozen]
        r.jitter_jac_bound = [get(jitter, i, "e") for i in unfrozen]
    return r


def table(kernel, draws, jacobian=False):
    """:func:`evaluate` for every row of ``draws`` (``(B, kernel.vector_size)``: unfrozen parameters, the layout of
    ``batch.kernel_coefficient_table``); the kernel's own parameters are restored.  A list of Results."""
    saved = kernel.get_parameter_vector()
    out = []
    try:
        for row in np.atleast_2d(np.asarray(draws, dtype=np.float64)).reshape(len(draws), -1):
            kernel.set_parameter_vector(row)
            out.append(evaluate(kernel, jacobian=jacobian))
    finally:
        kernel.set_parameter_vector(saved)
    return out


def deviation(got, value):
    """|got - value| as a Decimal, ``got`` a double taken exactly"""
    return abs(Decimal(float(got)) - value)
