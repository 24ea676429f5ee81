// celerite_amd/csrc/clr_kernel_program.h -- a `terms` kernel as a flat program: parameter vector -> coefficients.
//
// A tree of built-in terms (celerite_amd/terms.py) is a fixed formula from the kernel's parameter vector to the six
// coefficient blocks and the jitter.  batch.compile_kernel writes that formula down once as a position-independent
// program; the ONE evaluator below runs it for a draw -- on the host behind clr_kernel_coefficients / _jacobian
// (kernel_program.cpp) and on the device inside kernel_program_eval_kernel / _vjp_kernel (kernel_program.hip).  It uses
// + - * / sqrt and exp only, so host and device differ at most where their `exp` differ in the last bit (both units
// are compiled without fast-math and without contraction into FMAs: the Makefile).
//
// Encoding (`ops`: int32 words, `consts`: doubles).  One instruction after the other, each `opcode, operands...`:
//
//   CLR_KP_REAL        dst  pa pc                 a = exp(pa), c = exp(pc)                              RealTerm
//   CLR_KP_COMPLEX     dst  pa pb pc pd           a, b, c, d = exp(.)                                   ComplexTerm
//   CLR_KP_COMPLEX_B0  dst  pa pc pd              b = 0                                                 ComplexTerm without log_b
//   CLR_KP_SHO_OVER    dst0 dst1 pS pQ pw         two real terms; the draw must have Q <  1/2           SHOTerm
//   CLR_KP_SHO_UNDER   dst  pS pQ pw              one complex term; the draw must have Q >= 1/2         SHOTerm
//   CLR_KP_MATERN32    dst  ps pr keps            d = eps = consts[keps]                                Matern32Term
//   CLR_KP_JITTER      ps                         jitter += exp(2 ps)                                   JitterTerm
//   CLR_KP_MUL_RR      dst  r1 r2                 (a1 a2, c1 + c2)                                      TermProduct
//   CLR_KP_MUL_RC      dst  r1 c2                 (a1 a2, a1 b2, c1 + c2, d2)
//   CLR_KP_MUL_CC      dstm dstp c1 c2            ((a1 a2 -+ b1 b2) / 2, (b1 a2 +- a1 b2) / 2, c1 + c2, d1 -+ d2)
//
// A parameter operand `p*` is an index into the draw's (unfrozen) parameter vector when >= 0, and the constant
// consts[-(p + 1)] -- a frozen parameter's value at compile time -- when negative.  A destination `dst*` is the index
// of a term in its output block (real terms: columns a_real[dst], c_real[dst]; complex terms: a_comp[dst], b_comp[dst],
// c_comp[dst], d_comp[dst]) when >= 0, and the temporary term -(dst + 1) when negative.  The factors `r*`, `c*` of a
// product are temporaries, written by an earlier instruction, given as their index >= 0.  Output columns are numbered
// like the batched gradient's columns 1..: a_real | c_real | a_comp | b_comp | c_comp | d_comp, each block contiguous.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define CLR_KP_HD __host__ __device__
#else
#define CLR_KP_HD
#endif

enum {
  CLR_KP_REAL = 1, CLR_KP_COMPLEX = 2, CLR_KP_COMPLEX_B0 = 3, CLR_KP_SHO_OVER = 4, CLR_KP_SHO_UNDER = 5,
  CLR_KP_MATERN32 = 6, CLR_KP_JITTER = 7, CLR_KP_MUL_RR = 8, CLR_KP_MUL_RC = 9, CLR_KP_MUL_CC = 10
};
#define CLR_KP_MAX_TEMPS 16      /* temporary real terms, and as many temporary complex terms, of one program */
#define CLR_KP_MAX_OPS 2048      /* int32 words */
#define CLR_KP_MAX_CONSTS 256
#define CLR_KP_MAX_PARAMS 256

namespace clr_kp {

struct Program {
  int n_ops, n_consts, n_params, J_real, J_comp;
  const int* ops;
  const double* consts;
};

// instruction length in words by opcode (0: not an opcode)
CLR_KP_HD inline int op_length(int op) {
  switch (op) {
    case CLR_KP_REAL: return 4;
    case CLR_KP_COMPLEX: return 6;
    case CLR_KP_COMPLEX_B0: return 5;
    case CLR_KP_SHO_OVER: return 6;
    case CLR_KP_SHO_UNDER: return 5;
    case CLR_KP_MATERN32: return 5;
    case CLR_KP_JITTER: return 2;
    case CLR_KP_MUL_RR: return 4;
    case CLR_KP_MUL_RC: return 4;
    case CLR_KP_MUL_CC: return 5;
  }
  return 0;
}

CLR_KP_HD inline bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// value + one directional derivative: the arithmetic of terms._Dual for one direction of the parameter vector
struct Dual {
  double v, d;
};
CLR_KP_HD inline Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
CLR_KP_HD inline Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
CLR_KP_HD inline Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.v * b.d + b.v * a.d}; }
CLR_KP_HD inline Dual operator/(Dual a, Dual b) {
  const double q = a.v / b.v;
  return {q, (a.d - q * b.d) / b.v};
}
CLR_KP_HD inline Dual operator*(double s, Dual a) { return {s * a.v, s * a.d}; }
CLR_KP_HD inline Dual operator/(Dual a, double s) { return {a.v / s, a.d / s}; }
CLR_KP_HD inline Dual operator+(double s, Dual a) { return {s + a.v, a.d}; }
CLR_KP_HD inline Dual operator-(double s, Dual a) { return {s - a.v, 0.0 - a.d}; }
CLR_KP_HD inline Dual operator-(Dual a, double s) { return {a.v - s, a.d}; }
CLR_KP_HD inline Dual operator/(double s, Dual a) {
  const double q = s / a.v;
  return {q, (0.0 - q * a.d) / a.v};
}
CLR_KP_HD inline Dual kp_exp(Dual a) {
  const double e = exp(a.v);
  return {e, e * a.d};
}
CLR_KP_HD inline Dual kp_sqrt(Dual a) {
  const double r = sqrt(a.v);
  return {r, a.d / (2.0 * r)};
}
CLR_KP_HD inline double kp_exp(double a) { return exp(a); }
CLR_KP_HD inline double kp_sqrt(double a) { return sqrt(a); }
CLR_KP_HD inline double value_of(double a) { return a; }
CLR_KP_HD inline double value_of(Dual a) { return a.v; }
CLR_KP_HD inline void lift(double x, bool, double& out) { out = x; }
CLR_KP_HD inline void lift(double x, bool seed, Dual& out) { out.v = x; out.d = seed ? 1.0 : 0.0; }

// Runs the program on one draw.  T: double (values) or Dual (values + the derivative along parameter `dir`).
// `params(i)`: parameter i of the draw.  `out(column, x)`: receives every output column exactly once, `jit(x)` the
// jitter.  Returns 0, or 1 when the draw is not valid for this program: a non-finite parameter, an SHO term on the
// other side of Q = 1/2 than the program was compiled for, a non-finite coefficient.  The outputs of such a draw are
// still all delivered (whatever the formulas gave): the caller replaces them.
template <class T, class Params, class Out, class Jit>
CLR_KP_HD inline int evaluate(const Program& K, const Params& params, int dir, Out&& out, Jit&& jit) {
  T tr[CLR_KP_MAX_TEMPS][2], tc[CLR_KP_MAX_TEMPS][4];
  int err = 0;
  const int JR = K.J_real, JC = K.J_comp;
  for (int i = 0; i < K.n_params; ++i) err |= !finite(params(i));
  auto arg = [&](int ref) {
    T x;
    if (ref >= 0) lift(params(ref), ref == dir, x);
    else lift(K.consts[-(ref + 1)], false, x);
    return x;
  };
  auto put_real = [&](int dst, T a, T c) {
    err |= (!finite(value_of(a)) || !finite(value_of(c))) ? 1 : 0;
    if (dst >= 0) { out(dst, a); out(JR + dst, c); }
    else { tr[-(dst + 1)][0] = a; tr[-(dst + 1)][1] = c; }
  };
  auto put_comp = [&](int dst, T a, T b, T c, T d) {
    err |= (!finite(value_of(a)) || !finite(value_of(b)) || !finite(value_of(c)) || !finite(value_of(d))) ? 1 : 0;
    if (dst >= 0) { out(2 * JR + dst, a); out(2 * JR + JC + dst, b); out(2 * JR + 2 * JC + dst, c); out(2 * JR + 3 * JC + dst, d); }
    else { T* t = tc[-(dst + 1)]; t[0] = a; t[1] = b; t[2] = c; t[3] = d; }
  };
  T jitter;
  lift(0.0, false, jitter);
  T zero;
  lift(0.0, false, zero);
  for (int pc = 0; pc < K.n_ops;) {
    const int* w = K.ops + pc;
    const int op = w[0];
    switch (op) {
      case CLR_KP_REAL:
        put_real(w[1], kp_exp(arg(w[2])), kp_exp(arg(w[3])));
        break;
      case CLR_KP_COMPLEX:
        put_comp(w[1], kp_exp(arg(w[2])), kp_exp(arg(w[3])), kp_exp(arg(w[4])), kp_exp(arg(w[5])));
        break;
      case CLR_KP_COMPLEX_B0:
        put_comp(w[1], kp_exp(arg(w[2])), zero, kp_exp(arg(w[3])), kp_exp(arg(w[4])));
        break;
      case CLR_KP_SHO_OVER: {  // terms.py, SHOTerm.get_real_coefficients
        const T S0 = kp_exp(arg(w[3])), Q = kp_exp(arg(w[4])), w0 = kp_exp(arg(w[5]));
        err |= !(value_of(Q) < 0.5);
        const T f = kp_sqrt(1.0 - 4.0 * (Q * Q));
        const T pre = 0.5 * (S0 * w0 * Q), rate = 0.5 * (w0 / Q);
        put_real(w[1], pre * (1.0 + 1.0 / f), rate * (1.0 - f));
        put_real(w[2], pre * (1.0 - 1.0 / f), rate * (1.0 + f));
        break;
      }
      case CLR_KP_SHO_UNDER: {  // SHOTerm.get_complex_coefficients
        const T S0 = kp_exp(arg(w[2])), Q = kp_exp(arg(w[3])), w0 = kp_exp(arg(w[4]));
        err |= !(value_of(Q) >= 0.5);
        const T f = kp_sqrt(4.0 * (Q * Q) - 1.0);
        const T a = S0 * w0 * Q, rate = 0.5 * (w0 / Q);
        put_comp(w[1], a, a / f, rate, rate * f);
        break;
      }
      case CLR_KP_MATERN32: {  // Matern32Term.get_complex_coefficients
        const double eps = K.consts[w[4]];
        const T w0 = 1.7320508075688772 * kp_exp(0.0 - arg(w[3]));
        const T S0 = kp_exp(2.0 * arg(w[2])) / w0;
        T d;
        lift(eps, false, d);
        put_comp(w[1], w0 * S0, w0 * w0 * S0 / eps, w0, d);
        break;
      }
      case CLR_KP_JITTER: {
        const T j = kp_exp(2.0 * arg(w[1]));
        err |= !finite(value_of(j));
        jitter = jitter + j;
        break;
      }
      case CLR_KP_MUL_RR: {
        const T* x = tr[w[2]];
        const T* y = tr[w[3]];
        put_real(w[1], x[0] * y[0], x[1] + y[1]);
        break;
      }
      case CLR_KP_MUL_RC: {
        const T* x = tr[w[2]];
        const T* y = tc[w[3]];
        put_comp(w[1], x[0] * y[0], x[0] * y[1], x[1] + y[2], y[3]);
        break;
      }
      case CLR_KP_MUL_CC: {
        const T* x = tc[w[3]];
        const T* y = tc[w[4]];
        const T aa = x[0] * y[0], bb = x[1] * y[1], ba = x[1] * y[0], ab = x[0] * y[1];
        put_comp(w[1], 0.5 * (aa + bb), 0.5 * (ba - ab), x[2] + y[2], x[3] - y[3]);
        put_comp(w[2], 0.5 * (aa - bb), 0.5 * (ba + ab), x[2] + y[2], x[3] + y[3]);
        break;
      }
    }
    pc += op_length(op);
  }
  jit(jitter);
  return err;
}

}  // namespace clr_kp
