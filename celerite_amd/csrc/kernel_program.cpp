// celerite_amd/csrc/kernel_program.cpp -- clr_kernel_*: a compiled `terms` kernel on the host (no device work).
//
// clr_kernel_create checks a program of clr_kernel_program.h once, so that the evaluator -- here and in the device
// kernels of kernel_program.hip -- never reads outside the program, the parameter row, the constants or its
// temporaries; clr_kernel_coefficients / _jacobian run it per draw.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/celerite_hip.h"
#include "clr_kernel.h"

extern thread_local std::string clr_api_last_error;

namespace {

int refuse(const char* why) {
  clr_api_last_error = std::string("clr_kernel_create: ") + why;
  return CLR_INVALID_ARGUMENT;
}

// every operand in range, temporaries written before they are read, every output term written exactly once
int validate(int n_ops, const int* ops, int n_consts, int n_params, int J_real, int J_comp) {
  if (n_ops < 0 || n_consts < 0 || n_params < 0 || J_real < 0 || J_comp < 0) return refuse("negative size");
  if (n_ops > CLR_KP_MAX_OPS || n_consts > CLR_KP_MAX_CONSTS || n_params > CLR_KP_MAX_PARAMS)
    return refuse("program too long");
  if (2 * (long)J_real + 4 * (long)J_comp > 4 * CLR_MAX_WIDTH) return refuse("too many terms");
  std::vector<int> out_r(J_real, 0), out_c(J_comp, 0);
  bool tmp_r[CLR_KP_MAX_TEMPS] = {false}, tmp_c[CLR_KP_MAX_TEMPS] = {false};
  bool ok = true;
  auto param = [&](int ref) { ok = ok && (ref >= 0 ? ref < n_params : -(long)ref - 1 < n_consts); };
  auto dst = [&](int d, std::vector<int>& outs, bool* tmps) {
    if (d >= 0) {
      if (d < (int)outs.size()) ++outs[d];
      else ok = false;
    } else {
      const long k = -(long)d - 1;
      if (k < CLR_KP_MAX_TEMPS && !tmps[k]) tmps[k] = true;
      else ok = false;
    }
  };
  auto src = [&](int k, const bool* tmps) { ok = ok && k >= 0 && k < CLR_KP_MAX_TEMPS && tmps[k]; };
  for (int pc = 0; pc < n_ops;) {
    const int* w = ops + pc;
    const int len = clr_kp::op_length(w[0]);
    if (len == 0 || pc + len > n_ops) return refuse("unknown opcode or truncated instruction");
    switch (w[0]) {
      case CLR_KP_REAL: dst(w[1], out_r, tmp_r); param(w[2]); param(w[3]); break;
      case CLR_KP_COMPLEX: dst(w[1], out_c, tmp_c); param(w[2]); param(w[3]); param(w[4]); param(w[5]); break;
      case CLR_KP_COMPLEX_B0: dst(w[1], out_c, tmp_c); param(w[2]); param(w[3]); param(w[4]); break;
      case CLR_KP_SHO_OVER: dst(w[1], out_r, tmp_r); dst(w[2], out_r, tmp_r); param(w[3]); param(w[4]); param(w[5]); break;
      case CLR_KP_SHO_UNDER: dst(w[1], out_c, tmp_c); param(w[2]); param(w[3]); param(w[4]); break;
      case CLR_KP_MATERN32: dst(w[1], out_c, tmp_c); param(w[2]); param(w[3]); ok = ok && w[4] >= 0 && w[4] < n_consts; break;
      case CLR_KP_JITTER: param(w[1]); break;
      case CLR_KP_MUL_RR: src(w[2], tmp_r); src(w[3], tmp_r); dst(w[1], out_r, tmp_r); break;
      case CLR_KP_MUL_RC: src(w[2], tmp_r); src(w[3], tmp_c); dst(w[1], out_c, tmp_c); break;
      case CLR_KP_MUL_CC: src(w[3], tmp_c); src(w[4], tmp_c); dst(w[1], out_c, tmp_c); dst(w[2], out_c, tmp_c); break;
    }
    if (!ok) return refuse("operand out of range, temporary read before it is written, or written twice");
    pc += len;
  }
  for (int n : out_r) ok = ok && n == 1;
  for (int n : out_c) ok = ok && n == 1;
  if (!ok) return refuse("an output term is not written exactly once");
  return CLR_OK;
}

}  // namespace

extern "C" {

int clr_kernel_create(int n_ops, const int* ops, int n_consts, const double* consts, int n_params, int J_real,
                      int J_comp, clr_kernel** out) {
  if (!out || (n_ops > 0 && !ops) || (n_consts > 0 && !consts)) return refuse("null argument");
  *out = nullptr;
  const int st = validate(n_ops, ops, n_consts, n_params, J_real, J_comp);
  if (st != CLR_OK) return st;
  clr_kernel* k = new clr_kernel();
  k->ops.assign(ops, ops + n_ops);
  k->consts.assign(consts, consts + n_consts);
  k->n_params = n_params;
  k->J_real = J_real;
  k->J_comp = J_comp;
  *out = k;
  return CLR_OK;
}

void clr_kernel_destroy(clr_kernel* k) { delete k; }

int clr_kernel_get_shape(const clr_kernel* k, int* n_params, int* J_real, int* J_comp) {
  if (!k) return CLR_INVALID_ARGUMENT;
  if (n_params) *n_params = k->n_params;
  if (J_real) *J_real = k->J_real;
  if (J_comp) *J_comp = k->J_comp;
  return CLR_OK;
}

int clr_kernel_coefficients(const clr_kernel* k, int B, const double* params, double* a_real, double* c_real,
                            double* a_comp, double* b_comp, double* c_comp, double* d_comp, double* jitter,
                            int* status) {
  if (!k || B < 0 || (B > 0 && k->n_params > 0 && !params)) return CLR_INVALID_ARGUMENT;
  const clr_kp::Program K = k->view();
  const int JR = k->J_real, JC = k->J_comp, P = k->n_params;
  double* block[6] = {a_real, c_real, a_comp, b_comp, c_comp, d_comp};
  for (int i = 0; i < 6; ++i)
    if (!block[i] && (i < 2 ? JR : JC) > 0 && B > 0) return CLR_INVALID_ARGUMENT;
  const double nan = std::nan("");
  for (int b = 0; b < B; ++b) {
    const double* row = params + (size_t)b * P;
    auto out = [&](int col, double x) {
      if (col < 2 * JR) block[col / (JR ? JR : 1)][(size_t)b * JR + col % (JR ? JR : 1)] = x;
      else block[2 + (col - 2 * JR) / JC][(size_t)b * JC + (col - 2 * JR) % JC] = x;
    };
    double jit = 0.0;
    const int err = clr_kp::evaluate<double>(K, [&](int i) { return row[i]; }, -1, out, [&](double x) { jit = x; });
    if (err) {
      for (int col = 0; col < 2 * JR + 4 * JC; ++col) out(col, nan);
      jit = nan;
    }
    if (jitter) jitter[b] = jit;
    if (status) status[b] = err ? CLR_INVALID_ARGUMENT : CLR_OK;
  }
  return CLR_OK;
}

int clr_kernel_jacobian(const clr_kernel* k, int B, const double* params, double* jac, double* jitter_jac,
                        int* status) {
  if (!k || B < 0 || (B > 0 && k->n_params > 0 && !params)) return CLR_INVALID_ARGUMENT;
  const clr_kp::Program K = k->view();
  const int P = k->n_params, NC = 2 * k->J_real + 4 * k->J_comp;
  const double nan = std::nan("");
  for (int b = 0; b < B; ++b) {
    const double* row = params + (size_t)b * P;
    int err = 0;
    for (int p = 0; p < P; ++p) {
      double* jrow = jac ? jac + ((size_t)b * P + p) * NC : nullptr;
      double dj = 0.0;
      err |= clr_kp::evaluate<clr_kp::Dual>(
          K, [&](int i) { return row[i]; }, p, [&](int col, clr_kp::Dual x) { if (jrow) jrow[col] = x.d; },
          [&](clr_kp::Dual x) { dj = x.d; });
      if (jitter_jac) jitter_jac[(size_t)b * P + p] = dj;
    }
    if (err) {
      if (jac) for (size_t i = 0; i < (size_t)P * NC; ++i) jac[(size_t)b * P * NC + i] = nan;
      if (jitter_jac) for (int p = 0; p < P; ++p) jitter_jac[(size_t)b * P + p] = nan;
    }
    if (status) status[b] = err ? CLR_INVALID_ARGUMENT : CLR_OK;
  }
  return CLR_OK;
}

}  // extern "C"
