// celerite_amd/csrc/clr_kernel.h -- the object behind clr_kernel_* (kernel_program.cpp): a validated program of
// clr_kernel_program.h.  Shared with the plans (api_batch.hip), which copy it to the device.
#pragma once
#include <string>
#include <vector>

#include "clr_kernel_program.h"

struct clr_kernel {
  std::vector<int> ops;
  std::vector<double> consts;
  int n_params = 0, J_real = 0, J_comp = 0;
  clr_kp::Program view() const {
    return clr_kp::Program{(int)ops.size(), (int)consts.size(), n_params, J_real, J_comp, ops.data(), consts.data()};
  }
};

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace clr {

// a program resident in HBM: `ops` and `consts` are device pointers (clr_batch::kp_ops, kp_consts)
struct KernelProgramDevice {
  const int* ops;
  const double* consts;
  int n_ops, n_consts, n_params, J_real, J_comp;
};

// doubles per problem of kernel_program_eval_kernel's statistics block, stored [5][B]: the smallest decay rate, the
// largest |decay rate|, the largest |frequency|, the jitter, 1.0 when the draw was refused (0.0 otherwise)
enum { KP_STAT_CMIN = 0, KP_STAT_CMAX = 1, KP_STAT_DMAX = 2, KP_STAT_JITTER = 3, KP_STAT_ERROR = 4, KP_NSTAT = 5 };

// params[B][n_params] -> coeffs (the layout clr_batch_set_coefficients uploads: a_real c_real a_comp b_comp c_comp
// d_comp, each [B][J_*], | jitter[B]) and stats[KP_NSTAT][B]
void launch_kernel_program_eval(const KernelProgramDevice& K, int B, const double* params, double* coeffs, double* stats,
                                hipStream_t s);
// out[b][p] = jitter_jac[b][p] grad[b][0] + sum_c jac[b][p][c] grad[b][1 + c]; with dmean != NULL out has n_params + 1
// columns and the last one is dmean[b]
void launch_kernel_program_vjp(const KernelProgramDevice& K, int B, const double* params, const double* grad,
                               const double* dmean, double* out, hipStream_t s);

}  // namespace clr
#endif
