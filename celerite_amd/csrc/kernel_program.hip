// celerite_amd/csrc/kernel_program.hip -- a compiled `terms` kernel on the device (clr_batch_evaluate_params,
// clr_batch_grad_params): the evaluator of clr_kernel_program.h, one thread per draw.
//
// Both kernels are latency-sized: B (x P) threads of a few hundred flops each, a few microseconds of work.  So one
// small grid of one-wave workgroups (B = 1024: 16 workgroups on 16 CUs) and no second pass.  The program (validated by
// clr_kernel_create; at most 10 KB) is copied into LDS first, where every lane reads the same word at a time.  A row of
// `params` and a problem's coefficients are B-strided by the API's own layouts ([B][P] in, [B][J] blocks out), so the
// accesses of a wave are strided, not coalesced: 100 KB in all at the headline shape, served by L2.
//
// This unit is compiled without fast-math and with -ffp-contract=off (Makefile): sqrt and / are correctly rounded and no
// product is fused into an add, so the device and the host evaluator differ only where their exp differ (1 ulp each).
#include <hip/hip_runtime.h>

#include "clr_kernel.h"

namespace clr {

namespace {

constexpr int KP_BLOCK = 64;

__device__ inline clr_kp::Program stage_program(const KernelProgramDevice& K, int* s_ops, double* s_consts) {
  for (int i = threadIdx.x; i < K.n_ops; i += blockDim.x) s_ops[i] = K.ops[i];
  for (int i = threadIdx.x; i < K.n_consts; i += blockDim.x) s_consts[i] = K.consts[i];
  __syncthreads();
  return clr_kp::Program{K.n_ops, K.n_consts, K.n_params, K.J_real, K.J_comp, s_ops, s_consts};
}

// address of output column `col` of problem b in the plan's coefficient block
__device__ inline size_t coeff_index(int col, int b, int B, int JR, int JC) {
  if (col < 2 * JR) return (size_t)(col / JR) * B * JR + (size_t)b * JR + col % JR;
  const int cc = col - 2 * JR;
  return (size_t)2 * B * JR + (size_t)(cc / JC) * B * JC + (size_t)b * JC + cc % JC;
}

}  // namespace

__global__ __launch_bounds__(KP_BLOCK) void kernel_program_eval_kernel(KernelProgramDevice K, int B,
                                                                       const double* __restrict__ params,
                                                                       double* __restrict__ coeffs,
                                                                       double* __restrict__ stats) {
  __shared__ int s_ops[CLR_KP_MAX_OPS];
  __shared__ double s_consts[CLR_KP_MAX_CONSTS];
  const clr_kp::Program prog = stage_program(K, s_ops, s_consts);
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int JR = K.J_real, JC = K.J_comp, NC = 2 * JR + 4 * JC;
  const double* row = params + (size_t)b * K.n_params;
  double cmin = INFINITY, cmax = 0.0, dmax = 0.0, jitter = 0.0;
  auto out = [&](int col, double x) {
    coeffs[coeff_index(col, b, B, JR, JC)] = x;
    const int cc = col - 2 * JR;
    if ((col >= JR && col < 2 * JR) || (cc >= 2 * JC && cc < 3 * JC)) {  // a decay rate
      if (!(x >= cmin)) cmin = x;
      cmax = fmax(cmax, fabs(x));
    } else if (cc >= 3 * JC) {
      dmax = fmax(dmax, fabs(x));
    }
  };
  const int err = clr_kp::evaluate<double>(prog, [&](int i) { return row[i]; }, -1, out, [&](double x) { jitter = x; });
  if (err) {
    // a refused draw must not disturb the batch (NaNs in the scan, the batch-wide maxima): a harmless stand-in -- every
    // term exp(-tau), no jitter -- takes its place; the host reports the draw through its flag
    for (int col = 0; col < NC; ++col) {
      const int cc = col - 2 * JR;
      const bool zero = cc >= JC && (cc < 2 * JC || cc >= 3 * JC);  // b_comp, d_comp
      coeffs[coeff_index(col, b, B, JR, JC)] = zero ? 0.0 : 1.0;
    }
    cmin = 1.0; cmax = 1.0; dmax = 0.0; jitter = 0.0;
  }
  coeffs[(size_t)B * NC + b] = jitter;
  stats[(size_t)KP_STAT_CMIN * B + b] = cmin;
  stats[(size_t)KP_STAT_CMAX * B + b] = cmax;
  stats[(size_t)KP_STAT_DMAX * B + b] = dmax;
  stats[(size_t)KP_STAT_JITTER * B + b] = jitter;
  stats[(size_t)KP_STAT_ERROR * B + b] = err ? 1.0 : 0.0;
}

// one thread per (draw, parameter): the program on duals along that parameter, contracted with the draw's
// coefficient gradient as the outputs appear -- no [P][C] Jacobian is ever stored
__global__ __launch_bounds__(KP_BLOCK) void kernel_program_vjp_kernel(KernelProgramDevice K, int B,
                                                                      const double* __restrict__ params,
                                                                      const double* __restrict__ grad,
                                                                      const double* __restrict__ dmean,
                                                                      double* __restrict__ outp) {
  __shared__ int s_ops[CLR_KP_MAX_OPS];
  __shared__ double s_consts[CLR_KP_MAX_CONSTS];
  const clr_kp::Program prog = stage_program(K, s_ops, s_consts);
  const int P = K.n_params;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * P) return;
  const int b = (int)(idx / P), p = (int)(idx % P);
  const int NG = 1 + 2 * K.J_real + 4 * K.J_comp, ncol = P + (dmean ? 1 : 0);
  const double* row = params + (size_t)b * P;
  const double* g = grad + (size_t)b * NG;
  double acc = 0.0, accj = 0.0;
  (void)clr_kp::evaluate<clr_kp::Dual>(
      prog, [&](int i) { return row[i]; }, p, [&](int col, clr_kp::Dual x) { acc += x.d * g[1 + col]; },
      [&](clr_kp::Dual x) { accj = x.d * g[0]; });
  outp[(size_t)b * ncol + p] = accj + acc;
  if (dmean && p == 0) outp[(size_t)b * ncol + P] = dmean[b];
}

void launch_kernel_program_eval(const KernelProgramDevice& K, int B, const double* params, double* coeffs, double* stats,
                                hipStream_t s) {
  hipLaunchKernelGGL(kernel_program_eval_kernel, dim3((B + KP_BLOCK - 1) / KP_BLOCK), dim3(KP_BLOCK), 0, s, K, B, params,
                     coeffs, stats);
}

void launch_kernel_program_vjp(const KernelProgramDevice& K, int B, const double* params, const double* grad,
                               const double* dmean, double* out, hipStream_t s) {
  const long n = (long)B * K.n_params;
  if (n <= 0) return;
  hipLaunchKernelGGL(kernel_program_vjp_kernel, dim3((unsigned)((n + KP_BLOCK - 1) / KP_BLOCK)), dim3(KP_BLOCK), 0, s, K, B,
                     params, grad, dmean, out);
}

}  // namespace clr
