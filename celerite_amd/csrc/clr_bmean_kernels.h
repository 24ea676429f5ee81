// celerite_amd/csrc/clr_bmean_kernels.h
//
// A mean that is linear in its parameters on batched plans (clr_batch_set_mean_basis / _set_mean_weights /
// _grad_mean_weights): mean_b(t_n) = sum_k w[b][k] Phi_k[b][n], K <= CLR_MAX_MEAN_BASIS basis functions.  Two
// bandwidth-bound passes (mean_kernels.hip):
//   linear_residual   r[b][n] = y[b][n] - m[b][n] into the plan's y, m accumulated in the fixed order k = 0, 1, ... with
//                     every product and sum rounded on its own (no FMA): the bits of the same NumPy expression.
//   mean_project      g[b][k] = sum_n Phi_k[b][n] z[b][n] (z = K_b^-1 r_b, row-major, as the batched solve leaves it):
//                     one workgroup per (problem, slab of CLR_MEAN_SLAB samples), K accumulators per thread, a shuffle
//                     tree per wave, the waves through LDS, one partial per (problem, slab, k); a finishing kernel adds
//                     the slabs in order.  No atomics, and a slab is the same whatever B, K or the device: a problem's
//                     bits do not depend on the batch, on a sharding or on the run.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace clr {

constexpr int CLR_MEAN_SLAB = 4096;  // samples per workgroup of mean_project_kernel (fixed: see above)

// slabs per problem, and the doubles of `partial` launch_mean_project needs
inline long mean_project_slabs(int N) { return ((long)N + CLR_MEAN_SLAB - 1) / CLR_MEAN_SLAB; }
inline size_t mean_project_workspace(int B, int N, int K) { return (size_t)B * (size_t)mean_project_slabs(N) * (size_t)K; }

// r[p][n] = y[p * y_stride + n] - sum_k w[p][k] phi[p * phi_stride + k * N + n] for p < nout (strides 0 = shared;
// w is [nout][K], r is [nout][N])
void launch_linear_residual(const double* y, long y_stride, const double* phi, long phi_stride, const double* w, int K,
                            int nout, int N, double* r, hipStream_t s);
// g[b][k] = sum_n phi[b * phi_stride + k * N + n] z[b * N + n]; partial: [B][slabs][K].  False (nothing launched) when
// B x slabs does not fit a grid.
bool launch_mean_project(const double* phi, long phi_stride, const double* z, int K, int B, int N, double* partial,
                         double* g, hipStream_t s);

}  // namespace clr
