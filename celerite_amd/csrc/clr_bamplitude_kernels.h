// celerite_amd/csrc/clr_bamplitude_kernels.h
//
// A per-sample amplitude model on batched plans (clr_batch_set_amplitude_basis / _set_amplitudes / _grad_amplitudes): the
// same latent process seen with another amplitude per band, y_n = s_n f(t_n) + eps_n with
//   s[b][n] = sum_k a[b][k] Gamma_k[b][n],   K <= CLR_MAX_AMPLITUDE_BASIS basis functions (Gamma_k: the indicator of band k).
// With S = diag(s): K_y = S K S + D = S (K + S^-1 D S^-1) S, so every route of the plan evaluates the model once it reads
//   y' = r / s   and   d' = d / (s * s)
// and log det K_y = log det K' + 2 sum_n log|s_n|.  The passes (amplitude_kernels.hip), all without FMA contraction:
//   amplitude_scale    s into its resident [B][N] array, the basis accumulated in the fixed order k = 0, 1, ... with every
//                      product and sum rounded on its own: the bits of NumPy's a_0 * Gamma_0 + a_1 * Gamma_1 + ...; the
//                      same pass sums log|s_n| over fixed slabs of CLR_MEAN_SLAB samples (the slabs' partials added in slab
//                      order, no atomics: a problem's bits depend on neither B, a sharding nor the run) and flags a problem
//                      with a zero or non-finite s_n inside its length, where the stand-in s_n = 1 is written.
//   amplitude_divide   y' and d' from their sources (the caller's arrays kept aside, or -- in place -- the residual of the
//                      linear mean and the variances of the noise model in force).  Elementwise, grid (slab, problem),
//                      16-byte accesses where the rows are 16-byte aligned (N even).
//   three projections  slab_project_kernel (clr_bmean_kernels.h) with the per-sample factors of clr_batch_grad_amplitudes
//                      and of the amplitude-aware clr_batch_grad_mean_weights / _grad_noise_weights.
#pragma once

#include <hip/hip_runtime.h>

#include "clr_bmean_kernels.h"

namespace clr {

// doubles of `partial` launch_amplitude_scale needs: (log sum, flag) per (problem, slab)
inline size_t amplitude_scale_workspace(int B, int N) { return 2 * (size_t)B * (size_t)mean_project_slabs(N); }

// s[b][n] = sum_k a[b][k] gamma[b * gamma_stride + k * N + n] for n < len[b] (len null: N), the stand-in 1 where that is
// zero or not finite, 1 past len[b]; Lf[b] = sum_{n < len[b]} log|s[b][n]|, Lf[B + b] = 1.0 if a stand-in was used else 0.0.
// False (nothing launched) when B x slabs does not fit a grid.
bool launch_amplitude_scale(const double* gamma, long gamma_stride, const double* a, int K, int B, int N, const int* len,
                            double* s, double* partial, double* Lf, hipStream_t stream);
// y[b][n] = ysrc[b * ysrc_stride + n] / s[b][n] (y null: skipped) and d[b][n] = dsrc[b * dsrc_stride + n] / (s[b][n] *
// s[b][n]) (d null: skipped); a source may be its destination (stride N)
void launch_amplitude_divide(const double* ysrc, long ysrc_stride, double* y, const double* dsrc, long dsrc_stride, double* d,
                             const double* s, int B, int N, hipStream_t stream);
// g[b][k] = sum_n gamma_k[b][n] (alpha y' + d' (c - alpha^2) - 1) / s, every array but gamma [B][N]
bool launch_amplitude_project(const double* gamma, long gamma_stride, const double* alpha, const double* c, const double* y,
                              const double* d, const double* s, int K, int B, int N, double* partial, double* g,
                              hipStream_t stream);
// g[b][k] = sum_n phi_k[b][n] z / s: launch_mean_project in data units
bool launch_mean_project_scaled(const double* phi, long phi_stride, const double* z, const double* s, int K, int B, int N,
                                double* partial, double* g, hipStream_t stream);
// g[b][k] = 1/2 sum_n psi_k[b][n] (alpha^2 - c) / s^2: launch_noise_project in data units
bool launch_noise_project_scaled(const double* psi, long psi_stride, const double* alpha, const double* c, const double* s,
                                 int K, int B, int N, double* partial, double* g, hipStream_t stream);

}  // namespace clr
