// celerite_amd/csrc/clr_bnoise_kernels.h
//
// A noise model that is linear in its parameters on batched plans (clr_batch_set_noise_basis / _set_noise_weights /
// _grad_noise_weights): diag_eff[b][n] = diag[b][n] + sum_k s[b][k] Psi_k[b][n], K <= CLR_MAX_NOISE_BASIS basis functions
// (a jitter per instrument: Psi_g the indicator of instrument g; an error-bar inflation: Psi_0 = sigma^2, s_0 = f^2 - 1).
// Two bandwidth-bound passes (noise_kernels.hip):
//   noise_form      diag_eff into the plan's diag array from the caller's diagonal kept aside, the basis accumulated in the
//                   fixed order k = 0, 1, ... with every product and sum rounded on its own (no FMA): the bits of NumPy's
//                   diag + (s_0 * Psi_0 + s_1 * Psi_1 + ...).  Grid (slab of samples, problem), 16-byte accesses where
//                   the rows are 16-byte aligned (N even), 8-byte ones otherwise.
//   noise_project   g[b][k] = 1/2 sum_n Psi_k[b][n] (alpha[b][n]^2 - c[b][n]) with alpha = K_b^-1 r_b and c = diag(K_b^-1)
//                   row-major as clr_batch_leave_one_out leaves them: the reduction of mean_project (clr_bmean_kernels.h:
//                   slab_project_kernel) with another per-sample factor -- fixed slabs of CLR_MEAN_SLAB samples, partials
//                   added in order, no atomics: a problem's bits depend on neither B, K, a sharding nor the run.
#pragma once

#include <hip/hip_runtime.h>

#include "clr_bmean_kernels.h"

namespace clr {

// out[b][n] = src[b * src_stride + n] + sum_k s[b][k] psi[b * psi_stride + k * N + n] for b < B (strides 0 = shared; s is
// [B][K], out is [B][N])
void launch_noise_form(const double* src, long src_stride, const double* psi, long psi_stride, const double* s, int K, int B,
                       int N, double* out, hipStream_t stream);
// g[b][k] = 1/2 sum_n psi[b * psi_stride + k * N + n] (alpha[b * N + n]^2 - c[b * N + n]); partial: [B][slabs][K]
// (mean_project_workspace doubles).  False (nothing launched) when B x slabs does not fit a grid.
bool launch_noise_project(const double* psi, long psi_stride, const double* alpha, const double* c, int K, int B, int N,
                          double* partial, double* g, hipStream_t stream);

}  // namespace clr
