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
// and the generalised-least-squares fit of the weights (clr_batch_fit_mean_weights):
//   fit_rhs_*         the K + 1 right-hand sides R = (Phi_0 .. Phi_K-1, r) of a problem, a tile of columns at a time,
//                     straight from the resident basis and residual into the layout the batched solve reads.
//   mean_gram         S[b][j][k] = sum_n R_j[b][n] Z_k[b][n] (Z_k = K_b^-1 R_k): mean_project generalised -- one
//                     workgroup per (problem, slab, column k of the tile), K + 1 accumulators per thread, the same
//                     shuffle tree and LDS step; the finishing kernel adds the slabs in order and stores the symmetric
//                     part.  An entry's bits depend on neither B, the tile, a sharding nor the run.
//   gram_solve        clr_gram_solve.h, one thread per problem.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace clr {

constexpr int CLR_MAX_MEAN_RHS = 17;  // CLR_MAX_MEAN_BASIS basis functions and the residual
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


// ---- clr_batch_fit_mean_weights
// column c of problem b's right-hand sides: Phi_c (c < K) or the residual y (c == K)
struct FitRhs {
  const double* phi;
  long phi_stride;
  const double* y;
  long y_stride;
  int K, N;
};
// columns c0 .. c0 + nr of every problem chunk-interleaved, row b * nr + r of dst ([row][i][chunk], rows `cells` apart;
// cells past the series: zeros) -- the narrow plans' batched solve reads this.  The rows ride on grid.z: the caller keeps
// B * nr <= 65535 (api_batch_consumers.hip: clr_batch_fit_mean_weights sizes its tile so).
void launch_fit_rhs_interleaved(const FitRhs& R, int c0, int nr, int B, int L, int nchunk, double* dst, long cells, hipStream_t s);
// ... row-major, dst[(b * nr + r) * N + n] -- the wide plans' sweeps read this
void launch_fit_rhs_rowmajor(const FitRhs& R, int c0, int nr, int B, double* dst, hipStream_t s);
// doubles of the slab partials [B][slabs][K + 1][K + 1]
inline size_t mean_gram_workspace(int B, int N, int K) {
  return (size_t)B * (size_t)mean_project_slabs(N) * (size_t)(K + 1) * (size_t)(K + 1);
}
// the columns c0 .. c0 + nr of the bordered Gram matrix' slab partials: z is the tile's solutions row-major
// [B][nr][N]; grid (slab, column, problem)
void launch_mean_gram(const FitRhs& R, const double* z, int c0, int nr, int B, double* partial, hipStream_t s);
// gram[b][j][k] = 1/2 (S_jk + S_kj), the slabs added in order
void launch_mean_gram_finish(const double* partial, int K, int B, int N, double* gram, hipStream_t s);
// one thread per problem: clr_gram_solve.h on gram[b] and w0[b]; out[b] = (w_hat[K], cov[K][K], quad, logdet),
// status[b]; work: B * gram_solve_work(K) doubles
void launch_gram_solve(const double* gram, const double* w0, double min_pivot, int K, int B, double* out, int* status,
                       double* work, hipStream_t s);
size_t gram_solve_workspace(int B, int K);  // doubles of `work`
inline size_t gram_solve_out_doubles(int K) { return (size_t)K + (size_t)K * K + 2; }

}  // namespace clr
