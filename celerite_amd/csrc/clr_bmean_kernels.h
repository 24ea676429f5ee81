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
constexpr int CLR_MEAN_SLAB = 4096;  // samples per workgroup of slab_project_kernel (fixed: see above)

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

// The projection's reduction, shared by every pass of the shape g[b][k] = sum_n phi_k[b][n] f(b N + n): mean_project takes
// f = z (mean_kernels.hip), the noise model's gradient f = 1/2 (alpha^2 - c) (noise_kernels.hip).  One workgroup per
// (problem, slab): thread i takes the samples i, i + 256, ... of the slab in order, K running sums in registers (KT: the
// instantiation's register count, K <= KT); then the shuffle tree of each wave, the four waves in order through LDS.  A
// ragged last slab adds nothing for n >= N.
template <int KT, class Factor>
__global__ void __launch_bounds__(256) slab_project_kernel(const double* __restrict__ phi, long phi_stride, const Factor f,
                                                           int K, int N, long nslab, double* __restrict__ partial) {
  __shared__ double sh[4][KT];
  const long b = blockIdx.x / nslab, slab = blockIdx.x % nslab;
  const long row = b * (long)N;
  const double* pb = phi + b * phi_stride;
  double acc[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) acc[k] = 0.0;
  const long n0 = slab * CLR_MEAN_SLAB + threadIdx.x;
#pragma unroll 4
  for (int i = 0; i < CLR_MEAN_SLAB / 256; ++i) {
    const long n = n0 + i * 256;
    if (n < N) {
      const double zn = f(row + n);
#pragma unroll
      for (int k = 0; k < KT; ++k)
        if (k < K) acc[k] = fma(pb[(long)k * N + n], zn, acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < KT; ++k)
    if (k < K)
      for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_down(acc[k], off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < K) sh[wave][k] = acc[k];
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < K) partial[((long)blockIdx.x) * K + k] = ((sh[0][k] + sh[1][k]) + sh[2][k]) + sh[3][k];
}
// g[b][k] = the slabs' partials [B][slabs][K] added in slab order (mean_kernels.hip: mean_project_finish_kernel)
void launch_slab_project_finish(const double* partial, int K, int B, int N, double* g, hipStream_t s);
// the two launches; false (nothing launched) when B x slabs does not fit a grid
template <class Factor>
bool launch_slab_project(const double* phi, long phi_stride, const Factor& f, int K, int B, int N, double* partial, double* g,
                         hipStream_t s) {
  const long nslab = mean_project_slabs(N), blocks = (long)B * nslab;
  if (blocks > 2147483647L) return false;
  const dim3 grid((unsigned)blocks), block(256);
  if (K <= 4) hipLaunchKernelGGL((slab_project_kernel<4, Factor>), grid, block, 0, s, phi, phi_stride, f, K, N, nslab, partial);
  else if (K <= 8) hipLaunchKernelGGL((slab_project_kernel<8, Factor>), grid, block, 0, s, phi, phi_stride, f, K, N, nslab, partial);
  else hipLaunchKernelGGL((slab_project_kernel<16, Factor>), grid, block, 0, s, phi, phi_stride, f, K, N, nslab, partial);
  launch_slab_project_finish(partial, K, B, N, g, s);
  return true;
}


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

// ---- clr_batch_periodogram: what does not depend on the plan's width (the walks: clr_bperiodogram_kernels.h)
// `rows` rows of `cells` doubles, `stride` apart, all set to v (the constant column, chunk-interleaved)
void launch_fill_rows(double* dst, long stride, int rows, long cells, double v, hipStream_t s);
// base[b] = (q, G_00, d_0) = sum_n (z_r z_r, z_1 z_1, z_1 z_r)[n] / D_n from the chunk-interleaved whitened columns
// zT [B][nz][L][nchunk] (nz = 1: q alone) and the factor's D [B][L][nchunk]: per chunk, then the chunks in order;
// part: B * nchunk * 3 doubles
void launch_periodogram_base(const double* zT, const double* D, int nz, int B, int N, int L, int nchunk, double* part, double* base,
                             hipStream_t s);
// One thread per (problem, frequency of the tile): the chunks' sums [B][nf][nchunk][7] (cc, cs, ss, cr, sr, c1, s1) added in
// chunk order, the bordered matrix [[G, d], [d^T, q]] of the columns (c, s) or (1, c, s), mirrored, and the small solve
// (clr_gram_solve.h, w0 = 0).  Frequency f of the tile goes to entry b * F + f0 + f of the outputs; any may be null.
// power = 1/2 ((d_0 coef_0 + d_1 coef_1) + ...), with the offset less 1/2 d_0^2 / G_00, every operation rounded on its own.
struct PeriodogramOut {
  double *power, *coef, *cov, *gram;
  int* status;
};
void launch_periodogram_reduce(const double* part, const double* base, int B, int nf, int nchunk, int offset, double min_pivot,
                               long F, long f0, const PeriodogramOut& out, hipStream_t s);

}  // namespace clr
