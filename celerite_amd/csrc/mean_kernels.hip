// celerite_amd/csrc/mean_kernels.hip -- the two passes of a linear mean model on batched plans (clr_bmean_kernels.h).
#include "clr_bmean_kernels.h"
#include "clr_gram_solve.h"

#include <algorithm>

namespace clr {
namespace {

// The residual of clr_batch_set_mean_weights.  Contraction is off for this function (and for the unit: Makefile): hipcc
// would otherwise fuse w_k Phi_k into the running sum, and the result would no longer be the bits of
//   m = w[:, 0, None] * Phi[0];  m = m + w[:, k, None] * Phi[k]  (k = 1 .. K - 1);  r = y - m
// (the intrinsics __dmul_rn / __dadd_rn are plain operators to this compiler and would be fused like them).
__global__ void __launch_bounds__(256) linear_residual_kernel(const double* __restrict__ y, long y_stride,
                                                              const double* __restrict__ phi, long phi_stride,
                                                              const double* __restrict__ w, int K, int nout, int N,
                                                              double* __restrict__ r) {
#pragma clang fp contract(off)
  for (long p = blockIdx.y; p < nout; p += gridDim.y) {
    const double* wp = w + p * K;
    const double* src = y + p * y_stride;
    const double* basis = phi + p * phi_stride;
    double* dst = r + p * (long)N;
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long)gridDim.x * blockDim.x) {
      double m = wp[0] * basis[n];
      for (int k = 1; k < K; ++k) {
        const double term = wp[k] * basis[(long)k * N + n];
        m = m + term;
      }
      dst[n] = src[n] - m;
    }
  }
}

// the per-sample factor of clr_batch_grad_mean_weights' projection (slab_project_kernel, clr_bmean_kernels.h): z = K^-1 r
struct SolveFactor {
  const double* z;
  __device__ double operator()(long i) const { return z[i]; }
};

// g[b][k] = the slabs' partials added in slab order: one thread per (problem, k)
__global__ void __launch_bounds__(256) mean_project_finish_kernel(const double* __restrict__ partial, long nslab, int K,
                                                                  long BK, double* __restrict__ g) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= BK) return;
  const long b = i / K, k = i % K;
  const double* p = partial + b * nslab * K + k;
  double s = 0.0;
  for (long c = 0; c < nslab; ++c) s += p[c * K];
  g[i] = s;
}

// ---- the generalised-least-squares fit of the weights (clr_batch_fit_mean_weights)

__device__ inline const double* fit_rhs_column(const FitRhs& R, long b, int c) {
  return c < R.K ? R.phi + b * R.phi_stride + (long)c * R.N : R.y + b * R.y_stride;
}

// relayout_kernel (api_kernels.hip) reading row z = b * nr + r from column c0 + r of problem b's right-hand sides
__global__ void __launch_bounds__(256) fit_rhs_interleaved_kernel(FitRhs R, int c0, int nr, int L, int nchunk,
                                                                  double* __restrict__ dst, long cells) {
  __shared__ double tile[32][33];
  const int row = blockIdx.z, i0 = blockIdx.x * 32, ch0 = blockIdx.y * 32;
  const double* in = fit_rhs_column(R, row / nr, c0 + row % nr);
  double* out = dst + (long)row * cells;
  for (int r = threadIdx.y; r < 32; r += 8) {
    const int c = ch0 + r, i = i0 + threadIdx.x;
    const long n = (long)c * L + i;
    tile[r][threadIdx.x] = (c < nchunk && i < L && n < R.N) ? in[n] : 0.0;
  }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += 8) {
    const int i = i0 + r, c = ch0 + threadIdx.x;
    if (i < L && c < nchunk) out[(long)i * nchunk + c] = tile[threadIdx.x][r];
  }
}

__global__ void __launch_bounds__(256) fit_rhs_rowmajor_kernel(FitRhs R, int c0, int nr, double* __restrict__ dst) {
  const long b = blockIdx.z;
  const int r = blockIdx.y;
  const double* in = fit_rhs_column(R, b, c0 + r);
  double* out = dst + (b * nr + r) * (long)R.N;
  for (long n = (long)blockIdx.x * 256 + threadIdx.x; n < R.N; n += (long)gridDim.x * 256) out[n] = in[n];
}

// slab_project_kernel (clr_bmean_kernels.h) with the K + 1 right-hand sides in the place of the basis: the workgroup (slab, column k, problem
// b) sums R_j Z_k over its slab for j = 0 .. K (KT: the instantiation's register count, K + 1 <= KT).  partial:
// [b][slab][k][j].
template <int KT>
__global__ void __launch_bounds__(256) mean_gram_kernel(FitRhs R, const double* __restrict__ z, int c0, int nr, long nslab,
                                                        double* __restrict__ partial) {
  __shared__ double sh[4][KT];
  const long b = blockIdx.z, slab = blockIdx.x;
  const int K1 = R.K + 1, k = c0 + blockIdx.y, N = R.N;
  const double* zb = z + (b * nr + blockIdx.y) * (long)N;
  const double* pb = R.phi + b * R.phi_stride;
  const double* yb = R.y + b * R.y_stride;
  double acc[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j) acc[j] = 0.0;
  const long n0 = slab * CLR_MEAN_SLAB + threadIdx.x;
#pragma unroll 4
  for (int i = 0; i < CLR_MEAN_SLAB / 256; ++i) {
    const long n = n0 + i * 256;
    if (n < N) {
      const double zn = zb[n];
#pragma unroll
      for (int j = 0; j < KT; ++j)
        if (j < K1) acc[j] = fma(j < R.K ? pb[(long)j * N + n] : yb[n], zn, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < KT; ++j)
    if (j < K1)
      for (int off = 32; off > 0; off >>= 1) acc[j] += __shfl_down(acc[j], off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < KT; ++j)
      if (j < K1) sh[wave][j] = acc[j];
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j < K1) partial[((b * nslab + slab) * K1 + k) * K1 + j] = ((sh[0][j] + sh[1][j]) + sh[2][j]) + sh[3][j];
}

// one thread per (problem, j, k): S_jk and S_kj, each the slabs' partials in slab order, then their mean
__global__ void __launch_bounds__(256) mean_gram_finish_kernel(const double* __restrict__ partial, long nslab, int K1, long total,
                                                               double* __restrict__ gram) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long KK = (long)K1 * K1, b = i / KK, j = (i % KK) / K1, k = i % K1;
  const double* p = partial + b * nslab * KK;
  double sjk = 0.0, skj = 0.0;
  for (long c = 0; c < nslab; ++c) {
    sjk += p[c * KK + k * K1 + j];
    skj += p[c * KK + j * K1 + k];
  }
  gram[i] = 0.5 * (sjk + skj);
}

__global__ void __launch_bounds__(64) gram_solve_kernel(const double* __restrict__ gram, const double* __restrict__ w0, double min_pivot,
                                                        int K, int B, double* __restrict__ out, int* __restrict__ status,
                                                        double* __restrict__ work) {
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const long K1 = K + 1, no = (long)K + (long)K * K + 2;
  double* o = out + b * no;
  status[b] = gram_solve(K, gram + b * K1 * K1, w0 + b * K, min_pivot, o, o + K, o + K + (long)K * K, o + K + (long)K * K + 1,
                         work + b * gram_solve_work(K));
}

__global__ void __launch_bounds__(256) fill_rows_kernel(double* __restrict__ dst, long stride, long cells, double v) {
  double* row = dst + (long)blockIdx.y * stride;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < cells; i += (long)gridDim.x * 256) row[i] = v;
}

// one thread per (problem, chunk): the chunk's share of q, G_00, d_0
__global__ void __launch_bounds__(64) periodogram_base_kernel(const double* __restrict__ zT, const double* __restrict__ D, int nz,
                                                              int N, int L, int nchunk, double* __restrict__ part) {
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x;
  if (c >= nchunk) return;
  const long cells = (long)L * nchunk;
  const double* zr = zT + (long)b * nz * cells + c;
  const double* z1 = zr + cells;
  const double* d = D + (long)b * cells + c;
  const int last = (N - c * L < L) ? N - c * L : L;
  double q = 0.0, g00 = 0.0, d0 = 0.0;
  for (int i = 0; i < last; ++i) {
    const double dn = d[(long)i * nchunk], r = zr[(long)i * nchunk];
    q = q + (r * r) / dn;
    if (nz > 1) {
      const double o = z1[(long)i * nchunk];
      g00 = g00 + (o * o) / dn;
      d0 = d0 + (o * r) / dn;
    }
  }
  double* p = part + ((long)b * nchunk + c) * 3;
  p[0] = q; p[1] = g00; p[2] = d0;
}

__global__ void __launch_bounds__(64) periodogram_base_finish_kernel(const double* __restrict__ part, int B, int nchunk,
                                                                     double* __restrict__ base) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double s[3] = {0.0, 0.0, 0.0};
  for (int c = 0; c < nchunk; ++c)
    for (int i = 0; i < 3; ++i) s[i] = s[i] + part[((long)b * nchunk + c) * 3 + i];
  for (int i = 0; i < 3; ++i) base[(long)b * 3 + i] = s[i];
}

template <int K>  // 2: the columns (c, s); 3: (1, c, s)
__global__ void __launch_bounds__(64) periodogram_reduce_kernel(const double* __restrict__ part, const double* __restrict__ base, int B,
                                                                int nf, int nchunk, double min_pivot, long F, long f0,
                                                                const PeriodogramOut out) {
  constexpr bool offset = K == 3;
  const long idx = (long)blockIdx.x * 64 + threadIdx.x;
  if (idx >= (long)B * nf) return;
  const long b = idx / nf, f = idx % nf, o = b * F + f0 + f;
  double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double* p = part + idx * nchunk * 7;
  for (int c = 0; c < nchunk; ++c)
    for (int i = 0; i < 7; ++i) s[i] = s[i] + p[(long)c * 7 + i];
  const double q = base[b * 3], g00 = base[b * 3 + 1], d0 = base[b * 3 + 2];
  constexpr int K1 = K + 1;
  double S[K1 * K1];
  // the upper triangle, mirrored below: columns (c, s) or (1, c, s), then the border (d, q)
  constexpr int ic = offset ? 1 : 0, is = ic + 1;
  if (offset) {
    S[0] = g00; S[0 * K1 + ic] = s[5]; S[0 * K1 + is] = s[6]; S[0 * K1 + K] = d0;
  }
  S[ic * K1 + ic] = s[0]; S[ic * K1 + is] = s[1]; S[ic * K1 + K] = s[3];
  S[is * K1 + is] = s[2]; S[is * K1 + K] = s[4];
  S[K * K1 + K] = q;
  for (int i = 0; i < K1; ++i)
    for (int j = 0; j < i; ++j) S[i * K1 + j] = S[j * K1 + i];
  if (out.gram)
    for (int i = 0; i < K1 * K1; ++i) out.gram[o * K1 * K1 + i] = S[i];
  const double zero[3] = {0.0, 0.0, 0.0};
  double w[3], cv[9], quad, ld, work[15];
  const int st = gram_solve(K, S, zero, min_pivot, w, cv, &quad, &ld, work);
  const double nan = __builtin_nan("");
  double pw = nan;
  if (st == 0) {
    pw = S[0 * K1 + K] * w[0] + S[1 * K1 + K] * w[1];
    if (offset) pw = (pw + S[2 * K1 + K] * w[2]) - (d0 * d0) / g00;
    pw = 0.5 * pw;
  } else {
    for (int i = 0; i < K; ++i) w[i] = nan;  // (gram_solve leaves w0 there)
  }
  if (out.power) out.power[o] = pw;
  if (out.coef)
    for (int i = 0; i < K; ++i) out.coef[o * K + i] = w[i];
  if (out.cov)
    for (int i = 0; i < K * K; ++i) out.cov[o * K * K + i] = cv[i];
  if (out.status) out.status[o] = st;
}

}  // namespace

void launch_fill_rows(double* dst, long stride, int rows, long cells, double v, hipStream_t s) {
  const dim3 grid((unsigned)std::min<long>((cells + 255) / 256, 1024), (unsigned)rows);
  hipLaunchKernelGGL(fill_rows_kernel, grid, dim3(256), 0, s, dst, stride, cells, v);
}

void launch_periodogram_base(const double* zT, const double* D, int nz, int B, int N, int L, int nchunk, double* part, double* base,
                             hipStream_t s) {
  hipLaunchKernelGGL(periodogram_base_kernel, dim3((unsigned)((nchunk + 63) / 64), (unsigned)B), dim3(64), 0, s, zT, D, nz, N, L, nchunk,
                     part);
  hipLaunchKernelGGL(periodogram_base_finish_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, part, B, nchunk, base);
}

void launch_periodogram_reduce(const double* part, const double* base, int B, int nf, int nchunk, int offset, double min_pivot,
                               long F, long f0, const PeriodogramOut& out, hipStream_t s) {
  const long n = (long)B * nf;
  const dim3 grid((unsigned)((n + 63) / 64));
  if (offset) hipLaunchKernelGGL(periodogram_reduce_kernel<3>, grid, dim3(64), 0, s, part, base, B, nf, nchunk, min_pivot, F, f0, out);
  else hipLaunchKernelGGL(periodogram_reduce_kernel<2>, grid, dim3(64), 0, s, part, base, B, nf, nchunk, min_pivot, F, f0, out);
}

void launch_fit_rhs_interleaved(const FitRhs& R, int c0, int nr, int B, int L, int nchunk, double* dst, long cells, hipStream_t s) {
  const dim3 grid((L + 31) / 32, (nchunk + 31) / 32, (unsigned)(B * nr));
  hipLaunchKernelGGL(fit_rhs_interleaved_kernel, grid, dim3(32, 8), 0, s, R, c0, nr, L, nchunk, dst, cells);
}

void launch_fit_rhs_rowmajor(const FitRhs& R, int c0, int nr, int B, double* dst, hipStream_t s) {
  const dim3 grid((unsigned)std::min((R.N + 255) / 256, 256), (unsigned)nr, (unsigned)B);
  hipLaunchKernelGGL(fit_rhs_rowmajor_kernel, grid, dim3(256), 0, s, R, c0, nr, dst);
}

void launch_mean_gram(const FitRhs& R, const double* z, int c0, int nr, int B, double* partial, hipStream_t s) {
  const long nslab = mean_project_slabs(R.N);
  const dim3 grid((unsigned)nslab, (unsigned)nr, (unsigned)B), block(256);
  const int K1 = R.K + 1;
  if (K1 <= 4) hipLaunchKernelGGL(mean_gram_kernel<4>, grid, block, 0, s, R, z, c0, nr, nslab, partial);
  else if (K1 <= 8) hipLaunchKernelGGL(mean_gram_kernel<8>, grid, block, 0, s, R, z, c0, nr, nslab, partial);
  else hipLaunchKernelGGL(mean_gram_kernel<CLR_MAX_MEAN_RHS>, grid, block, 0, s, R, z, c0, nr, nslab, partial);
}

void launch_mean_gram_finish(const double* partial, int K, int B, int N, double* gram, hipStream_t s) {
  const long K1 = K + 1, total = (long)B * K1 * K1;
  hipLaunchKernelGGL(mean_gram_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, partial,
                     mean_project_slabs(N), (int)K1, total, gram);
}

size_t gram_solve_workspace(int B, int K) { return (size_t)B * (size_t)gram_solve_work(K); }

void launch_gram_solve(const double* gram, const double* w0, double min_pivot, int K, int B, double* out, int* status,
                       double* work, hipStream_t s) {
  hipLaunchKernelGGL(gram_solve_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, gram, w0, min_pivot, K, B, out, status, work);
}

void launch_linear_residual(const double* y, long y_stride, const double* phi, long phi_stride, const double* w, int K,
                            int nout, int N, double* r, hipStream_t s) {
  const int bx = std::min((N + 255) / 256, 64);
  hipLaunchKernelGGL(linear_residual_kernel, dim3(bx, std::min(nout, 65535)), dim3(256), 0, s, y, y_stride, phi,
                     phi_stride, w, K, nout, N, r);
}

bool launch_mean_project(const double* phi, long phi_stride, const double* z, int K, int B, int N, double* partial,
                         double* g, hipStream_t s) {
  return launch_slab_project(phi, phi_stride, SolveFactor{z}, K, B, N, partial, g, s);
}

void launch_slab_project_finish(const double* partial, int K, int B, int N, double* g, hipStream_t s) {
  const long BK = (long)B * K;
  hipLaunchKernelGGL(mean_project_finish_kernel, dim3((unsigned)((BK + 255) / 256)), dim3(256), 0, s, partial,
                     mean_project_slabs(N), K, BK, g);
}

}  // namespace clr
