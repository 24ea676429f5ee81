// celerite_amd/csrc/mean_kernels.hip -- the two passes of a linear mean model on batched plans (clr_bmean_kernels.h).
#include "clr_bmean_kernels.h"

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

// One workgroup per (problem, slab): thread i takes the samples i, i + 256, ... of the slab in order, K running sums in
// registers (KT: the instantiation's register count, K <= KT); then the shuffle tree of each wave, the four waves in
// order through LDS.  A ragged last slab adds nothing for n >= N.
template <int KT>
__global__ void __launch_bounds__(256) mean_project_kernel(const double* __restrict__ phi, long phi_stride,
                                                           const double* __restrict__ z, int K, int N, long nslab,
                                                           double* __restrict__ partial) {
  __shared__ double sh[4][KT];
  const long b = blockIdx.x / nslab, slab = blockIdx.x % nslab;
  const double* zb = z + b * (long)N;
  const double* pb = phi + b * phi_stride;
  double acc[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) acc[k] = 0.0;
  const long n0 = slab * CLR_MEAN_SLAB + threadIdx.x;
#pragma unroll 4
  for (int i = 0; i < CLR_MEAN_SLAB / 256; ++i) {
    const long n = n0 + i * 256;
    if (n < N) {
      const double zn = zb[n];
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

}  // namespace

void launch_linear_residual(const double* y, long y_stride, const double* phi, long phi_stride, const double* w, int K,
                            int nout, int N, double* r, hipStream_t s) {
  const int bx = std::min((N + 255) / 256, 64);
  hipLaunchKernelGGL(linear_residual_kernel, dim3(bx, std::min(nout, 65535)), dim3(256), 0, s, y, y_stride, phi,
                     phi_stride, w, K, nout, N, r);
}

bool launch_mean_project(const double* phi, long phi_stride, const double* z, int K, int B, int N, double* partial,
                         double* g, hipStream_t s) {
  const long nslab = mean_project_slabs(N), blocks = (long)B * nslab, BK = (long)B * K;
  if (blocks > 2147483647L) return false;
  const dim3 grid((unsigned)blocks), block(256);
  if (K <= 4) hipLaunchKernelGGL(mean_project_kernel<4>, grid, block, 0, s, phi, phi_stride, z, K, N, nslab, partial);
  else if (K <= 8) hipLaunchKernelGGL(mean_project_kernel<8>, grid, block, 0, s, phi, phi_stride, z, K, N, nslab, partial);
  else hipLaunchKernelGGL(mean_project_kernel<16>, grid, block, 0, s, phi, phi_stride, z, K, N, nslab, partial);
  hipLaunchKernelGGL(mean_project_finish_kernel, dim3((unsigned)((BK + 255) / 256)), block, 0, s, partial, nslab, K, BK, g);
  return true;
}

}  // namespace clr
