// celerite_amd/csrc/noise_kernels.hip -- the two passes of a linear noise model on batched plans (clr_bnoise_kernels.h).
#include "clr_bnoise_kernels.h"

#include <algorithm>

namespace clr {
namespace {

// V doubles per access: 2 (16 bytes) where every row of src, psi and out starts 16-byte aligned, else 1
template <int V>
struct Pack;
template <>
struct Pack<1> { using type = double; };
template <>
struct Pack<2> { using type = double2; };

// The variances of clr_batch_set_noise_weights.  Contraction is off for this function (and for the unit: Makefile), as for
// linear_residual_kernel (mean_kernels.hip): hipcc would otherwise fuse s_k Psi_k into the running sum, and the result
// would no longer be the bits of
//   m = s[:, 0, None] * Psi[0];  m = m + s[:, k, None] * Psi[k]  (k = 1 .. K - 1);  diag_eff = diag + m
// Grid (slab of samples, problem): a thread takes V consecutive samples, a wave 512 V contiguous bytes of each array.
template <int V>
__global__ void __launch_bounds__(256) noise_form_kernel(const double* __restrict__ src, long src_stride,
                                                         const double* __restrict__ psi, long psi_stride,
                                                         const double* __restrict__ s, int K, int B, int N,
                                                         double* __restrict__ out) {
#pragma clang fp contract(off)
  using P = typename Pack<V>::type;
  const long NV = N / V;  // (V == 2 only with N even)
  for (long b = blockIdx.y; b < B; b += gridDim.y) {
    const double* sb = s + b * K;
    const P* d = reinterpret_cast<const P*>(src + b * src_stride);
    const P* basis = reinterpret_cast<const P*>(psi + b * psi_stride);
    P* dst = reinterpret_cast<P*>(out + b * (long)N);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < NV; i += (long)gridDim.x * blockDim.x) {
      P pk = basis[i];
      double m[V];
      const double* pv = reinterpret_cast<const double*>(&pk);
      const double s0 = sb[0];
#pragma unroll
      for (int v = 0; v < V; ++v) m[v] = s0 * pv[v];
      for (int k = 1; k < K; ++k) {
        pk = basis[(long)k * NV + i];
        const double sk = sb[k];
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const double term = sk * pv[v];
          m[v] = m[v] + term;
        }
      }
      P dv = d[i];
      double* o = reinterpret_cast<double*>(&dv);
#pragma unroll
      for (int v = 0; v < V; ++v) o[v] = o[v] + m[v];
      dst[i] = dv;
    }
  }
}

// the per-sample factor of clr_batch_grad_noise_weights' projection (slab_project_kernel): 1/2 (alpha^2 - c), the square
// and the difference rounded on their own (the halving is exact)
struct NoiseFactor {
  const double* alpha;
  const double* c;
  __device__ double operator()(long i) const {
#pragma clang fp contract(off)
    const double a = alpha[i];
    const double aa = a * a;
    return 0.5 * (aa - c[i]);
  }
};

}  // namespace

void launch_noise_form(const double* src, long src_stride, const double* psi, long psi_stride, const double* s, int K, int B,
                       int N, double* out, hipStream_t stream) {
  const int V = (N % 2 == 0) ? 2 : 1;
  const int bx = std::min((N / V + 255) / 256, 64);
  const dim3 grid((unsigned)std::max(bx, 1), (unsigned)std::min(B, 65535)), block(256);
  if (V == 2) hipLaunchKernelGGL(noise_form_kernel<2>, grid, block, 0, stream, src, src_stride, psi, psi_stride, s, K, B, N, out);
  else hipLaunchKernelGGL(noise_form_kernel<1>, grid, block, 0, stream, src, src_stride, psi, psi_stride, s, K, B, N, out);
}

bool launch_noise_project(const double* psi, long psi_stride, const double* alpha, const double* c, int K, int B, int N,
                          double* partial, double* g, hipStream_t stream) {
  return launch_slab_project(psi, psi_stride, NoiseFactor{alpha, c}, K, B, N, partial, g, stream);
}

}  // namespace clr
