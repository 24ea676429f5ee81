// celerite_amd/csrc/amplitude_kernels.hip -- the passes of a per-sample amplitude model on batched plans
// (clr_bamplitude_kernels.h).
#include "clr_bamplitude_kernels.h"

#include <algorithm>

namespace clr {
namespace {

// V doubles per access: 2 (16 bytes) where every row starts 16-byte aligned (N even), else 1
template <int V>
struct Pack;
template <>
struct Pack<1> { using type = double; };
template <>
struct Pack<2> { using type = double2; };

// The scale of clr_batch_set_amplitudes and its log term.  Contraction is off for this function (and for the unit:
// Makefile), as for noise_form_kernel: the result is the bits of
//   s = a[:, 0, None] * Gamma[0];  s = s + a[:, k, None] * Gamma[k]  (k = 1 .. K - 1)
// One workgroup per (problem, slab of CLR_MEAN_SLAB samples), as slab_project_kernel: thread i takes the V consecutive
// samples at V (i + 256 j), j = 0, 1, ... in order and adds their log|s| in that order; then the shuffle tree of each wave,
// the four waves in order through LDS.  Inside the problem's length a zero or non-finite s_n raises the slab's flag and is
// replaced by 1 (no infinity enters a scan); past it s is 1 and adds nothing -- Gamma's tail may hold anything.
template <int V>
__global__ void __launch_bounds__(256) amplitude_scale_kernel(const double* __restrict__ gamma, long gamma_stride,
                                                              const double* __restrict__ a, int K, int N,
                                                              const int* __restrict__ len, long nslab,
                                                              double* __restrict__ s, double* __restrict__ partial) {
#pragma clang fp contract(off)
  using P = typename Pack<V>::type;
  __shared__ double sh[4];
  __shared__ int shf[4];
  const long b = blockIdx.x / nslab, slab = blockIdx.x % nslab;
  const int nb = len ? len[b] : N;
  const double* ab = a + b * K;
  const double* gb = gamma + b * gamma_stride;
  double* sb = s + b * (long)N;
  double acc = 0.0;
  int bad = 0;
  for (int j = 0; j < CLR_MEAN_SLAB / (256 * V); ++j) {
    const long n = slab * CLR_MEAN_SLAB + ((long)j * 256 + threadIdx.x) * V;
    if (n >= N) break;  // (V == 2 only with N even: n + 1 < N too)
    P pk = *reinterpret_cast<const P*>(gb + n);
    const double* pv = reinterpret_cast<const double*>(&pk);
    double m[V];
    const double a0 = ab[0];
#pragma unroll
    for (int v = 0; v < V; ++v) m[v] = a0 * pv[v];
    for (int k = 1; k < K; ++k) {
      pk = *reinterpret_cast<const P*>(gb + (long)k * N + n);
      const double ak = ab[k];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const double term = ak * pv[v];
        m[v] = m[v] + term;
      }
    }
    P out;
    double* o = reinterpret_cast<double*>(&out);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      double sv = 1.0;
      if (n + v < nb) {
        sv = m[v];
        if (sv == 0.0 || !(fabs(sv) <= 1.7976931348623157e308)) {  // (zero, infinite or NaN)
          bad = 1;
          sv = 1.0;
        }
        acc = acc + log(fabs(sv));
      }
      o[v] = sv;
    }
    *reinterpret_cast<P*>(sb + n) = out;
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  const int any = __any(bad);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh[wave] = acc;
    shf[wave] = any;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[2 * (long)blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    partial[2 * (long)blockIdx.x + 1] = (shf[0] | shf[1] | shf[2] | shf[3]) ? 1.0 : 0.0;
  }
}

// Lf[b] = the slabs' log sums added in slab order, Lf[B + b] = whether any slab raised its flag: one thread per problem
__global__ void __launch_bounds__(256) amplitude_scale_finish_kernel(const double* __restrict__ partial, long nslab, int B,
                                                                     double* __restrict__ Lf) {
#pragma clang fp contract(off)
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double sum = 0.0, flag = 0.0;
  for (long i = 0; i < nslab; ++i) {
    sum = sum + partial[2 * (b * nslab + i)];
    if (partial[2 * (b * nslab + i) + 1] != 0.0) flag = 1.0;
  }
  Lf[b] = sum;
  Lf[B + b] = flag;
}

// y' = r / s and d' = d / (s * s), the product and the quotients rounded on their own.  A source may be its destination
// (the residual of a linear mean, the variances of a noise model): a thread reads what it overwrites before it does.
// Grid (slab of samples, problem): a thread takes V consecutive samples, a wave 512 V contiguous bytes of each array.
template <int V>
__global__ void __launch_bounds__(256) amplitude_divide_kernel(const double* ysrc, long ysrc_stride, double* y,
                                                               const double* dsrc, long dsrc_stride, double* d,
                                                               const double* __restrict__ s, int B, int N) {
#pragma clang fp contract(off)
  using P = typename Pack<V>::type;
  const long NV = N / V;  // (V == 2 only with N even)
  for (long b = blockIdx.y; b < B; b += gridDim.y) {
    const P* sp = reinterpret_cast<const P*>(s + b * (long)N);
    const P* yi = reinterpret_cast<const P*>(ysrc + b * ysrc_stride);
    const P* di = reinterpret_cast<const P*>(dsrc + b * dsrc_stride);
    P* yo = reinterpret_cast<P*>(y + b * (long)N);
    P* dout = reinterpret_cast<P*>(d + b * (long)N);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < NV; i += (long)gridDim.x * blockDim.x) {
      const P sk = sp[i];
      const double* sv = reinterpret_cast<const double*>(&sk);
      if (y) {
        P yk = yi[i];
        double* o = reinterpret_cast<double*>(&yk);
#pragma unroll
        for (int v = 0; v < V; ++v) o[v] = o[v] / sv[v];
        yo[i] = yk;
      }
      if (d) {
        P dk = di[i];
        double* o = reinterpret_cast<double*>(&dk);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const double ss = sv[v] * sv[v];
          o[v] = o[v] / ss;
        }
        dout[i] = dk;
      }
    }
  }
}

// the per-sample factor of clr_batch_grad_amplitudes' projection (slab_project_kernel):
// (alpha' y' + d' (c' - alpha'^2) - 1) / s, every operation rounded on its own
struct AmplitudeFactor {
  const double* alpha;
  const double* c;
  const double* y;
  const double* d;
  const double* s;
  __device__ double operator()(long i) const {
#pragma clang fp contract(off)
    const double a = alpha[i];
    const double ay = a * y[i];
    const double aa = a * a;
    const double diff = c[i] - aa;
    const double dd = d[i] * diff;
    const double num = (ay + dd) - 1.0;
    return num / s[i];
  }
};

// ... of clr_batch_grad_mean_weights with amplitudes in force: alpha_y = alpha' / s
struct ScaledSolveFactor {
  const double* z;
  const double* s;
  __device__ double operator()(long i) const { return z[i] / s[i]; }
};

// ... of clr_batch_grad_noise_weights with amplitudes in force: 1/2 (alpha'^2 - c') / s^2
struct ScaledNoiseFactor {
  const double* alpha;
  const double* c;
  const double* s;
  __device__ double operator()(long i) const {
#pragma clang fp contract(off)
    const double a = alpha[i];
    const double aa = a * a;
    const double sv = s[i];
    const double ss = sv * sv;
    return 0.5 * (aa - c[i]) / ss;
  }
};

}  // namespace

bool launch_amplitude_scale(const double* gamma, long gamma_stride, const double* a, int K, int B, int N, const int* len,
                            double* s, double* partial, double* Lf, hipStream_t stream) {
  const long nslab = mean_project_slabs(N), blocks = (long)B * nslab;
  if (blocks > 2147483647L) return false;
  const dim3 grid((unsigned)blocks), block(256);
  if (N % 2 == 0)
    hipLaunchKernelGGL(amplitude_scale_kernel<2>, grid, block, 0, stream, gamma, gamma_stride, a, K, N, len, nslab, s, partial);
  else
    hipLaunchKernelGGL(amplitude_scale_kernel<1>, grid, block, 0, stream, gamma, gamma_stride, a, K, N, len, nslab, s, partial);
  hipLaunchKernelGGL(amplitude_scale_finish_kernel, dim3((unsigned)((B + 255) / 256)), block, 0, stream, partial, nslab, B, Lf);
  return true;
}

void launch_amplitude_divide(const double* ysrc, long ysrc_stride, double* y, const double* dsrc, long dsrc_stride, double* d,
                             const double* s, int B, int N, hipStream_t stream) {
  const int V = (N % 2 == 0) ? 2 : 1;
  const int bx = std::min((N / V + 255) / 256, 64);
  const dim3 grid((unsigned)std::max(bx, 1), (unsigned)std::min(B, 65535)), block(256);
  if (V == 2)
    hipLaunchKernelGGL(amplitude_divide_kernel<2>, grid, block, 0, stream, ysrc, ysrc_stride, y, dsrc, dsrc_stride, d, s, B, N);
  else
    hipLaunchKernelGGL(amplitude_divide_kernel<1>, grid, block, 0, stream, ysrc, ysrc_stride, y, dsrc, dsrc_stride, d, s, B, N);
}

bool launch_amplitude_project(const double* gamma, long gamma_stride, const double* alpha, const double* c, const double* y,
                              const double* d, const double* s, int K, int B, int N, double* partial, double* g,
                              hipStream_t stream) {
  return launch_slab_project(gamma, gamma_stride, AmplitudeFactor{alpha, c, y, d, s}, K, B, N, partial, g, stream);
}

bool launch_mean_project_scaled(const double* phi, long phi_stride, const double* z, const double* s, int K, int B, int N,
                                double* partial, double* g, hipStream_t stream) {
  return launch_slab_project(phi, phi_stride, ScaledSolveFactor{z, s}, K, B, N, partial, g, stream);
}

bool launch_noise_project_scaled(const double* psi, long psi_stride, const double* alpha, const double* c, const double* s,
                                 int K, int B, int N, double* partial, double* g, hipStream_t stream) {
  return launch_slab_project(psi, psi_stride, ScaledNoiseFactor{alpha, c, s}, K, B, N, partial, g, stream);
}

}  // namespace clr
