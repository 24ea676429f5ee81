// celerite_amd/csrc/information_kernels.hip -- the Gram pass of clr_batch_information (clr_binfo_kernels.h): I_b = R_b R_b^T
// over the 2 C cells of every direction's row, M <= CLR_INFO_MAX_M rows.  The pattern of the linear mean's Gram pass
// (mean_kernels.hip): slabs of a fixed size, every sum in a fixed order, no atomics.
#include "clr_batch_kernels.h"

namespace clr {

// workgroup = (slab, problem of the tile).  The slab's cells go through LDS CLR_INFO_TILE at a time (rows padded by one
// double: the threads of a wave read different rows at the same cell); thread p < M (M + 1) / 2 owns entry (i, j), i <= j,
// of the upper triangle and adds the products cell by cell.  Cells past 2 C are staged as zeros.
__global__ void __launch_bounds__(256) info_gram_kernel(const BInfoParams I) {
  __shared__ double T[CLR_INFO_MAX_M][CLR_INFO_TILE + 1];
  const int slab = blockIdx.x, bl = blockIdx.y, tid = threadIdx.x, M = I.M, NP = M * (M + 1) / 2;
  const long W = 2 * I.C, k_lo = (long)slab * CLR_INFO_SLAB, k_hi = k_lo + CLR_INFO_SLAB < W ? k_lo + CLR_INFO_SLAB : W;
  const double* R = I.rows + (long)bl * M * W;
  int i = 0, j = 0;
  {  // p -> (i, j): column j of the packed upper triangle holds j + 1 entries
    int p = tid;
    while (j < M && p > j) { p -= j + 1; ++j; }
    i = p;
  }
  const bool mine = tid < NP;
  double acc = 0.0;
  for (long k0 = k_lo; k0 < k_hi; k0 += CLR_INFO_TILE) {
    for (int e = tid; e < M * CLR_INFO_TILE; e += 256) {
      const int r = e / CLR_INFO_TILE, k = e % CLR_INFO_TILE;
      T[r][k] = k0 + k < k_hi ? R[(long)r * W + k0 + k] : 0.0;
    }
    __syncthreads();
    if (mine) {
#pragma unroll 8
      for (int k = 0; k < CLR_INFO_TILE; ++k) acc = fma(T[i][k], T[j][k], acc);
    }
    __syncthreads();
  }
  if (mine) I.part[((long)bl * I.nslab + slab) * NP + tid] = acc;
}

// one workgroup per problem of the tile: the slabs in order; both triangles are written from the one sum
__global__ void __launch_bounds__(256) info_gram_finish_kernel(const BInfoParams I) {
  const int bl = blockIdx.x, tid = threadIdx.x, M = I.M, NP = M * (M + 1) / 2;
  if (tid >= NP) return;
  int i = 0, j = 0;
  {
    int p = tid;
    while (j < M && p > j) { p -= j + 1; ++j; }
    i = p;
  }
  const double* part = I.part + (long)bl * I.nslab * NP + tid;
  double acc = 0.0;
  for (int s = 0; s < I.nslab; ++s) acc += part[(long)s * NP];
  double* out = I.out + (long)bl * M * M;
  out[i * M + j] = acc;
  out[j * M + i] = acc;
}

void launch_info_gram(const BInfoParams& I, hipStream_t s) {
  hipLaunchKernelGGL(info_gram_kernel, dim3(I.nslab, I.nb), dim3(256), 0, s, I);
  hipLaunchKernelGGL(info_gram_finish_kernel, dim3(I.nb), dim3(256), 0, s, I);
}

}  // namespace clr
