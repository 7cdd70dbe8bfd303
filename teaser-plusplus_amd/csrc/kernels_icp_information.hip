// kernels_icp_information.hip -- the information matrix of registered pairs (Open3D's
// GetInformationMatrixFromPointClouds; the contract is written out in include/teaser_hip.h, "Information matrices")
// for gfx950: the reduction over the correspondences that icp_corr_kernel<0> left in the match array.
//
// Two launches.  icp_info_block_kernel runs over the block map of the correspondence pass (problem, kIcpBlock-point
// source chunk): a thread reads the match of its source point, gathers q = Q[j] from the targets as the caller gave
// them (B_Q: not the bucket order, not centred) and forms the 21 upper-triangle terms of G^T G, G = [-[q]x | I]; the
// block adds them in the fixed order of icp_block_sum (lanes by xor shuffles, then the four waves) and writes its
// partial.  icp_info_finalize_kernel (one workgroup per problem) adds the partials of the problem's blocks, thread t
// taking blocks t, t + 256, ... in ascending order, then the same block sum, and writes the symmetric 6 x 6.
// No floating-point atomics; the chunking and both orders depend on n_s alone, so a problem gives the same bits run
// to run, alone and inside any batch.  A kernel of its own: a fourth mode of icp_corr_kernel would change the
// registers of instantiations that are measured.
#include "icp_internal.h"

namespace thip {

namespace {

__device__ __forceinline__ double info_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sums v[0..kIcpInfoSums) over the 256 threads of the block in a fixed order; valid in thread k < kIcpInfoSums for
// its own k.
__device__ __forceinline__ double info_block_sum(const double (&v)[kIcpInfoSums], double (*s)[kIcpInfoSums]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kIcpInfoSums; ++k) {
    const double w = info_wave_sum(v[k]);
    if (lane == 0) s[wave][k] = w;
  }
  __syncthreads();
  const int k = threadIdx.x;
  return k < kIcpInfoSums ? (s[0][k] + s[1][k]) + (s[2][k] + s[3][k]) : 0.0;
}

}  // namespace

__global__ __launch_bounds__(kIcpBlock) void icp_info_block_kernel(const IcpDesc* __restrict__ descs,
                                                                   const int32_t* __restrict__ blk_prob,
                                                                   const double* __restrict__ q,
                                                                   const int32_t* __restrict__ match,
                                                                   double* __restrict__ partials) {
  static_assert(kIcpBlock == 256, "info_block_sum adds four waves");
  __shared__ double s[4][kIcpInfoSums];
  const int p = blk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const int64_t i = (int64_t)((int)blockIdx.x - d.blk_off) * kIcpBlock + threadIdx.x;
  double v[kIcpInfoSums];
#pragma unroll
  for (int k = 0; k < kIcpInfoSums; ++k) v[k] = 0.0;
  const int32_t j = i < d.n_s ? match[d.s_off + i] : -1;
  if (j >= 0) {  // j < n_t: written by the correspondence pass of this call
    const double* qp = q + 3 * (d.t_off + j);
    const double x = qp[0], y = qp[1], z = qp[2];
    // upper triangle of G^T G by rows; G rows: (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1)
    v[0] = z * z + y * y;   // (0,0)
    v[1] = 0.0 - y * x;     // (0,1)
    v[2] = 0.0 - z * x;     // (0,2)
    v[3] = 0.0;             // (0,3)
    v[4] = 0.0 - z;         // (0,4)
    v[5] = y + 0.0;         // (0,5)   (+ 0.0: a coordinate -0.0 enters as +0.0, like the products)
    v[6] = z * z + x * x;   // (1,1)
    v[7] = 0.0 - z * y;     // (1,2)
    v[8] = z + 0.0;         // (1,3)
    v[9] = 0.0;             // (1,4)
    v[10] = 0.0 - x;        // (1,5)
    v[11] = y * y + x * x;  // (2,2)
    v[12] = 0.0 - y;        // (2,3)
    v[13] = x + 0.0;        // (2,4)
    v[14] = 0.0;            // (2,5)
    v[15] = 1.0;            // (3,3)
    v[16] = 0.0;            // (3,4)
    v[17] = 0.0;            // (3,5)
    v[18] = 1.0;            // (4,4)
    v[19] = 0.0;            // (4,5)
    v[20] = 1.0;            // (5,5)
  }
  const double tot = info_block_sum(v, s);
  if (threadIdx.x < kIcpInfoSums) partials[(int64_t)blockIdx.x * kIcpInfoSums + threadIdx.x] = tot;
}

__global__ __launch_bounds__(256) void icp_info_finalize_kernel(const IcpDesc* __restrict__ descs,
                                                                const double* __restrict__ partials,
                                                                double* __restrict__ info) {
  __shared__ double s[4][kIcpInfoSums];
  __shared__ double tot[kIcpInfoSums];
  const int p = blockIdx.x;
  const IcpDesc& d = descs[p];
  double v[kIcpInfoSums];
#pragma unroll
  for (int k = 0; k < kIcpInfoSums; ++k) v[k] = 0.0;
  for (int b = threadIdx.x; b < d.nblk; b += 256) {
    const double* pb = partials + (int64_t)(d.blk_off + b) * kIcpInfoSums;
#pragma unroll
    for (int k = 0; k < kIcpInfoSums; ++k) v[k] += pb[k];
  }
  const double t = info_block_sum(v, s);
  if (threadIdx.x < kIcpInfoSums) tot[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x < 36) {  // row-major 6 x 6 from the upper triangle by rows
    const int r = threadIdx.x / 6, c = threadIdx.x % 6;
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    info[36 * (int64_t)p + threadIdx.x] = tot[6 * lo - lo * (lo - 1) / 2 + (hi - lo)];
  }
}

void launch_icp_information(hipStream_t s, const IcpDesc* d_desc, const int32_t* d_blk_prob, int n_blk, int batch,
                            const double* d_q, const int32_t* d_match, double* d_partials, double* d_info) {
  if (n_blk > 0)
    hipLaunchKernelGGL(icp_info_block_kernel, dim3(n_blk), dim3(kIcpBlock), 0, s, d_desc, d_blk_prob, d_q, d_match,
                       d_partials);
  hipLaunchKernelGGL(icp_info_finalize_kernel, dim3(batch), dim3(256), 0, s, d_desc, d_partials, d_info);
}

}  // namespace thip
