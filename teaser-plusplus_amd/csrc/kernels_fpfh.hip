// kernels_fpfh.hip -- the Open3D-form FPFH for gfx950 (include/teaser_hip.h, "FPFH (Open3D form)"; device code:
// icp_fpfh_device.h; host side: icp_fpfh.hip; design and the resource report: DESIGN.md section 29).
//
// The neighbour lists are written by the search kernels of kernels_search.hip with the cloud as its own query set.  A
// "piece" is a run of points of one cloud whose lists fit the list scratch: an IcpDesc (n_s points from s_off of the
// packed points; the cloud is its "target" at t_off) and an IcpSearchDesc (k = max_nn slots per row from out_off of the
// list scratch).  A launch covers the map blocks of the hybrid pieces, then those of the k-NN pieces; each kind counts
// its blocks from its own start, as the search launches do.
//
// SPFH: one thread per point.  The 33 bins of the 64 points of a block lie in LDS, bin-major, so a thread's bin is
// addressed at run time without a register array, and the block stores its 64 finished rows as one contiguous run.
// FPFH: one wave per point, four waves per block.  Lane l < 33 owns bin l and walks the list in order; a neighbour's SPFH
// row is one 264-byte load.  The sum S[g] of group g is ONE chain over (neighbour, then bin inside the group): every lane
// of the group reads the group's 11 terms in order through cross-lane reads and carries the same chain, so no lane has
// to broadcast it afterwards.  No atomics, no scratch, launches independent of the data.
#include "icp_fpfh_device.h"
#include "icp_internal.h"

namespace thip {

__global__ __launch_bounds__(kIcpCovBlock) void icp_fpfh_spfh_kernel(
    const IcpDesc* __restrict__ descs, const IcpSearchDesc* __restrict__ sds, const int32_t* __restrict__ blk_prob,
    int n_hyb, const double* __restrict__ q, const double* __restrict__ normals, const int32_t* __restrict__ list_idx,
    double* __restrict__ spfh) {
  __shared__ double hist[kFpfhDim][kIcpCovBlock];  // bin-major: lane l owns hist[.][l]
  int64_t i0;
  const int p = list_block_piece(descs, blk_prob, n_hyb, &i0);
  const IcpDesc& d = descs[p];
  const IcpSearchDesc& sd = sds[p];
  const int lane = threadIdx.x;
  const int64_t i = i0 + lane;
  for (int j = 0; j < kFpfhDim; ++j) hist[j][lane] = 0.0;
  if (i < d.n_s) {
    const int32_t* idx = list_idx + sd.out_off + i * sd.k;
    const int m = fpfh_list_length(idx, sd.k);
    // the cloud's own arrays begin at t_off; the piece's point i is the cloud's point (s_off - t_off) + i
    fpfh_spfh_row(q + 3 * d.t_off, normals + 3 * d.t_off, (d.s_off - d.t_off) + i, idx, m, &hist[0][lane], kIcpCovBlock);
  }
  __syncthreads();
  const int64_t left = d.n_s - i0;
  const int rows = left < kIcpCovBlock ? (int)left : kIcpCovBlock;
  double* out = spfh + kFpfhDim * (d.s_off + i0);
  for (int e = lane; e < rows * kFpfhDim; e += kIcpCovBlock) out[e] = hist[e % kFpfhDim][e / kFpfhDim];
}

__global__ __launch_bounds__(kIcpCovBlock* kFpfhWaves) void icp_fpfh_kernel(
    const IcpDesc* __restrict__ descs, const IcpSearchDesc* __restrict__ sds, const int32_t* __restrict__ blk_prob,
    int n_hyb, const int32_t* __restrict__ list_idx, const double* __restrict__ list_d2,
    const double* __restrict__ spfh, double* __restrict__ fpfh) {
  int64_t i0;
  const int p = list_block_piece(descs, blk_prob, n_hyb, &i0);
  const IcpDesc& d = descs[p];
  const IcpSearchDesc& sd = sds[p];
  const int lane = threadIdx.x % kIcpCovBlock, wave = threadIdx.x / kIcpCovBlock;
  const bool owner = lane < kFpfhDim;
  const int bin = owner ? lane : 0;                 // the idle lanes read bin 0 and store nothing
  const int first = owner ? lane / kFpfhBins * kFpfhBins : 0;  // the first lane of this lane's group
  const double* cloud = spfh + kFpfhDim * d.t_off;  // the SPFH rows of the cloud, by its own indices
  for (int t = wave; t < kIcpCovBlock; t += kFpfhWaves) {  // uniform over the wave
    const int64_t i = i0 + t;
    if (i >= d.n_s) break;
    const int32_t* idx = list_idx + sd.out_off + i * sd.k;
    const double* d2 = list_d2 + sd.out_off + i * sd.k;
    const int m = fpfh_list_length(idx, sd.k);
    double F = 0.0, S = 0.0;
    for (int k = 1; k < m; ++k) {
      const double dk = d2[k];
      if (dk == 0.0) continue;
      const double val = fpfh_term(cloud[(int64_t)kFpfhDim * idx[k] + bin], dk);
#pragma unroll
      for (int j = 0; j < kFpfhBins; ++j) S += __shfl(val, first + j, kIcpCovBlock);
      F += val;
    }
    if (owner) {
      const double own = spfh[kFpfhDim * (d.s_off + i) + bin];
      fpfh[kFpfhDim * (d.s_off + i) + bin] = m <= 1 ? 0.0 : fpfh_finish(F, fpfh_scale(S), own);
    }
  }
}

void launch_icp_fpfh_spfh(hipStream_t s, const IcpDesc* d_desc, const IcpSearchDesc* d_sd, const int32_t* d_blk_prob,
                          int n_hyb, int n_knn, const double* d_q, const double* d_normals, const int32_t* d_list_idx,
                          double* d_spfh) {
  if (n_hyb + n_knn <= 0) return;
  hipLaunchKernelGGL(icp_fpfh_spfh_kernel, dim3(n_hyb + n_knn), dim3(kIcpCovBlock), 0, s, d_desc, d_sd, d_blk_prob,
                     n_hyb, d_q, d_normals, d_list_idx, d_spfh);
}

void launch_icp_fpfh(hipStream_t s, const IcpDesc* d_desc, const IcpSearchDesc* d_sd, const int32_t* d_blk_prob,
                     int n_hyb, int n_knn, const int32_t* d_list_idx, const double* d_list_d2, const double* d_spfh,
                     double* d_fpfh) {
  if (n_hyb + n_knn <= 0) return;
  hipLaunchKernelGGL(icp_fpfh_kernel, dim3(n_hyb + n_knn), dim3(kIcpCovBlock * kFpfhWaves), 0, s, d_desc, d_sd,
                     d_blk_prob, n_hyb, d_list_idx, d_list_d2, d_spfh, d_fpfh);
}

}  // namespace thip
