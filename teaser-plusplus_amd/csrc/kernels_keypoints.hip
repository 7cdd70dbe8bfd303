// kernels_keypoints.hip -- gfx950 kernels of ISS keypoint detection (include/teaser_hip.h, "ISS keypoints"; host side:
// icp_keypoints.hip; design and register table: DESIGN.md section 19).
//
// Per call, over the points of every cloud at once:
//   keys      one thread per point: its key in the grid of r_s and its key in the grid of r_n (icp_iss_device.h);
//   sort      rocprim's stable LSD radix sort of (key, entry) over the bits in use;
//   gather    the points in sorted order;
//   saliency  one query per lane in SORTED order, so the 64 queries of a wave walk the same runs: the uncapped
//             neighbourhood sum in ascending (c_x, c_y, c_z, j), ten FP64 accumulators in registers, the Jacobi, the two
//             ratio tests, one store;
//   suppress  count and "is any neighbour's saliency larger" over the r_n ball on the grid of r_n, the mask, and the
//             keypoint count (an integer atomic per wave: the count does not depend on the order).
// The bodies live in icp_iss_device.h; the kernels here are their shells.  No LDS, no floating-point atomics.
#include <rocprim/device/device_radix_sort.hpp>

#include "icp_iss_device.h"

namespace thip {

namespace {

__global__ __launch_bounds__(kIssBlock) void iss_keys_kernel(const IssDesc* __restrict__ descs,
                                                             const int32_t* __restrict__ blk_prob,
                                                             const double* __restrict__ pts, int64_t total,
                                                             int grids, uint64_t* __restrict__ key,
                                                             int32_t* __restrict__ iota) {
  iss_keys_grids_body(descs, blk_prob, pts, total, grids, key, iota);
}

__global__ __launch_bounds__(kIssBlock) void iss_gather_kernel(int64_t total, int64_t entries,
                                                               const double* __restrict__ pts,
                                                               const int32_t* __restrict__ sidx,
                                                               double* __restrict__ spts) {
  iss_gather_entries_body(total, entries, pts, sidx, spts);
}

__global__ __launch_bounds__(kIssBlock) void iss_saliency_kernel(const IssDesc* __restrict__ descs,
                                                                 const int32_t* __restrict__ blk_prob,
                                                                 const uint64_t* __restrict__ skey,
                                                                 const int32_t* __restrict__ sidx,
                                                                 const double* __restrict__ spts,
                                                                 double* __restrict__ sal, int32_t* __restrict__ count) {
  iss_saliency_body(descs, blk_prob, skey, sidx, spts, sal, count);
}

__global__ __launch_bounds__(kIssBlock) void iss_suppress_kernel(const IssDesc* __restrict__ descs,
                                                                 const int32_t* __restrict__ blk_prob, int64_t total,
                                                                 const uint64_t* __restrict__ skey,
                                                                 const int32_t* __restrict__ sidx,
                                                                 const double* __restrict__ spts,
                                                                 const double* __restrict__ sal,
                                                                 int32_t* __restrict__ count, uint8_t* __restrict__ keep,
                                                                 int32_t* __restrict__ kept) {
  int p = 0;
  const bool kp = iss_suppress_body(descs, blk_prob, total, skey, sidx, spts, sal, count, keep, p);
  const unsigned long long bal = __ballot(kp);  // a block holds one cloud: p is the same in every lane
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&kept[p], (int32_t)__popcll(bal));
}

__global__ __launch_bounds__(256) void iss_res_block_kernel(const IcpDesc* __restrict__ descs,
                                                            const IcpKnnDesc* __restrict__ knns,
                                                            const int32_t* __restrict__ tblk_prob, int n_tblk,
                                                            const double* __restrict__ d2,
                                                            double* __restrict__ partials) {
  iss_res_block_body(descs, knns, tblk_prob, n_tblk, d2, partials);
}

__global__ __launch_bounds__(256) void iss_res_reduce_kernel(const IcpDesc* __restrict__ descs, int batch,
                                                             const double* __restrict__ partials,
                                                             double* __restrict__ res) {
  iss_res_reduce_body(descs, batch, partials, res);
}

}  // namespace

size_t iss_sort_temp_bytes(int64_t entries) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                  (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)entries, 0, 64, (hipStream_t)0);
  return bytes;
}

hipError_t launch_iss_sort(hipStream_t s, void* d_temp, size_t temp_bytes, int64_t entries, int bits,
                           const uint64_t* d_key, const int32_t* d_iota, uint64_t* d_skey, int32_t* d_sidx) {
  size_t tb = temp_bytes;
  return rocprim::radix_sort_pairs(d_temp, tb, d_key, d_skey, d_iota, d_sidx, (size_t)entries, 0, (unsigned)bits, s);
}

void launch_iss_keys_grids(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                           const double* d_pts, int64_t total, int grids, uint64_t* d_key, int32_t* d_iota) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(iss_keys_kernel, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, d_pts, total, grids,
                     d_key, d_iota);
}

void launch_iss_keys(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk, const double* d_pts,
                     int64_t total, uint64_t* d_key, int32_t* d_iota) {
  launch_iss_keys_grids(s, d_desc, d_blk_prob, n_blk, d_pts, total, 2, d_key, d_iota);
}

void launch_iss_gather_entries(hipStream_t s, int64_t total, int64_t entries, const double* d_pts,
                               const int32_t* d_sidx, double* d_spts) {
  if (entries <= 0) return;
  hipLaunchKernelGGL(iss_gather_kernel, dim3((unsigned)((entries + kIssBlock - 1) / kIssBlock)), dim3(kIssBlock), 0, s,
                     total, entries, d_pts, d_sidx, d_spts);
}

void launch_iss_gather(hipStream_t s, int64_t total, const double* d_pts, const int32_t* d_sidx, double* d_spts) {
  launch_iss_gather_entries(s, total, 2 * total, d_pts, d_sidx, d_spts);
}

void launch_iss_saliency(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, double* d_sal,
                         int32_t* d_count) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(iss_saliency_kernel, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, d_skey, d_sidx,
                     d_spts, d_sal, d_count);
}

void launch_iss_suppress(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk, int64_t total,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, const double* d_sal,
                         int32_t* d_count, uint8_t* d_keep, int32_t* d_kept) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(iss_suppress_kernel, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, total, d_skey, d_sidx,
                     d_spts, d_sal, d_count, d_keep, d_kept);
}

void launch_iss_resolution(hipStream_t s, const IcpDesc* d_desc, const IcpKnnDesc* d_knn, const int32_t* d_tblk_prob,
                           int n_tblk, int batch, const double* d_d2, double* d_partials, double* d_res) {
  if (n_tblk <= 0) return;
  hipLaunchKernelGGL(iss_res_block_kernel, dim3((n_tblk + 255) / 256), dim3(256), 0, s, d_desc, d_knn, d_tblk_prob,
                     n_tblk, d_d2, d_partials);
  hipLaunchKernelGGL(iss_res_reduce_kernel, dim3((batch + 255) / 256), dim3(256), 0, s, d_desc, batch, d_partials,
                     d_res);
}

}  // namespace thip
