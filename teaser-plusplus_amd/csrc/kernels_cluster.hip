// kernels_cluster.hip -- gfx950 kernels of DBSCAN clustering (include/teaser_hip.h, "DBSCAN clustering"; host side:
// icp_cluster.hip; design, termination argument and register table: DESIGN.md section 26).
//
// Per call, over the points of every cloud at once, after the keys, the sort and the gather of kernels_keypoints.hip
// (one grid per cloud):
//   count     one query per lane in SORTED order, so the 64 queries of a wave walk the same runs: the number of points
//             with d2 < eps^2, and parent[g] = g;
//   union     the same walk by the core points: a lock-free unite with every core neighbour of smaller index, the larger
//             root hooked under the smaller by one 32-bit compare-and-swap;
//   flatten   one point per lane, reading only: its root, and the flag "is a root";
//   scan      rocprim's exclusive scan of the flags over total + 1 entries: the cluster numbers in ascending root;
//   label     core points take their root's number, the others walk the ball for the smallest root among their core
//             neighbours; the lane of a cloud's first position writes its cluster count.
// The bodies live in icp_dbscan_device.h; the kernels here are their shells.  No LDS, no floating-point atomics, no
// loop on the host: five launches and one scan whatever the data.
#include <rocprim/device/device_scan.hpp>

#include "icp_dbscan_device.h"

namespace thip {

namespace {

__global__ __launch_bounds__(kIssBlock) void dbscan_count_kernel(const IssDesc* __restrict__ descs,
                                                                 const int32_t* __restrict__ blk_prob,
                                                                 const uint64_t* __restrict__ skey,
                                                                 const int32_t* __restrict__ sidx,
                                                                 const double* __restrict__ spts,
                                                                 int32_t* __restrict__ count,
                                                                 int32_t* __restrict__ parent) {
  dbscan_count_body(descs, blk_prob, skey, sidx, spts, count, parent);
}

__global__ __launch_bounds__(kIssBlock) void dbscan_union_kernel(const IssDesc* __restrict__ descs,
                                                                 const int32_t* __restrict__ blk_prob,
                                                                 const uint64_t* __restrict__ skey,
                                                                 const int32_t* __restrict__ sidx,
                                                                 const double* __restrict__ spts,
                                                                 const int32_t* __restrict__ count,
                                                                 int32_t* __restrict__ parent) {
  dbscan_union_body(descs, blk_prob, skey, sidx, spts, count, parent);
}

__global__ __launch_bounds__(kIssBlock) void dbscan_flatten_kernel(const IssDesc* __restrict__ descs,
                                                                   const int32_t* __restrict__ blk_prob,
                                                                   const int32_t* __restrict__ count,
                                                                   const int32_t* __restrict__ parent,
                                                                   int32_t* __restrict__ root,
                                                                   int32_t* __restrict__ is_root) {
  dbscan_flatten_body(descs, blk_prob, count, parent, root, is_root);
}

__global__ __launch_bounds__(kIssBlock) void dbscan_label_kernel(const IssDesc* __restrict__ descs,
                                                                 const int32_t* __restrict__ blk_prob,
                                                                 const uint64_t* __restrict__ skey,
                                                                 const int32_t* __restrict__ sidx,
                                                                 const double* __restrict__ spts,
                                                                 const int32_t* __restrict__ root,
                                                                 const int32_t* __restrict__ scan,
                                                                 int32_t* __restrict__ label,
                                                                 int32_t* __restrict__ n_clusters) {
  dbscan_label_body(descs, blk_prob, skey, sidx, spts, root, scan, label, n_clusters);
}

}  // namespace

size_t dbscan_scan_temp_bytes(int64_t entries) {
  size_t bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, bytes, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, (size_t)entries,
                                rocprim::plus<int32_t>(), (hipStream_t)0);
  return bytes;
}

hipError_t launch_dbscan_scan(hipStream_t s, void* d_temp, size_t temp_bytes, int64_t entries, const int32_t* d_flag,
                              int32_t* d_scan) {
  size_t tb = temp_bytes;
  return rocprim::exclusive_scan(d_temp, tb, d_flag, d_scan, (int32_t)0, (size_t)entries, rocprim::plus<int32_t>(), s);
}

void launch_dbscan_count(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, int32_t* d_count,
                         int32_t* d_parent) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(dbscan_count_kernel, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, d_skey, d_sidx,
                     d_spts, d_count, d_parent);
}

void launch_dbscan_union(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, const int32_t* d_count,
                         int32_t* d_parent) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(dbscan_union_kernel, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, d_skey, d_sidx,
                     d_spts, d_count, d_parent);
}

void launch_dbscan_flatten(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                           const int32_t* d_count, const int32_t* d_parent, int32_t* d_root, int32_t* d_is_root) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(dbscan_flatten_kernel, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, d_count, d_parent,
                     d_root, d_is_root);
}

void launch_dbscan_label(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, const int32_t* d_root,
                         const int32_t* d_scan, int32_t* d_label, int32_t* d_n_clusters) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(dbscan_label_kernel, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, d_skey, d_sidx,
                     d_spts, d_root, d_scan, d_label, d_n_clusters);
}

}  // namespace thip
