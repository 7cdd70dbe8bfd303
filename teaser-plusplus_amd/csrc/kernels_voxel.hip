// kernels_voxel.hip -- gfx950 kernels of the batched voxel down-sampling (include/teaser_hip.h, "Voxel
// down-sampling"; host side: voxel.hip).
//
// Per call, over the points of every problem at once:
//   keys    one thread per point: the 128-bit key (problem, i_x, i_y, i_z), packed with as many bits per axis as
//           each problem's grid needs, and the identity permutation;
//   sort    rocprim's stable LSD radix sort of (key, point index) over the bits in use: one pass when they fit in
//           64 bits, otherwise a pass over the low word and a stable pass over the high word;
//   runs    the sorted points, run heads (key differs from the previous one), run ids (inclusive scan of the heads)
//           and run starts;
//   reduce  per problem its first run and run count; per run (= voxel) the FP64 sum of its points in sorted order,
//           which is input order (the sort is stable), then the mean and the count: a lane per short run, a wave
//           per long one;
//   trace   optionally the output voxel of every input point.
// Nothing uses atomics: every output is a function of the input alone, so results do not depend on the batch.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "voxel_internal.h"

namespace thip {

namespace {

__global__ __launch_bounds__(kVoxBlock) void vox_keys(const VoxDesc* __restrict__ desc,
                                                      const int32_t* __restrict__ blk_prob,
                                                      const double* __restrict__ pts, int prob_shift,
                                                      uint64_t* __restrict__ key_lo, uint64_t* __restrict__ key_hi,
                                                      int32_t* __restrict__ iota) {
  const int b = blk_prob[blockIdx.x];
  const VoxDesc d = desc[b];
  const int64_t local = (int64_t)(blockIdx.x - d.blk_off) * kVoxBlock + threadIdx.x;
  if (local >= d.n) return;
  const int64_t i = d.off + local;
  uint64_t lo = 0, hi = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) vox_put(lo, hi, vox_index(pts[3 * i + c], d.lo[c], d.v), d.shift[c]);
  vox_put(lo, hi, (uint64_t)b, prob_shift);
  key_lo[i] = lo;
  if (key_hi) key_hi[i] = hi;
  iota[i] = (int32_t)i;
}

__global__ __launch_bounds__(256) void vox_gather_hi(int64_t n, const uint64_t* __restrict__ key_hi,
                                                     const int32_t* __restrict__ perm, uint64_t* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) out[j] = key_hi[perm[j]];
}

__global__ __launch_bounds__(256) void vox_heads(int64_t n, int two_words, const double* __restrict__ pts,
                                                 const uint64_t* __restrict__ key_lo,
                                                 const uint64_t* __restrict__ key_hi,
                                                 const int32_t* __restrict__ perm, double* __restrict__ sorted_pts,
                                                 int32_t* __restrict__ head) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int64_t p = perm[j];
  for (int c = 0; c < 3; ++c) sorted_pts[3 * j + c] = pts[3 * p + c];
  int h = 1;
  if (j > 0) {
    const int64_t q = perm[j - 1];
    h = key_lo[p] != key_lo[q] || (two_words && key_hi[p] != key_hi[q]);
  }
  head[j] = h;
}

__global__ __launch_bounds__(256) void vox_starts(int64_t n, const int32_t* __restrict__ head,
                                                  const int32_t* __restrict__ run_id,
                                                  int32_t* __restrict__ run_start) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  if (head[j]) run_start[run_id[j] - 1] = (int32_t)j;
  if (j == n - 1) run_start[run_id[j]] = (int32_t)n;
}

__global__ __launch_bounds__(256) void vox_summary(const VoxDesc* __restrict__ desc, int batch,
                                                   const int32_t* __restrict__ run_id,
                                                   int32_t* __restrict__ summary) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  const VoxDesc d = desc[b];
  int32_t first = 0, count = 0;
  if (d.n > 0) {
    first = run_id[d.off] - 1;
    count = run_id[d.off + d.n - 1] - run_id[d.off] + 1;
  }
  summary[2 * b] = first;
  summary[2 * b + 1] = count;
}

// Short runs (at most kVoxLaneRun points): one lane per run, adding its points one at a time.
__global__ __launch_bounds__(256) void vox_sums_short(int64_t n, const int32_t* __restrict__ run_id,
                                                      const int32_t* __restrict__ run_start,
                                                      const double* __restrict__ sp, double* __restrict__ mean,
                                                      int32_t* __restrict__ count) {
  const int64_t runs = run_id[n - 1];
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= runs) return;
  const int32_t s = run_start[r], e = run_start[r + 1];
  if (e - s > kVoxLaneRun) return;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int32_t k = s; k < e; ++k) {
    sx += sp[3 * (int64_t)k];
    sy += sp[3 * (int64_t)k + 1];
    sz += sp[3 * (int64_t)k + 2];
  }
  const double cnt = (double)(e - s);
  mean[3 * r] = sx / cnt;
  mean[3 * r + 1] = sy / cnt;
  mean[3 * r + 2] = sz / cnt;
  count[r] = e - s;
}

__device__ __forceinline__ double vox_readlane(double x, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), lane),
                          __builtin_amdgcn_readlane(__double2loint(x), lane));
}

// Long runs: one wave per run (grid-stride over the runs).  The lanes load 64 consecutive points at a time; every lane
// then adds them in order from the broadcast values, so all lanes hold the same sum and lane 0 stores it.  The cost of
// a run is about one dependent FP64 add per point, so one voxel holding a whole cloud stays in the milliseconds, and
// distinct long runs proceed in parallel on distinct waves.
__global__ __launch_bounds__(256) void vox_sums_long(int64_t n, const int32_t* __restrict__ run_id,
                                                     const int32_t* __restrict__ run_start,
                                                     const double* __restrict__ sp, double* __restrict__ mean,
                                                     int32_t* __restrict__ count) {
  const int64_t runs = run_id[n - 1];
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < runs; r += waves) {
    const int32_t s = run_start[r], e = run_start[r + 1];
    if (e - s <= kVoxLaneRun) continue;
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int32_t c = s; c < e; c += 64) {
      const int64_t k = (int64_t)c + lane;
      double x = 0.0, y = 0.0, z = 0.0;
      if (k < e) {
        x = sp[3 * k];
        y = sp[3 * k + 1];
        z = sp[3 * k + 2];
      }
      if (e - c >= 64) {
#pragma unroll
        for (int t = 0; t < 64; ++t) {
          ax += vox_readlane(x, t);
          ay += vox_readlane(y, t);
          az += vox_readlane(z, t);
        }
      } else {
        for (int t = 0; t < e - c; ++t) {
          ax += vox_readlane(x, t);
          ay += vox_readlane(y, t);
          az += vox_readlane(z, t);
        }
      }
    }
    if (lane == 0) {
      const double cnt = (double)(e - s);
      mean[3 * r] = ax / cnt;
      mean[3 * r + 1] = ay / cnt;
      mean[3 * r + 2] = az / cnt;
      count[r] = e - s;
    }
  }
}

__global__ __launch_bounds__(kVoxBlock) void vox_trace(const VoxDesc* __restrict__ desc,
                                                       const int32_t* __restrict__ blk_prob,
                                                       const int32_t* __restrict__ perm,
                                                       const int32_t* __restrict__ run_id,
                                                       const int32_t* __restrict__ summary,
                                                       int32_t* __restrict__ trace) {
  const int b = blk_prob[blockIdx.x];
  const VoxDesc d = desc[b];
  const int64_t local = (int64_t)(blockIdx.x - d.blk_off) * kVoxBlock + threadIdx.x;
  if (local >= d.n) return;
  const int64_t j = d.off + local;  // sorted position: a problem keeps its range through the sort
  trace[perm[j]] = run_id[j] - 1 - summary[2 * b];
}

inline unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

size_t voxel_sort_temp_bytes(int64_t n) {
  size_t sort_bytes = 0, scan_bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                  (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)n, 0, 64, (hipStream_t)0);
  (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)n,
                                rocprim::plus<int32_t>(), (hipStream_t)0);
  return sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
}

void launch_voxel_keys(hipStream_t s, const VoxDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                       const double* d_pts, int prob_shift, uint64_t* d_key_lo, uint64_t* d_key_hi, int32_t* d_iota) {
  if (n_blk > 0)
    vox_keys<<<n_blk, kVoxBlock, 0, s>>>(d_desc, d_blk_prob, d_pts, prob_shift, d_key_lo, d_key_hi, d_iota);
}

hipError_t launch_voxel_sort(hipStream_t s, void* d_temp, size_t temp_bytes, int64_t n, int bits,
                             const uint64_t* d_key_lo, const uint64_t* d_key_hi, const int32_t* d_iota,
                             uint64_t* d_sorted, uint64_t* d_gathered, int32_t* d_perm1, int32_t* d_perm) {
  size_t tb = temp_bytes;
  if (bits <= 64)
    return rocprim::radix_sort_pairs(d_temp, tb, d_key_lo, d_sorted, d_iota, d_perm, (size_t)n, 0, (unsigned)bits,
                                     s);
  hipError_t e = rocprim::radix_sort_pairs(d_temp, tb, d_key_lo, d_sorted, d_iota, d_perm1, (size_t)n, 0, 64, s);
  if (e != hipSuccess) return e;
  vox_gather_hi<<<blocks(n, 256), 256, 0, s>>>(n, d_key_hi, d_perm1, d_gathered);
  tb = temp_bytes;
  return rocprim::radix_sort_pairs(d_temp, tb, (const uint64_t*)d_gathered, d_sorted, (const int32_t*)d_perm1, d_perm,
                                   (size_t)n, 0, (unsigned)(bits - 64), s);
}

hipError_t launch_voxel_runs(hipStream_t s, void* d_temp, size_t temp_bytes, int64_t n, bool two_words,
                             const double* d_pts, const uint64_t* d_key_lo, const uint64_t* d_key_hi,
                             const int32_t* d_perm, double* d_sorted_pts, int32_t* d_head, int32_t* d_run_id,
                             int32_t* d_run_start) {
  vox_heads<<<blocks(n, 256), 256, 0, s>>>(n, two_words ? 1 : 0, d_pts, d_key_lo, d_key_hi, d_perm, d_sorted_pts,
                                           d_head);
  size_t tb = temp_bytes;
  hipError_t e = rocprim::inclusive_scan(d_temp, tb, (const int32_t*)d_head, d_run_id, (size_t)n,
                                         rocprim::plus<int32_t>(), s);
  if (e != hipSuccess) return e;
  vox_starts<<<blocks(n, 256), 256, 0, s>>>(n, d_head, d_run_id, d_run_start);
  return hipGetLastError();
}

void launch_voxel_reduce(hipStream_t s, const VoxDesc* d_desc, int batch, int64_t n, const int32_t* d_run_id,
                         const int32_t* d_run_start, const double* d_sorted_pts, int32_t* d_summary, double* d_mean,
                         int32_t* d_count) {
  vox_summary<<<blocks(batch, 256), 256, 0, s>>>(d_desc, batch, d_run_id, d_summary);
  vox_sums_short<<<blocks(n, 256), 256, 0, s>>>(n, d_run_id, d_run_start, d_sorted_pts, d_mean, d_count);
  const unsigned long_blocks = blocks(n, 4) < kVoxLongBlocks ? blocks(n, 4) : kVoxLongBlocks;
  vox_sums_long<<<long_blocks, 256, 0, s>>>(n, d_run_id, d_run_start, d_sorted_pts, d_mean, d_count);
}

void launch_voxel_trace(hipStream_t s, const VoxDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                        const int32_t* d_perm, const int32_t* d_run_id, const int32_t* d_summary, int32_t* d_trace) {
  if (n_blk > 0) vox_trace<<<n_blk, kVoxBlock, 0, s>>>(d_desc, d_blk_prob, d_perm, d_run_id, d_summary, d_trace);
}

}  // namespace thip
