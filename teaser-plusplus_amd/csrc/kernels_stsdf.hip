// kernels_stsdf.hip -- the scalable TSDF volume for gfx950 (include/teaser_hip.h, "Scalable TSDF volume"; device code:
// stsdf_device.h and, for the voxels of a block, tsdf_device.h; host side: stsdf.hip; design, bytes moved and the
// resource report: DESIGN.md section 37).
//
// Touch.  One thread per (frame, sampled pixel): the FP64 unprojection of "Depth frames" and ONE candidate -- the lowest
// block the point touches, with the extent of its box (at most 4 blocks an axis) and the frame beside it.  Two stable
// passes of rocprim's radix sort, by value and then by key, bring equal candidates together; a head flag, a scan and a
// compaction leave the distinct ones.  The host reads those back, expands the boxes and merges the directory.
//
// Integration.  One workgroup per (touched block, pass of kTsdfChunk frames); its 256 threads are the block's columns
// in the [z][x][y] layout and walk 16 z steps with the dense volume's functions and the block's own origin.  The frame
// mask of an item is wave-uniform: a frame that does not touch the block costs a scalar branch.
//
// Extraction.  count: a workgroup per block counts the rows of its columns and sums them; the dense scan runs over the
// blocks; write: a workgroup scans its columns in LDS and writes from the block's offset.  The order falls out of the
// directory order: no sort and no atomic cursor.  The only atomic of the file is the integer add of the touch pass.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "stsdf_device.h"

namespace thip {

__global__ __launch_bounds__(kRgbdTile) void stsdf_touch_kernel(const IcpFrameDesc* __restrict__ frames,
                                                                const unsigned char* __restrict__ in, const double trunc,
                                                                const double ul, uint64_t* __restrict__ keys,
                                                                uint32_t* __restrict__ vals,
                                                                unsigned long long* __restrict__ oor) {
  const IcpFrameDesc& f = frames[blockIdx.y];
  const int t = (int)(blockIdx.x * kRgbdTile + threadIdx.x);
  if (t >= f.n_vis) return;
  uint64_t key = kStsdfNoKey;
  uint32_t ext = 0;
  bool clipped;
  if (!stsdf_touch_pixel(f, in, t, trunc, ul, &key, &ext, &clipped)) key = kStsdfNoKey;
  keys[f.point_off + t] = key;
  vals[f.point_off + t] = ((uint32_t)blockIdx.y << 6) | ext;
  if (clipped) atomicAdd(oor, 1ull);
}

void launch_stsdf_touch(hipStream_t s, const IcpFrameDesc* d_frames, int n_frames, int max_vis, const unsigned char* d_in,
                        double trunc, double ul, uint64_t* d_keys, uint32_t* d_vals, unsigned long long* d_oor) {
  if (n_frames < 1 || max_vis < 1) return;
  hipLaunchKernelGGL(stsdf_touch_kernel, dim3((unsigned)((max_vis + kRgbdTile - 1) / kRgbdTile), (unsigned)n_frames),
                     dim3(kRgbdTile), 0, s, d_frames, d_in, trunc, ul, d_keys, d_vals, d_oor);
}

__global__ __launch_bounds__(256) void stsdf_head_kernel(const int64_t n, const uint64_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ vals, int32_t* __restrict__ head) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const uint64_t key = keys[k];
  head[k] = key != kStsdfNoKey && (k == 0 || keys[k - 1] != key || vals[k - 1] != vals[k]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void stsdf_compact_kernel(const int64_t n, const uint64_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ vals,
                                                            const int32_t* __restrict__ head,
                                                            const int32_t* __restrict__ pos, uint64_t* __restrict__ ukeys,
                                                            uint32_t* __restrict__ uvals, int32_t* __restrict__ count) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  if (head[k]) {
    ukeys[pos[k] - 1] = keys[k];
    uvals[pos[k] - 1] = vals[k];
  }
  if (k == n - 1) *count = pos[k];
}

size_t stsdf_unique_temp_bytes(int64_t n) {
  size_t by_val = 0, by_key = 0, scan_bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, by_val, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint64_t*)nullptr,
                                  (uint64_t*)nullptr, (size_t)n, 0, 32, (hipStream_t)0);
  (void)rocprim::radix_sort_pairs(nullptr, by_key, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (size_t)n, 0, 64, (hipStream_t)0);
  (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)n,
                                rocprim::plus<int32_t>(), (hipStream_t)0);
  return std::max(std::max(by_val, by_key), scan_bytes);
}

// Two stable passes, by value and then by key, leave the pairs in (key, value) order in d_keys / d_vals again.
hipError_t launch_stsdf_unique(hipStream_t s, int64_t n, void* d_temp, size_t temp_bytes, uint64_t* d_keys, uint32_t* d_vals,
                               uint64_t* d_tmp_keys, uint32_t* d_tmp_vals, int32_t* d_head, int32_t* d_pos,
                               uint64_t* d_ukeys, uint32_t* d_uvals, int32_t* d_count) {
  size_t tb = temp_bytes;
  hipError_t e = rocprim::radix_sort_pairs(d_temp, tb, (const uint32_t*)d_vals, d_tmp_vals, (const uint64_t*)d_keys, d_tmp_keys,
                                           (size_t)n, 0, 32, s);
  if (e != hipSuccess) return e;
  tb = temp_bytes;
  e = rocprim::radix_sort_pairs(d_temp, tb, (const uint64_t*)d_tmp_keys, d_keys, (const uint32_t*)d_tmp_vals, d_vals, (size_t)n,
                                0, 64, s);
  if (e != hipSuccess) return e;
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(stsdf_head_kernel, dim3(blocks), dim3(256), 0, s, n, d_keys, d_vals, d_head);
  tb = temp_bytes;
  e = rocprim::inclusive_scan(d_temp, tb, (const int32_t*)d_head, d_pos, (size_t)n, rocprim::plus<int32_t>(), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(stsdf_compact_kernel, dim3(blocks), dim3(256), 0, s, n, d_keys, d_vals, d_head, d_pos, d_ukeys, d_uvals,
                     d_count);
  return hipGetLastError();
}

__global__ __launch_bounds__(kStsdfCols) void stsdf_integrate_kernel(const TsdfGrid g0, const double ul,
                                                                     const TsdfChunkArgs ck,
                                                                     const unsigned char* __restrict__ in,
                                                                     const StsdfItem* __restrict__ items) {
  const StsdfItem item = items[blockIdx.x];
  const uint32_t mask = __builtin_amdgcn_readfirstlane(item.mask);
  int b[3];
  stsdf_unkey(item.key, b);
  const TsdfGrid g = stsdf_block_grid(g0, ul, b);
  const TsdfFields v = stsdf_fields(item.base, g.color_type);
  const int col = (int)threadIdx.x;
  const int x = col / kStsdfU, y = col - x * kStsdfU;
  float c[kTsdfChunk][3];
#pragma unroll
  for (int k = 0; k < kTsdfChunk; ++k)
    if ((mask >> k) & 1u) tsdf_column_start(g, ck.f[k], x, y, c[k]);
  for (int z = 0; z < kStsdfU; ++z) {
    const int64_t at = (int64_t)z * kStsdfCols + col;
    bool loaded = false;
    float tv = 0.0f, wv = 0.0f;
    double cv[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kTsdfChunk; ++k)
      if ((mask >> k) & 1u) {
        float t;
        double s[3] = {0.0, 0.0, 0.0};
        if (tsdf_hit(g, ck.f[k], in, c[k], &t, s)) {
          if (!loaded) {
            loaded = true;
            tv = v.tsdf[at];
            wv = v.weight[at];
            if (g.color_type != 0)
              for (int q = 0; q < 3; ++q) cv[q] = v.color[q * v.n + at];
          }
          tsdf_update(g, t, s, &tv, &wv, cv);
        }
        tsdf_column_step(ck.f[k], c[k]);
      }
    if (loaded) {
      v.tsdf[at] = tv;
      v.weight[at] = wv;
      if (g.color_type != 0)
        for (int q = 0; q < 3; ++q) v.color[q * v.n + at] = cv[q];
    }
  }
}

void launch_stsdf_integrate(hipStream_t s, const TsdfGrid& g0, double ul, const TsdfChunkArgs& ck, const unsigned char* d_in,
                            const StsdfItem* d_items, int n_items) {
  if (n_items < 1) return;
  hipLaunchKernelGGL(stsdf_integrate_kernel, dim3((unsigned)n_items), dim3(kStsdfCols), 0, s, g0, ul, ck, d_in, d_items);
}

__global__ __launch_bounds__(kStsdfCols) void stsdf_count_kernel(const TsdfGrid g0, const StsdfDir d, const int mode,
                                                                 int32_t* __restrict__ counts,
                                                                 int32_t* __restrict__ totals) {
  __shared__ int32_t sum[kStsdfCols];
  const int e = (int)blockIdx.x, col = (int)threadIdx.x;
  const int x = col / kStsdfU, y = col - x * kStsdfU;
  char* up[3];
  stsdf_up_blocks(d, e, up);
  const TsdfFields v = stsdf_fields(d.base[e], g0.color_type);
  int32_t rows = 0;
  for (int z = 0; z < kStsdfU; ++z) rows += stsdf_voxel_rows(g0, v, up, mode, x, y, z);
  counts[(int64_t)e * kStsdfCols + col] = rows;
  sum[col] = rows;
  __syncthreads();
  for (int o = kStsdfCols / 2; o > 0; o >>= 1) {
    if (col < o) sum[col] += sum[col + o];
    __syncthreads();
  }
  if (col == 0) totals[e] = sum[0];
}

void launch_stsdf_count(hipStream_t s, const TsdfGrid& g0, const StsdfDir& d, int mode, int32_t* d_counts,
                        int32_t* d_totals, int64_t* d_offsets) {
  if (d.n > 0) hipLaunchKernelGGL(stsdf_count_kernel, dim3((unsigned)d.n), dim3(kStsdfCols), 0, s, g0, d, mode, d_counts, d_totals);
  launch_tsdf_scan(s, d_totals, d.n, d_offsets);
}

__global__ __launch_bounds__(kStsdfCols) void stsdf_write_kernel(const TsdfGrid g0, const double ul, const StsdfDir d,
                                                                 const int mode, const int32_t* __restrict__ counts,
                                                                 const int64_t* __restrict__ offsets,
                                                                 const int64_t capacity, double* __restrict__ points,
                                                                 double* __restrict__ normals,
                                                                 double* __restrict__ colors) {
  __shared__ int32_t run[kStsdfCols];
  const int e = (int)blockIdx.x, col = (int)threadIdx.x;
  if (offsets[d.n] > capacity || offsets[e + 1] == offsets[e]) return;  // the same for every thread of the block
  const int32_t mine = counts[(int64_t)e * kStsdfCols + col];
  run[col] = mine;
  __syncthreads();
  for (int o = 1; o < kStsdfCols; o <<= 1) {  // inclusive Hillis-Steele scan of the columns' rows
    const int32_t add = col >= o ? run[col - o] : 0;
    __syncthreads();
    run[col] += add;
    __syncthreads();
  }
  if (mine == 0) return;
  char* up[3];
  stsdf_up_blocks(d, e, up);
  const int x = col / kStsdfU, y = col - x * kStsdfU;
  stsdf_write_column(g0, ul, d, e, up, mode, x, y, offsets[e] + (run[col] - mine), points, normals, colors);
}

void launch_stsdf_write(hipStream_t s, const TsdfGrid& g0, double ul, const StsdfDir& d, int mode, const int32_t* d_counts,
                        const int64_t* d_offsets, int64_t capacity, double* d_points, double* d_normals, double* d_colors) {
  if (d.n < 1) return;
  hipLaunchKernelGGL(stsdf_write_kernel, dim3((unsigned)d.n), dim3(kStsdfCols), 0, s, g0, ul, d, mode, d_counts, d_offsets,
                     capacity, d_points, d_normals, d_colors);
}

// A block per workgroup, a column per thread, walking z: as the dense export and import.
__global__ __launch_bounds__(kStsdfCols) void stsdf_export_kernel(const int color_type, char* const* __restrict__ base,
                                                                  float* __restrict__ tw, double* __restrict__ color) {
  const TsdfFields v = stsdf_fields(base[blockIdx.x], color_type);
  const int col = (int)threadIdx.x;
  for (int z = 0; z < kStsdfU; ++z) {
    const int64_t at = (int64_t)z * kStsdfCols + col, o = (int64_t)blockIdx.x * kStsdfVoxels + col * kStsdfU + z;
    if (tw) {
      tw[2 * o] = v.tsdf[at];
      tw[2 * o + 1] = v.weight[at];
    }
    if (color)
      for (int k = 0; k < 3; ++k) color[3 * o + k] = v.color[k * v.n + at];
  }
}

__global__ __launch_bounds__(kStsdfCols) void stsdf_import_kernel(const int color_type, char* const* __restrict__ base,
                                                                  const float* __restrict__ tw,
                                                                  const double* __restrict__ color) {
  const TsdfFields v = stsdf_fields(base[blockIdx.x], color_type);
  const int col = (int)threadIdx.x;
  for (int z = 0; z < kStsdfU; ++z) {
    const int64_t at = (int64_t)z * kStsdfCols + col, o = (int64_t)blockIdx.x * kStsdfVoxels + col * kStsdfU + z;
    if (tw) {
      v.tsdf[at] = tw[2 * o];
      v.weight[at] = tw[2 * o + 1];
    }
    if (color)
      for (int k = 0; k < 3; ++k) v.color[k * v.n + at] = rgbd_canonical(color[3 * o + k]);
  }
}

void launch_stsdf_export(hipStream_t s, int color_type, char* const* d_base, int n, float* d_tw, double* d_color) {
  if (n < 1) return;
  hipLaunchKernelGGL(stsdf_export_kernel, dim3((unsigned)n), dim3(kStsdfCols), 0, s, color_type, d_base, d_tw, d_color);
}

void launch_stsdf_import(hipStream_t s, int color_type, char* const* d_base, int n, const float* d_tw, const double* d_color) {
  if (n < 1) return;
  hipLaunchKernelGGL(stsdf_import_kernel, dim3((unsigned)n), dim3(kStsdfCols), 0, s, color_type, d_base, d_tw, d_color);
}

}  // namespace thip
