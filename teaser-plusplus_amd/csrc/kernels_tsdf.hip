// kernels_tsdf.hip -- the TSDF volume for gfx950 (include/teaser_hip.h, "TSDF volume"; device code: tsdf_device.h; host
// side: tsdf.hip; design, bytes moved and the resource report: DESIGN.md section 32).
//
// Integration.  The camera point of a voxel is Open3D's running sum along z, which is serial, so a thread is a column
// (x, y) walking z.  The volume lies as [z][x][y] planes, one array per field: the lanes of a wave are consecutive
// columns and touch consecutive addresses at every step.  A pass applies up to kTsdfChunk frames, in order, to every
// voxel: the voxel is loaded when the first frame of the pass touches it and stored once, and only if touched.  The
// frame records are a kernel argument (scalar loads); the depth and colour images are read through the caches.  Where
// R R columns are too few to fill the chip a column is cut into z segments (blockIdx.y): a segment replays the additions
// in front of it -- three adds per frame and step, no memory -- and so arrives at the same bits.
//
// Extraction.  count: a column counts its rows.  scan: one block, the exclusive sum over the columns in (x, y) order.
// write: a column writes its rows from its offset walking z, the axes 0, 1, 2 inside a voxel.  That is Open3D's serial
// order with no sort and no atomic cursor.
#include "tsdf_device.h"

namespace thip {

__global__ __launch_bounds__(kTsdfBlock) void tsdf_integrate_kernel(const TsdfGrid g, const TsdfChunkArgs ck,
                                                                    const unsigned char* __restrict__ in,
                                                                    float* __restrict__ tsdf, float* __restrict__ weight,
                                                                    double* __restrict__ color) {
  const int64_t plane = (int64_t)g.R * g.R;
  const int64_t col = (int64_t)blockIdx.x * kTsdfBlock + threadIdx.x;
  if (col >= plane) return;
  const int x = (int)(col / g.R), y = (int)(col - (int64_t)x * g.R);
  const int seg_len = (g.R + ck.segments - 1) / ck.segments;
  const int z0 = (int)blockIdx.y * seg_len;
  const int z1 = z0 + seg_len < g.R ? z0 + seg_len : g.R;
  const int64_t n = plane * g.R;
  float c[kTsdfChunk][3];
#pragma unroll
  for (int k = 0; k < kTsdfChunk; ++k)
    if (k < ck.n) tsdf_column_start(g, ck.f[k], x, y, c[k]);
  for (int z = 0; z < z0; ++z) {  // the additions of the segments in front
#pragma unroll
    for (int k = 0; k < kTsdfChunk; ++k)
      if (k < ck.n) tsdf_column_step(ck.f[k], c[k]);
  }
  for (int z = z0; z < z1; ++z) {
    const int64_t at = (int64_t)z * plane + col;
    bool loaded = false;
    float tv = 0.0f, wv = 0.0f;
    double cv[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kTsdfChunk; ++k)
      if (k < ck.n) {
        float t;
        double s[3] = {0.0, 0.0, 0.0};
        if (tsdf_hit(g, ck.f[k], in, c[k], &t, s)) {
          if (!loaded) {
            loaded = true;
            tv = tsdf[at];
            wv = weight[at];
            if (g.color_type != 0)
              for (int q = 0; q < 3; ++q) cv[q] = color[q * n + at];
          }
          tsdf_update(g, t, s, &tv, &wv, cv);
        }
        tsdf_column_step(ck.f[k], c[k]);
      }
    if (loaded) {
      tsdf[at] = tv;
      weight[at] = wv;
      if (g.color_type != 0)
        for (int q = 0; q < 3; ++q) color[q * n + at] = cv[q];
    }
  }
}

void launch_tsdf_integrate(hipStream_t s, const TsdfGrid& g, const TsdfChunkArgs& ck, const unsigned char* d_in,
                           const TsdfFields& v) {
  const int64_t plane = (int64_t)g.R * g.R;
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((plane + kTsdfBlock - 1) / kTsdfBlock), (unsigned)ck.segments),
                     dim3(kTsdfBlock), 0, s, g, ck, d_in, v.tsdf, v.weight, v.color);
}

__global__ __launch_bounds__(kTsdfBlock) void tsdf_count_kernel(const TsdfGrid g, const TsdfFields v, const int mode,
                                                                int32_t* __restrict__ counts) {
  const int64_t col = (int64_t)blockIdx.x * kTsdfBlock + threadIdx.x;
  if (col >= (int64_t)g.R * g.R) return;
  const int x = (int)(col / g.R), y = (int)(col - (int64_t)x * g.R);
  int32_t rows = 0;
  for (int z = 0; z < g.R; ++z) rows += tsdf_voxel_rows(g, v, mode, x, y, z);
  counts[col] = rows;
}

// One block: offsets[c] = the rows of the columns in front of c, offsets[n_cols] = all rows.
__global__ __launch_bounds__(kTsdfScanThreads) void tsdf_scan_kernel(const int32_t* __restrict__ counts,
                                                                     const int64_t n_cols,
                                                                     int64_t* __restrict__ offsets) {
  __shared__ int64_t s[kTsdfScanThreads];
  const int64_t chunk = (n_cols + kTsdfScanThreads - 1) / kTsdfScanThreads;
  const int64_t lo0 = (int64_t)threadIdx.x * chunk;
  const int64_t lo = lo0 < n_cols ? lo0 : n_cols, hi = lo + chunk < n_cols ? lo + chunk : n_cols;
  int64_t sum = 0;
  for (int64_t k = lo; k < hi; ++k) sum += counts[k];
  s[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < kTsdfScanThreads; o <<= 1) {  // inclusive Hillis-Steele scan of the per-thread sums
    const int64_t add = threadIdx.x >= (unsigned)o ? s[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  int64_t run = s[threadIdx.x] - sum;
  for (int64_t k = lo; k < hi; ++k) {
    offsets[k] = run;
    run += counts[k];
  }
  if (threadIdx.x == kTsdfScanThreads - 1) offsets[n_cols] = s[threadIdx.x];
}

void launch_tsdf_scan(hipStream_t s, const int32_t* d_counts, int64_t n, int64_t* d_offsets) {
  hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(kTsdfScanThreads), 0, s, d_counts, n, d_offsets);
}

void launch_tsdf_count(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, int mode, int32_t* d_counts,
                       int64_t* d_offsets) {
  const int64_t plane = (int64_t)g.R * g.R;
  hipLaunchKernelGGL(tsdf_count_kernel, dim3((unsigned)((plane + kTsdfBlock - 1) / kTsdfBlock)), dim3(kTsdfBlock), 0, s, g,
                     v, mode, d_counts);
  launch_tsdf_scan(s, d_counts, plane, d_offsets);
}

__global__ __launch_bounds__(kTsdfBlock) void tsdf_write_kernel(const TsdfGrid g, const TsdfFields v, const int mode,
                                                                const int64_t* __restrict__ offsets,
                                                                const int64_t capacity, double* __restrict__ points,
                                                                double* __restrict__ normals,
                                                                double* __restrict__ colors) {
  const int64_t plane = (int64_t)g.R * g.R;
  const int64_t col = (int64_t)blockIdx.x * kTsdfBlock + threadIdx.x;
  if (col >= plane || offsets[plane] > capacity) return;
  const int64_t end = offsets[col + 1];
  int64_t row = offsets[col];
  if (row == end) return;
  const int x = (int)(col / g.R), y = (int)(col - (int64_t)x * g.R);
  for (int z = 0; z < g.R && row < end; ++z) {
    const int64_t at0 = tsdf_index(g.R, x, y, z);
    const float f0 = v.tsdf[at0];
    if (!tsdf_usable(v.weight[at0], f0)) continue;
    if (mode == 1) {
      tsdf_voxel_point(g, x, y, z, f0, points + 3 * row, colors ? colors + 3 * row : nullptr);
      ++row;
      continue;
    }
    for (int i = 0; i < 3; ++i) {
      int64_t at1;
      float f1;
      if (!tsdf_surface_row(g, v, x, y, z, i, f0, &at1, &f1)) continue;
      tsdf_surface_point(g, v, x, y, z, i, f0, at1, f1, points + 3 * row, normals ? normals + 3 * row : nullptr,
                         colors ? colors + 3 * row : nullptr);
      ++row;
    }
  }
}

void launch_tsdf_write(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, int mode, const int64_t* d_offsets,
                       int64_t capacity, double* d_points, double* d_normals, double* d_colors) {
  const int64_t plane = (int64_t)g.R * g.R;
  hipLaunchKernelGGL(tsdf_write_kernel, dim3((unsigned)((plane + kTsdfBlock - 1) / kTsdfBlock)), dim3(kTsdfBlock), 0, s, g,
                     v, mode, d_offsets, capacity, d_points, d_normals, d_colors);
}

// A column per thread, walking z: the reads (export) or writes (import) of the device layout are coalesced, the other
// side runs along a column's own stretch of Open3D's order.
__global__ __launch_bounds__(kTsdfBlock) void tsdf_export_kernel(const TsdfGrid g, const TsdfFields v,
                                                                 float* __restrict__ tw, double* __restrict__ color) {
  const int64_t col = (int64_t)blockIdx.x * kTsdfBlock + threadIdx.x;
  if (col >= (int64_t)g.R * g.R) return;
  const int x = (int)(col / g.R), y = (int)(col - (int64_t)x * g.R);
  for (int z = 0; z < g.R; ++z) {
    const int64_t at = tsdf_index(g.R, x, y, z), o = col * g.R + z;
    if (tw) {
      tw[2 * o] = v.tsdf[at];
      tw[2 * o + 1] = v.weight[at];
    }
    if (color)
      for (int k = 0; k < 3; ++k) color[3 * o + k] = v.color[k * v.n + at];
  }
}

__global__ __launch_bounds__(kTsdfBlock) void tsdf_import_kernel(const TsdfGrid g, const TsdfFields v,
                                                                 const float* __restrict__ tw,
                                                                 const double* __restrict__ color) {
  const int64_t col = (int64_t)blockIdx.x * kTsdfBlock + threadIdx.x;
  if (col >= (int64_t)g.R * g.R) return;
  const int x = (int)(col / g.R), y = (int)(col - (int64_t)x * g.R);
  for (int z = 0; z < g.R; ++z) {
    const int64_t at = tsdf_index(g.R, x, y, z), o = col * g.R + z;
    if (tw) {
      v.tsdf[at] = tw[2 * o];
      v.weight[at] = tw[2 * o + 1];
    }
    if (color)
      for (int k = 0; k < 3; ++k) v.color[k * v.n + at] = rgbd_canonical(color[3 * o + k]);
  }
}

void launch_tsdf_export(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, float* d_tw, double* d_color) {
  const int64_t plane = (int64_t)g.R * g.R;
  hipLaunchKernelGGL(tsdf_export_kernel, dim3((unsigned)((plane + kTsdfBlock - 1) / kTsdfBlock)), dim3(kTsdfBlock), 0, s,
                     g, v, d_tw, d_color);
}

void launch_tsdf_import(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, const float* d_tw, const double* d_color) {
  const int64_t plane = (int64_t)g.R * g.R;
  hipLaunchKernelGGL(tsdf_import_kernel, dim3((unsigned)((plane + kTsdfBlock - 1) / kTsdfBlock)), dim3(kTsdfBlock), 0, s,
                     g, v, d_tw, d_color);
}

}  // namespace thip
