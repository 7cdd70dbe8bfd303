// kernels_rgbd.hip -- depth frames to clouds and clouds to depth frames for gfx950 (include/teaser_hip.h, "Depth frames";
// device code: icp_rgbd_device.h; host side: icp_rgbd.hip; design, bytes moved and the resource report: DESIGN.md
// section 31).
//
// Unprojection.  The visited pixels of every frame are cut into tiles of kRgbdTile in visiting order; a block of four
// waves serves one tile, a launch all tiles of all frames.  count: the rows a tile emits (the valid pixels, or with
// valid_only = 0 all of them), by a ballot and a population count per wave.  scan: one block per frame, the exclusive
// sum of its tiles' counts and the frame's count.  write: the depth is read again, a lane's row is the tile's start plus
// the rows of the waves in front of it plus the set bits of its own wave's ballot below it -- never an atomic cursor,
// so the rows stand in visiting order.  The 24-byte rows are stored as they are, three doubles per lane: the lanes of a
// wave cover one contiguous stretch of 1.5 KB, which the L2 merges; no LDS staging.
//
// Projection.  scatter: one thread per point, a 64-bit unsigned atomic minimum of (bits(d) << 32) | k on the pixel's key.
// resolve: one thread per pixel decodes the key, gathers the colour and adds the block's hits to the frame's counter (an
// int32 sum: any order gives the same number).
#include "icp_internal.h"
#include "icp_rgbd_device.h"

namespace thip {

// The pixel this thread visits: false behind the frame's last one.  *zf its depth, (*i, *j) its coordinates, *ri its
// row among the packed visited rows.
__device__ __forceinline__ bool rgbd_visit(const IcpFrameDesc& f, const unsigned char* __restrict__ in, int tile,
                                           int* i, int* j, int* ri, float* zf) {
  const int v = tile * kRgbdTile + (int)threadIdx.x;
  if (v >= f.n_vis) return false;
  *ri = v / f.nj;
  *i = *ri * f.stride;
  *j = (v - *ri * f.nj) * f.stride;
  const unsigned char* row = in + f.depth_off + (int64_t)*ri * f.width * rgbd_depth_bytes(f.depth_format);
  *zf = rgbd_depth(f, row, *j);
  return true;
}

__global__ __launch_bounds__(kRgbdTile) void rgbd_count_kernel(const IcpFrameDesc* __restrict__ frames,
                                                               const int32_t* __restrict__ tile_frame,
                                                               const unsigned char* __restrict__ in,
                                                               int32_t* __restrict__ tile_count) {
  __shared__ int32_t wave_rows[kRgbdTile / 64];
  const IcpFrameDesc& f = frames[tile_frame[blockIdx.x]];
  int i, j, ri;
  float zf;
  const bool in_frame = rgbd_visit(f, in, (int)blockIdx.x - f.tile_off, &i, &j, &ri, &zf);
  const bool emit = in_frame && (f.valid_only == 0 || rgbd_valid(zf));
  const unsigned long long ballot = __ballot(emit);
  if (threadIdx.x % 64 == 0) wave_rows[threadIdx.x / 64] = __popcll(ballot);
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = (wave_rows[0] + wave_rows[1]) + (wave_rows[2] + wave_rows[3]);
}

// One block per frame: tile_start = the exclusive sum of the frame's tile counts, count[frame] = their sum.
__global__ __launch_bounds__(kIcpScanThreads) void rgbd_scan_kernel(const IcpFrameDesc* __restrict__ frames,
                                                                   const int32_t* __restrict__ tile_count,
                                                                   int32_t* __restrict__ tile_start,
                                                                   int32_t* __restrict__ count) {
  __shared__ int32_t s[kIcpScanThreads];
  const IcpFrameDesc& f = frames[blockIdx.x];
  const int n = f.n_tiles;
  const int chunk = (n + kIcpScanThreads - 1) / kIcpScanThreads;
  const int lo0 = (int)threadIdx.x * chunk;
  const int lo = lo0 < n ? lo0 : n, hi = lo + chunk < n ? lo + chunk : n;
  int32_t sum = 0;
  for (int k = lo; k < hi; ++k) sum += tile_count[f.tile_off + k];
  s[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < kIcpScanThreads; o <<= 1) {  // inclusive Hillis-Steele scan of the per-thread sums
    const int32_t add = threadIdx.x >= (unsigned)o ? s[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  int32_t run = s[threadIdx.x] - sum;
  for (int k = lo; k < hi; ++k) {
    tile_start[f.tile_off + k] = run;
    run += tile_count[f.tile_off + k];
  }
  if (threadIdx.x == kIcpScanThreads - 1) count[blockIdx.x] = s[threadIdx.x];
}

__global__ __launch_bounds__(kRgbdTile) void rgbd_write_kernel(const IcpFrameDesc* __restrict__ frames,
                                                               const int32_t* __restrict__ tile_frame,
                                                               const unsigned char* __restrict__ in,
                                                               const int32_t* __restrict__ tile_start,
                                                               double* __restrict__ points, double* __restrict__ colors,
                                                               int32_t* __restrict__ pixels) {
  __shared__ int32_t wave_rows[kRgbdTile / 64];
  const IcpFrameDesc& f = frames[tile_frame[blockIdx.x]];
  int i = 0, j = 0, ri = 0;
  float zf = 0.0f;
  const bool in_frame = rgbd_visit(f, in, (int)blockIdx.x - f.tile_off, &i, &j, &ri, &zf);
  const bool valid = in_frame && rgbd_valid(zf);
  const bool emit = in_frame && (f.valid_only == 0 || valid);
  const unsigned long long ballot = __ballot(emit);
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  if (lane == 0) wave_rows[wave] = __popcll(ballot);
  __syncthreads();
  if (!emit) return;
  int rank = tile_start[blockIdx.x] + __popcll(ballot & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) rank += wave_rows[w];
  double p[3];
  if (valid) {
    rgbd_point(f, i, j, zf, p);
  } else {
    p[0] = p[1] = p[2] = __builtin_nan("");
  }
  double* out = points + 3 * (f.point_off + rank);
  out[0] = p[0], out[1] = p[1], out[2] = p[2];
  if (f.color_out >= 0) {
    double c[3];
    rgbd_color(f, in + f.color_off + (int64_t)ri * f.width * rgbd_color_bytes(f.color_format), j, c);
    double* co = colors + 3 * (f.color_out + rank);
    co[0] = c[0], co[1] = c[1], co[2] = c[2];
  }
  if (f.pixel_out >= 0) pixels[f.pixel_out + rank] = i * f.width + j;
}

void launch_icp_rgbd_unproject(hipStream_t s, const IcpFrameDesc* d_frames, const int32_t* d_tile_frame, int n_tiles,
                               int batch, const unsigned char* d_in, int32_t* d_tile_count, int32_t* d_tile_start,
                               int32_t* d_count, double* d_points, double* d_colors, int32_t* d_pixels) {
  if (n_tiles > 0)
    hipLaunchKernelGGL(rgbd_count_kernel, dim3(n_tiles), dim3(kRgbdTile), 0, s, d_frames, d_tile_frame, d_in,
                       d_tile_count);
  hipLaunchKernelGGL(rgbd_scan_kernel, dim3(batch), dim3(kIcpScanThreads), 0, s, d_frames, d_tile_count, d_tile_start,
                     d_count);
  if (n_tiles > 0)
    hipLaunchKernelGGL(rgbd_write_kernel, dim3(n_tiles), dim3(kRgbdTile), 0, s, d_frames, d_tile_frame, d_in,
                       d_tile_start, d_points, d_colors, d_pixels);
}

__global__ __launch_bounds__(kRgbdTile) void rgbd_scatter_kernel(const IcpProjDesc* __restrict__ descs,
                                                                 const int32_t* __restrict__ blk_prob,
                                                                 const double* __restrict__ points,
                                                                 unsigned long long* __restrict__ keys) {
  const IcpProjDesc& d = descs[blk_prob[blockIdx.x]];
  const int k = ((int)blockIdx.x - d.blk_off) * kRgbdTile + (int)threadIdx.x;
  if (k >= d.n) return;
  const double* xp = points + 3 * (d.p_off + k);
  const double X[3] = {xp[0], xp[1], xp[2]};
  int32_t pixel;
  uint64_t key;
  if (rgbd_project(d, X, k, &pixel, &key)) atomicMin(keys + d.img_off + pixel, (unsigned long long)key);
}

__global__ __launch_bounds__(kRgbdTile) void rgbd_resolve_kernel(
    const IcpProjDesc* __restrict__ descs, const int32_t* __restrict__ tile_prob,
    const unsigned long long* __restrict__ keys, const double* __restrict__ colors, float* __restrict__ depth,
    float* __restrict__ color_img, int32_t* __restrict__ index_img, int32_t* __restrict__ n_hit) {
  __shared__ int32_t wave_hits[kRgbdTile / 64];
  const int b = tile_prob[blockIdx.x];
  const IcpProjDesc& d = descs[b];
  const int64_t px = (int64_t)((int)blockIdx.x - d.tile_off) * kRgbdTile + threadIdx.x;
  const bool in_image = px < (int64_t)d.width * d.height;
  bool hit = false;
  if (in_image) {
    float z;
    int32_t k;
    hit = rgbd_resolve(keys[d.img_off + px], &z, &k);
    depth[d.img_off + px] = z;
    if (d.index_out >= 0) index_img[d.index_out + px] = k;
    if (d.color_out >= 0) {
      float* c = color_img + 3 * (d.color_out + px);
      const double* src = colors + 3 * (d.p_off + (hit ? k : 0));
      for (int t = 0; t < 3; ++t) c[t] = hit ? (float)src[t] : 0.0f;
    }
  }
  // the block's hits in one add: the waves' counts meet in LDS
  const unsigned long long ballot = __ballot(hit);
  if (threadIdx.x % 64 == 0) wave_hits[threadIdx.x / 64] = (int32_t)__popcll(ballot);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int32_t hits = (wave_hits[0] + wave_hits[1]) + (wave_hits[2] + wave_hits[3]);
    if (hits) atomicAdd(n_hit + b, hits);
  }
}

void launch_icp_rgbd_project(hipStream_t s, const IcpProjDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                             const int32_t* d_tile_prob, int n_tiles, const double* d_points, const double* d_colors,
                             uint64_t* d_keys, float* d_depth, float* d_color_img, int32_t* d_index_img,
                             int32_t* d_n_hit) {
  if (n_blk > 0)
    hipLaunchKernelGGL(rgbd_scatter_kernel, dim3(n_blk), dim3(kRgbdTile), 0, s, d_desc, d_blk_prob, d_points,
                       (unsigned long long*)d_keys);
  if (n_tiles > 0)
    hipLaunchKernelGGL(rgbd_resolve_kernel, dim3(n_tiles), dim3(kRgbdTile), 0, s, d_desc, d_tile_prob,
                       (const unsigned long long*)d_keys, d_colors, d_depth, d_color_img, d_index_img, d_n_hit);
}

}  // namespace thip
