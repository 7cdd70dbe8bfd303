// icp_rgbd_device.h -- the per-pixel and per-point rules of the depth-frame calls that do not depend on the launch shape
// (include/teaser_hip.h, "Depth frames"; kernels: kernels_rgbd.hip, host side: icp_rgbd.hip, design: DESIGN.md section
// 31): the depth sample of a pixel as float32, its point and colour, the pixel and key of a projected point, and what a
// key decodes to.  Nothing here uses a wave operation or LDS, so tests/rgbd_host_driver.cpp runs this very source in
// serial loops.
//
// The library is compiled with -ffp-contract=off: no product-add is fused, and every sum is written out left to right.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace thip {

constexpr int kRgbdTile = 256;            // visited pixels (unprojection) or pixels (projection) of a block: four waves
constexpr int kRgbdMaxSide = 16384;       // the largest width and height
constexpr uint64_t kRgbdEmptyKey = ~0ull; // a pixel no point has landed on

// One frame of an unprojection call (host-built, read-only on the device).  The visited rows of the frame (i = 0, stride,
// ...) lie packed in the input buffer, one after the other without padding; so do the rows of its colour image.
struct IcpFrameDesc {
  int32_t width, height, stride;
  int32_t depth_format, color_format, intensity, valid_only;
  int32_t nj;           // visited pixels per visited row: ceil(width / stride)
  int32_t n_vis;        // visited pixels: ceil(height / stride) nj
  int32_t tile_off;     // first tile of the frame; it has ceil(n_vis / kRgbdTile)
  int32_t n_tiles;
  int32_t pad;
  int64_t depth_off;    // byte offsets into the input buffer
  int64_t color_off;
  int64_t point_off;    // first row of the frame in the packed points; the frame has room for n_vis rows
  int64_t color_out;    // first row in the packed colours, -1: not asked for
  int64_t pixel_out;    // first row in the packed pixel indices, -1: not asked for
  double fx, fy, cx, cy;
  double pose[12];      // rows 0 .. 2 of camera_pose
  double depth_trunc;
  float depth_scale;    // (float)depth_scale
  float pad2;
};

// One problem of a projection call.
struct IcpProjDesc {
  int32_t width, height;
  int32_t n;            // points
  int32_t has_color;
  int32_t blk_off;      // first scatter block (kRgbdTile points each)
  int32_t tile_off;     // first resolve block (kRgbdTile pixels each)
  int64_t p_off;        // first point in the packed points (and colours)
  int64_t img_off;      // first pixel in the key image and the packed depth image
  int64_t color_out;    // first pixel in the packed colour image, -1: not asked for
  int64_t index_out;    // first pixel in the packed index image, -1: not asked for
  double fx, fy, cx, cy;
  double ext[12];       // rows 0 .. 2 of extrinsic
  double depth_scale, depth_max;
};

__host__ __device__ __forceinline__ int rgbd_depth_bytes(int format) { return format == 0 ? 2 : 4; }
__host__ __device__ __forceinline__ int rgbd_color_bytes(int format) { return format == 1 ? 3 : (format == 2 ? 4 : 12); }

// A NaN is stored as THE quiet NaN (sign and payload of an arithmetic NaN differ between machines).
__host__ __device__ __forceinline__ double rgbd_canonical(double x) { return x != x ? __builtin_nan("") : x; }

__host__ __device__ __forceinline__ float rgbd_load_f32(const unsigned char* p) {
  float v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// The depth of pixel j of a packed row as float32; 0 where truncated.
__host__ __device__ __forceinline__ float rgbd_depth(const IcpFrameDesc& f, const unsigned char* row, int j) {
  if (f.depth_format == 0) {
    uint16_t d;
    __builtin_memcpy(&d, row + 2 * (int64_t)j, 2);
    float zf = (float)d / f.depth_scale;
    if ((double)zf >= f.depth_trunc) zf = 0.0f;
    return zf;
  }
  return rgbd_load_f32(row + 4 * (int64_t)j);
}

__host__ __device__ __forceinline__ bool rgbd_valid(float zf) { return zf > 0.0f; }

// The point of pixel (i, j) with the valid depth zf.
__host__ __device__ __forceinline__ void rgbd_point(const IcpFrameDesc& f, int i, int j, float zf, double* p) {
  const double z = (double)zf;
  const double x = (((double)j - f.cx) * z) / f.fx;
  const double y = (((double)i - f.cy) * z) / f.fy;
  for (int r = 0; r < 3; ++r) {
    const double* m = f.pose + 4 * r;
    p[r] = rgbd_canonical(((m[0] * x + m[1] * y) + m[2] * z) + m[3]);
  }
}

// The colour of pixel j of a packed colour row.
__host__ __device__ __forceinline__ void rgbd_color(const IcpFrameDesc& f, const unsigned char* row, int j, double* c) {
  if (f.color_format == 1) {
    const unsigned char* px = row + 3 * (int64_t)j;
    if (f.intensity) {
      const float v = ((0.2990f * (float)px[0] + 0.5870f * (float)px[1]) + 0.1140f * (float)px[2]) / 255.0f;
      c[0] = c[1] = c[2] = (double)v;
    } else {
      for (int k = 0; k < 3; ++k) c[k] = (double)px[k] / 255.0;
    }
  } else if (f.color_format == 2) {
    c[0] = c[1] = c[2] = rgbd_canonical((double)rgbd_load_f32(row + 4 * (int64_t)j));
  } else {
    for (int k = 0; k < 3; ++k) c[k] = rgbd_canonical((double)rgbd_load_f32(row + 12 * (int64_t)j + 4 * k));
  }
}

__host__ __device__ __forceinline__ bool rgbd_finite(double x) { return __builtin_fabs(x) <= 1.7976931348623157e308; }

// Point k (X) of a projection problem: false when it is skipped, else its pixel vi width + ui and its key
// (bits(d) << 32) | k.  d is not negative, so the keys of a pixel order as (d, k).
__host__ __device__ __forceinline__ bool rgbd_project(const IcpProjDesc& d, const double* X, int32_t k, int32_t* pixel,
                                                      uint64_t* key) {
  double c[3];
  for (int r = 0; r < 3; ++r) {
    const double* e = d.ext + 4 * r;
    c[r] = ((e[0] * X[0] + e[1] * X[1]) + e[2] * X[2]) + e[3];
  }
  const double zc = c[2];
  if (!(zc > 0.0) || !(zc <= d.depth_max)) return false;
  const double u = (d.fx * c[0]) / zc + d.cx, v = (d.fy * c[1]) / zc + d.cy;
  if (!rgbd_finite(u) || !rgbd_finite(v)) return false;
  if (!(__builtin_fabs(u) < 2147483648.0) || !(__builtin_fabs(v) < 2147483648.0)) return false;
  const double ur = __builtin_round(u), vr = __builtin_round(v);  // halves away from zero
  if (!(ur >= 0.0 && ur < (double)d.width) || !(vr >= 0.0 && vr < (double)d.height)) return false;
  const float depth = (float)(zc * d.depth_scale);
  if (!(__builtin_fabsf(depth) <= 3.4028234663852886e38f)) return false;
  uint32_t bits;
  __builtin_memcpy(&bits, &depth, 4);
  *pixel = (int32_t)vr * d.width + (int32_t)ur;
  *key = ((uint64_t)bits << 32) | (uint32_t)k;
  return true;
}

// What a pixel's key decodes to; false: the pixel is empty (depth 0, index -1).
__host__ __device__ __forceinline__ bool rgbd_resolve(uint64_t key, float* depth, int32_t* index) {
  if (key == kRgbdEmptyKey) {
    *depth = 0.0f;
    *index = -1;
    return false;
  }
  const uint32_t bits = (uint32_t)(key >> 32);
  __builtin_memcpy(depth, &bits, 4);
  *index = (int32_t)(uint32_t)key;
  return true;
}

}  // namespace thip
