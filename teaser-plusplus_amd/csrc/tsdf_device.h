// tsdf_device.h -- the per-voxel rules of the TSDF volume that do not depend on the launch shape (include/teaser_hip.h,
// "TSDF volume"; kernels: kernels_tsdf.hip, host side: tsdf.hip, design: DESIGN.md section 32): where a column of voxels
// starts in a camera, whether a frame touches a voxel and with what, the running averages, the surface rows of a voxel,
// an interpolated point with its colour and normal, and the device layout.  Nothing here uses a wave operation or LDS, so
// tests/tsdf_host_driver.cpp runs this very source in serial loops.
//
// The library is compiled with -ffp-contract=off: no product-add is fused, and every sum is written out left to right.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icp_rgbd_device.h"

namespace thip {

constexpr int kTsdfChunk = 8;           // frames one pass over the volume applies: 24 registers of running camera points
constexpr int kTsdfBlock = 256;         // threads of a block: four waves of consecutive columns
constexpr int kTsdfMaxR = 1024;         // the largest resolution
constexpr int kTsdfScanThreads = 1024;  // the one block of the column scan
constexpr int64_t kTsdfWaveTarget = 8192;  // waves the integration aims for: eight per SIMD of 256 CUs

// The volume as the kernels see it.  Device layout: voxel (x, y, z) lies at (z R + x) R + y of every field, so that the
// lanes of a wave (consecutive y, running on into the next x) touch consecutive addresses at every z.
struct TsdfGrid {
  int32_t R, color_type;
  float vl_f, half_f, trunc_f, inv_f;
  float org_f[3];
  float pad;
  double vl, half;
  double origin[3];
};

// One frame of an integration call (host-built).  The rows of its images lie packed in the input buffer.
struct TsdfFrame {
  float E[12];            // rows 0 .. 2 of the extrinsic, rounded to float32
  float s[3];             // E[r][2] vl_f: what one step along z adds to the camera point
  float fx, fy, cx, cy;
  float inv_fx, inv_fy;   // 1.0f / fx_f, 1.0f / fy_f
  float safe_w, safe_h;
  float depth_scale;      // (float)depth_scale
  int32_t width, height, depth_format;
  int32_t pad;
  int64_t depth_off;      // byte offsets into the input buffer
  int64_t color_off;
  double depth_trunc;
};

struct TsdfChunkArgs {  // a kernel argument: the records are read through scalar loads
  TsdfFrame f[kTsdfChunk];
  int32_t n;            // frames of this pass, 1 .. kTsdfChunk
  int32_t segments;     // z segments a column is cut into (a launch shape: no bit depends on it)
};

__host__ __device__ __forceinline__ int64_t tsdf_index(int R, int x, int y, int z) {
  return ((int64_t)z * R + x) * R + y;
}

// The camera point of voxel (x, y, 0) in frame f.
__host__ __device__ __forceinline__ void tsdf_column_start(const TsdfGrid& g, const TsdfFrame& f, int x, int y, float* c) {
  const float px = (g.half_f + g.vl_f * (float)x) + g.org_f[0];
  const float py = (g.half_f + g.vl_f * (float)y) + g.org_f[1];
  const float pz = g.half_f + g.org_f[2];
  for (int r = 0; r < 3; ++r) {
    const float* e = f.E + 4 * r;
    c[r] = ((e[0] * px + e[1] * py) + e[2] * pz) + e[3];
  }
}

// One step along z: Open3D's running sum, never a product.
__host__ __device__ __forceinline__ void tsdf_column_step(const TsdfFrame& f, float* c) {
  for (int r = 0; r < 3; ++r) c[r] = c[r] + f.s[r];
}

// The depth sample of pixel (v, u): the rule of "Depth frames".
__host__ __device__ __forceinline__ float tsdf_depth(const TsdfFrame& f, const unsigned char* in, int v, int u) {
  IcpFrameDesc d;  // the three fields rgbd_depth reads
  d.depth_format = f.depth_format;
  d.depth_scale = f.depth_scale;
  d.depth_trunc = f.depth_trunc;
  return rgbd_depth(d, in + f.depth_off + (int64_t)v * f.width * rgbd_depth_bytes(f.depth_format), u);
}

// Whether frame f updates the voxel whose camera point is c; then *t is the truncated distance and s the colour sample.
__host__ __device__ __forceinline__ bool tsdf_hit(const TsdfGrid& g, const TsdfFrame& f, const unsigned char* in,
                                                  const float* c, float* t, double* s) {
  if (!(c[2] > 0.0f)) return false;
  const float u_f = ((c[0] * f.fx) / c[2] + f.cx) + 0.5f;
  const float v_f = ((c[1] * f.fy) / c[2] + f.cy) + 0.5f;
  if (!(u_f >= 0.0001f && u_f < f.safe_w && v_f >= 0.0001f && v_f < f.safe_h)) return false;
  const int u = (int)u_f, v = (int)v_f;  // 0 <= u < width, 0 <= v < height by the test above
  const float d = tsdf_depth(f, in, v, u);
  if (!(d > 0.0f)) return false;
  const float xx = ((float)u - f.cx) * f.inv_fx, yy = ((float)v - f.cy) * f.inv_fy;
  const float m = __builtin_sqrtf((xx * xx + yy * yy) + 1.0f);
  const float sdf = (d - c[2]) * m;
  if (!(sdf > -g.trunc_f)) return false;
  const float q = sdf * g.inv_f;
  *t = q < 1.0f ? q : 1.0f;
  if (g.color_type == 1) {
    const unsigned char* px = in + f.color_off + 3 * ((int64_t)v * f.width + u);
    for (int k = 0; k < 3; ++k) s[k] = (double)px[k];
  } else if (g.color_type == 2) {
    s[0] = s[1] = s[2] = (double)rgbd_load_f32(in + f.color_off + 4 * ((int64_t)v * f.width + u));
  }
  return true;
}

// The running averages of one voxel; the weight last.
__host__ __device__ __forceinline__ void tsdf_update(const TsdfGrid& g, float t, const double* s, float* tsdf,
                                                     float* weight, double* color) {
  const float w = *weight, w1 = w + 1.0f;
  *tsdf = (*tsdf * w + t) / w1;
  if (g.color_type != 0)
    for (int k = 0; k < 3; ++k) {
      const double v = (color[k] * (double)w + s[k]) / (double)w1;
      color[k] = g.color_type == 2 ? rgbd_canonical(v) : v;
    }
  *weight = w1;
}

__host__ __device__ __forceinline__ bool tsdf_usable(float w, float f) { return w != 0.0f && f < 0.98f && f >= -0.98f; }

// The fields of the volume on the device; color is three planes of n voxels (NULL without a colour type).
struct TsdfFields {
  float* tsdf;
  float* weight;
  double* color;
  int64_t n;  // R^3
};

// Whether the usable voxel (x, y, z) with value f0 gives a row along axis i; then *at1 is its neighbour and *f1 its value.
__host__ __device__ __forceinline__ bool tsdf_surface_row(const TsdfGrid& g, const TsdfFields& v, int x, int y, int z,
                                                          int i, float f0, int64_t* at1, float* f1) {
  const int nx = x + (i == 0), ny = y + (i == 1), nz = z + (i == 2);
  const int along = i == 0 ? nx : (i == 1 ? ny : nz);
  if (!(along < g.R - 1)) return false;
  *at1 = tsdf_index(g.R, nx, ny, nz);
  *f1 = v.tsdf[*at1];
  return tsdf_usable(v.weight[*at1], *f1) && f0 * *f1 < 0.0f;
}

// The rows voxel (x, y, z) gives: 0 .. 3 (mode 0, the surface) or 0 .. 1 (mode 1, the voxel cloud).
__host__ __device__ __forceinline__ int tsdf_voxel_rows(const TsdfGrid& g, const TsdfFields& v, int mode, int x, int y,
                                                        int z) {
  const int64_t at0 = tsdf_index(g.R, x, y, z);
  const float f0 = v.tsdf[at0];
  if (!tsdf_usable(v.weight[at0], f0)) return 0;
  if (mode == 1) return 1;
  int rows = 0;
  for (int i = 0; i < 3; ++i) {
    int64_t at1;
    float f1;
    if (tsdf_surface_row(g, v, x, y, z, i, f0, &at1, &f1)) ++rows;
  }
  return rows;
}

// T(q): the trilinear value of the TSDF at q (volume coordinates); a corner outside the volume has the value 0.
__host__ __device__ __forceinline__ double tsdf_trilinear(const TsdfGrid& g, const TsdfFields& v, const double* q) {
  int idx[3];
  double r[3];
  for (int k = 0; k < 3; ++k) {
    const double a = q[k] / g.vl - 0.5, fl = __builtin_floor(a);
    r[k] = a - fl;
    idx[k] = (int)fl;  // q lies within a voxel of the volume: no overflow
  }
  double sum = 0.0;
  for (int corner = 0; corner < 8; ++corner) {
    const int ox = corner >> 2, oy = (corner >> 1) & 1, oz = corner & 1;
    const int cx = idx[0] + ox, cy = idx[1] + oy, cz = idx[2] + oz;
    const bool inside = cx >= 0 && cx < g.R && cy >= 0 && cy < g.R && cz >= 0 && cz < g.R;
    const float f = inside ? v.tsdf[tsdf_index(g.R, cx, cy, cz)] : 0.0f;
    const double term = (((ox ? r[0] : 1.0 - r[0]) * (oy ? r[1] : 1.0 - r[1])) * (oz ? r[2] : 1.0 - r[2])) * (double)f;
    sum = corner == 0 ? term : sum + term;
  }
  return sum;
}

// The normal at p (volume coordinates): the central differences of T over g = 0.99 vl, normalised unless zero.
__host__ __device__ __forceinline__ void tsdf_normal_at(const TsdfGrid& g, const TsdfFields& v, const double* p,
                                                        double* normal) {
  const double gstep = 0.99 * g.vl;
  double n[3];
  for (int k = 0; k < 3; ++k) {
    double hi[3] = {p[0], p[1], p[2]}, lo[3] = {p[0], p[1], p[2]};
    hi[k] = p[k] + gstep;
    lo[k] = p[k] - gstep;
    n[k] = tsdf_trilinear(g, v, hi) - tsdf_trilinear(g, v, lo);
  }
  const double s = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  if (s > 0.0) {
    const double len = __builtin_sqrt(s);
    for (int k = 0; k < 3; ++k) n[k] = n[k] / len;
  }
  for (int k = 0; k < 3; ++k) normal[k] = n[k];
}

// The surface point between voxel (x, y, z) (value f0) and its neighbour along i (at1, value f1): point, and where the
// pointers are given the normal and the colour.
__host__ __device__ __forceinline__ void tsdf_surface_point(const TsdfGrid& g, const TsdfFields& v, int x, int y, int z,
                                                            int i, float f0, int64_t at1, float f1, double* point,
                                                            double* normal, double* color) {
  const float r0 = __builtin_fabsf(f0), r1 = __builtin_fabsf(f1);
  const double den = (double)(r0 + r1);
  double p[3] = {g.half + g.vl * (double)x, g.half + g.vl * (double)y, g.half + g.vl * (double)z};
  const double p1 = p[i] + g.vl;
  p[i] = (p[i] * (double)r1 + p1 * (double)r0) / den;
  for (int k = 0; k < 3; ++k) point[k] = p[k] + g.origin[k];
  if (color) {
    const int64_t at0 = tsdf_index(g.R, x, y, z);
    for (int k = 0; k < 3; ++k) {
      double c = (v.color[k * v.n + at0] * (double)r1 + v.color[k * v.n + at1] * (double)r0) / den;
      if (g.color_type == 1) c = c / 255.0;
      color[k] = g.color_type == 2 ? rgbd_canonical(c) : c;
    }
  }
  if (normal) tsdf_normal_at(g, v, p, normal);
}

// The row of the voxel cloud for the usable voxel (x, y, z) with value f0.
__host__ __device__ __forceinline__ void tsdf_voxel_point(const TsdfGrid& g, int x, int y, int z, float f0, double* point,
                                                          double* color) {
  point[0] = (g.half + g.vl * (double)x) + g.origin[0];
  point[1] = (g.half + g.vl * (double)y) + g.origin[1];
  point[2] = (g.half + g.vl * (double)z) + g.origin[2];
  if (color) color[0] = color[1] = color[2] = ((double)f0 + 1.0) * 0.5;
}

// The z segments of the integration launch: enough of them to reach kTsdfWaveTarget waves, R at the most.
__host__ __device__ __forceinline__ int tsdf_segments(int R) {
  const int64_t waves = ((int64_t)R * R + 63) / 64;
  const int64_t want = (kTsdfWaveTarget + waves - 1) / waves;
  return (int)(want < 1 ? 1 : (want > R ? R : want));
}

// ---- launchers (kernels_tsdf.hip; tests/tsdf_host_driver.cpp has serial stand-ins) ----
// One pass: ck.n frames applied in order to every voxel.
void launch_tsdf_integrate(hipStream_t s, const TsdfGrid& g, const TsdfChunkArgs& ck, const unsigned char* d_in,
                           const TsdfFields& v);
// counts[x R + y] = the rows of the column, offsets = their exclusive sum with the total at offsets[R R].
void launch_tsdf_count(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, int mode, int32_t* d_counts,
                       int64_t* d_offsets);
// The scan alone (one block): offsets = the exclusive sum of n counts with the total at offsets[n].  The scalable volume
// runs it over its blocks (kernels_stsdf.hip).
void launch_tsdf_scan(hipStream_t s, const int32_t* d_counts, int64_t n, int64_t* d_offsets);
// The rows, from every column's offset, unless the total exceeds capacity (then nothing is written).  Any of normals and
// colors may be NULL.
void launch_tsdf_write(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, int mode, const int64_t* d_offsets,
                       int64_t capacity, double* d_points, double* d_normals, double* d_colors);
// Between the device layout and Open3D's voxel order (x R + y) R + z: tw is n x 2 floats (tsdf, weight), color n x 3.
void launch_tsdf_export(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, float* d_tw, double* d_color);
void launch_tsdf_import(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, const float* d_tw, const double* d_color);

}  // namespace thip
