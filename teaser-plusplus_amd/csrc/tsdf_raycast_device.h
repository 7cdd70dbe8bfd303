// tsdf_raycast_device.h -- the per-pixel rules of the ray cast of the TSDF volume (include/teaser_hip.h, "TSDF ray
// casting"; kernel: kernels_tsdf_raycast.hip, host side: tsdf_raycast.hip, design, bounds and the resource report:
// DESIGN.md section 35): which pixel a thread of a block serves, the ray of a pixel, its clip against the volume's box,
// the march to the first surface and the maps of a hit.  Nothing here uses a wave operation or LDS, so
// tests/tsdf_raycast_host_driver.cpp runs this very source in serial loops.
//
// The library is compiled with -ffp-contract=off: no product-add is fused, and every sum is written out left to right.
#pragma once

#include "tsdf_device.h"

namespace thip {

constexpr int kTsdfRayTile = 16;                            // a block serves 16 x 16 pixels of one view
constexpr int kTsdfRayBlock = kTsdfRayTile * kTsdfRayTile;  // its threads: four waves

// One view of a ray-cast call (host-built, read-only on the device).  The maps are float offsets into the output
// buffer, -1 for a map that is not wanted.
struct TsdfRayView {
  float o[3];    // the centre in volume coordinates
  float Rt[9];   // camera to world, row-major
  float fx, fy, cx, cy;
  float dmin, dmax, wthr;
  int32_t width, height;
  int32_t tiles_x;  // blocks across a row of tiles
  int32_t blk0;     // the view's first block
  int32_t n_cap;    // the step cap of the scalable volume's march (stsdf_raycast_device.h); 0 and unread in the dense call
  int64_t depth_off, vertex_off, normal_off, color_off;
};

struct TsdfRayArgs {
  const TsdfRayView* views;
  const int32_t* blk_view;  // the block map: the view of every block
  float* out;               // the maps
  int32_t* blk_hits;        // per block the number of hit pixels
  float L_f;                // (float)length
  int32_t pad;
};

// The pixel of thread `thread` of the view's tile `tile`: false outside the image.  A wave (64 consecutive threads)
// serves an 8 x 8 quadrant of the tile, so that its rays stay neighbours in all three axes of the volume; the mapping
// lives here alone and no bit depends on it.
__host__ __device__ __forceinline__ bool tsdf_ray_pixel(const TsdfRayView& w, int tile, int thread, int* v, int* u) {
  const int ty = tile / w.tiles_x, tx = tile - ty * w.tiles_x;
  const int wave = thread >> 6, lane = thread & 63;
  *u = tx * kTsdfRayTile + ((wave & 1) << 3) + (lane & 7);
  *v = ty * kTsdfRayTile + ((wave >> 1) << 3) + (lane >> 3);
  return *u < w.width && *v < w.height;
}

__host__ __device__ __forceinline__ void tsdf_ray(const TsdfRayView& w, int v, int u, float* d) {
  const float a = ((float)u - w.cx) / w.fx, b = ((float)v - w.cy) / w.fy;
  for (int k = 0; k < 3; ++k) d[k] = (w.Rt[3 * k] * a + w.Rt[3 * k + 1] * b) + w.Rt[3 * k + 2];
}

// The box clip: false when an axis the ray runs along a plane of lies outside the volume.
__host__ __device__ __forceinline__ bool tsdf_ray_clip(const TsdfRayView& w, float L_f, const float* d, float* t0,
                                                       float* t1) {
  float a = w.dmin, b = w.dmax;
  for (int k = 0; k < 3; ++k) {
    if (d[k] != 0.0f) {
      float lo = (0.0f - w.o[k]) / d[k], hi = (L_f - w.o[k]) / d[k];
      if (hi < lo) {
        const float s = lo;
        lo = hi;
        hi = s;
      }
      a = a < lo ? lo : a;
      b = hi < b ? hi : b;
    } else if (!(w.o[k] >= 0.0f && w.o[k] < L_f)) {
      return false;
    }
  }
  *t0 = a;
  *t1 = b;
  return true;
}

struct TsdfRayHit {
  float t, t_prev, f, f_prev;
};

// The march from t0: true at a hit.  No voxel outside the volume is read whatever t is, and the loop ends after
// 2 R + 2 steps whatever the floats do.
__host__ __device__ __forceinline__ bool tsdf_ray_march(const TsdfGrid& g, const TsdfFields& v, const TsdfRayView& w,
                                                        const float* d, float t0, float t1, TsdfRayHit* hit) {
  float t = t0, t_prev = t0, f_prev = -1.0f;
  const float R_f = (float)g.R;
  const int cap = 2 * g.R + 2;
  for (int step = 0; step < cap; ++step) {
    if (!(t <= t1)) return false;
    float q[3];
    for (int k = 0; k < 3; ++k) {
      const float p = w.o[k] + t * d[k];
      q[k] = __builtin_floorf(p / g.vl_f);
    }
    float f = 0.0f, wgt = 0.0f;
    if (q[0] >= 0.0f && q[0] < R_f && q[1] >= 0.0f && q[1] < R_f && q[2] >= 0.0f && q[2] < R_f) {
      const int64_t at = tsdf_index(g.R, (int)q[0], (int)q[1], (int)q[2]);  // 0 <= every index < R by the test
      f = v.tsdf[at];
      wgt = v.weight[at];
    }
    if (f_prev > 0.0f && wgt >= w.wthr && f <= 0.0f) {
      hit->t = t, hit->t_prev = t_prev, hit->f = f, hit->f_prev = f_prev;
      return true;
    }
    t_prev = t;
    f_prev = f;
    const float delta = f * g.trunc_f;
    t = t + (delta < g.vl_f ? g.vl_f : delta);
  }
  return false;
}

__host__ __device__ __forceinline__ float tsdf_ray_f32(double x) {
  return x != x ? __builtin_bit_cast(float, 0x7fc00000u) : (float)x;
}

// The colour at q (volume coordinates, NEAR): the weighted mean over the observed trilinear corners.
__host__ __device__ __forceinline__ void tsdf_ray_color(const TsdfGrid& g, const TsdfFields& v, const double* q,
                                                        double* color) {
  int idx[3];
  double r[3];
  for (int k = 0; k < 3; ++k) {
    const double a = q[k] / g.vl - 0.5, fl = __builtin_floor(a);
    r[k] = a - fl;
    idx[k] = (int)fl;  // q is NEAR: within three voxels of the volume
  }
  double num[3] = {0.0, 0.0, 0.0}, den = 0.0;
  for (int corner = 0; corner < 8; ++corner) {
    const int ox = corner >> 2, oy = (corner >> 1) & 1, oz = corner & 1;
    const int cx = idx[0] + ox, cy = idx[1] + oy, cz = idx[2] + oz;
    if (!(cx >= 0 && cx < g.R && cy >= 0 && cy < g.R && cz >= 0 && cz < g.R)) continue;
    const int64_t at = tsdf_index(g.R, cx, cy, cz);
    if (!(v.weight[at] != 0.0f)) continue;
    const double omega = ((ox ? r[0] : 1.0 - r[0]) * (oy ? r[1] : 1.0 - r[1])) * (oz ? r[2] : 1.0 - r[2]);
    for (int k = 0; k < 3; ++k) num[k] = num[k] + omega * v.color[k * v.n + at];
    den = den + omega;
  }
  for (int k = 0; k < 3; ++k) {
    double c = den > 0.0 ? num[k] / den : 0.0;
    if (g.color_type == 1) c = c / 255.0;
    color[k] = c;
  }
}

// The maps of a hit: the depth and, where the pointers are given, the world point, the normal and the colour (three
// floats each).
__host__ __device__ __forceinline__ void tsdf_ray_finish(const TsdfGrid& g, const TsdfFields& v, const TsdfRayView& w,
                                                         const float* d, const TsdfRayHit& hit, float* depth, float* vertex,
                                                         float* normal, float* color) {
  const float ts = (hit.t * hit.f_prev - hit.t_prev * hit.f) / (hit.f_prev - hit.f);
  *depth = ts;
  double q[3];
  bool is_near = true;
  const double length = g.vl * (double)g.R, margin = 2.0 * g.vl;
  for (int k = 0; k < 3; ++k) {
    q[k] = (double)w.o[k] + (double)ts * (double)d[k];
    is_near = is_near && q[k] >= -margin && q[k] <= length + margin;
  }
  if (vertex)
    for (int k = 0; k < 3; ++k) vertex[k] = (float)(q[k] + g.origin[k]);
  if (normal) {
    double n[3] = {0.0, 0.0, 0.0};
    if (is_near) tsdf_normal_at(g, v, q, n);
    for (int k = 0; k < 3; ++k) normal[k] = (float)n[k];
  }
  if (color) {
    double c[3] = {0.0, 0.0, 0.0};
    if (is_near) tsdf_ray_color(g, v, q, c);
    for (int k = 0; k < 3; ++k) color[k] = tsdf_ray_f32(c[k]);
  }
}

// Everything thread `thread` of block `block` does but the block's hit count: true when its pixel is a hit.  Every
// requested map of every pixel of the image is written, a missed pixel with zeros.
__host__ __device__ __forceinline__ bool tsdf_ray_thread(const TsdfGrid& g, const TsdfFields& v, const TsdfRayArgs& a,
                                                         int block, int thread) {
  const TsdfRayView& w = a.views[a.blk_view[block]];
  int pv, pu;
  if (!tsdf_ray_pixel(w, block - w.blk0, thread, &pv, &pu)) return false;
  float d[3], t0, t1;
  TsdfRayHit hit;
  tsdf_ray(w, pv, pu, d);
  const bool is_hit = tsdf_ray_clip(w, a.L_f, d, &t0, &t1) && tsdf_ray_march(g, v, w, d, t0, t1, &hit);
  const int64_t px = (int64_t)pv * w.width + pu;
  float* depth = w.depth_off >= 0 ? a.out + w.depth_off + px : nullptr;
  float* vertex = w.vertex_off >= 0 ? a.out + w.vertex_off + 3 * px : nullptr;
  float* normal = w.normal_off >= 0 ? a.out + w.normal_off + 3 * px : nullptr;
  float* color = w.color_off >= 0 ? a.out + w.color_off + 3 * px : nullptr;
  if (is_hit) {  // after the march: the 48 loads of a normal and the corners of a colour are a hit lane's alone
    float z;
    tsdf_ray_finish(g, v, w, d, hit, &z, vertex, normal, color);
    if (depth) *depth = z;
    return true;
  }
  if (depth) *depth = 0.0f;
  for (int k = 0; k < 3; ++k) {
    if (vertex) vertex[k] = 0.0f;
    if (normal) normal[k] = 0.0f;
    if (color) color[k] = 0.0f;
  }
  return false;
}

// ---- launcher (kernels_tsdf_raycast.hip; tests/tsdf_raycast_host_driver.cpp has a serial stand-in) ----
// n_blocks blocks of kTsdfRayBlock threads; blk_hits[b] = the hit pixels of block b.
void launch_tsdf_raycast(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, const TsdfRayArgs& a, int32_t n_blocks);

}  // namespace thip
