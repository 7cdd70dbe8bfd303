// stsdf_raycast_device.h -- the per-pixel rules of the ray cast of the scalable TSDF volume (include/teaser_hip.h,
// "Scalable TSDF ray casting"; kernel: kernels_stsdf_raycast.hip, host side: stsdf_raycast.hip, design, bounds and the
// resource report: DESIGN.md section 38): the march over the open blocks with the skip of a block that is not open, and
// the maps of a hit on the global lattice.  The view, the ray of a pixel and the pixel a thread serves are those of the
// dense ray cast (tsdf_raycast_device.h).  Nothing here uses a wave operation or LDS, so
// tests/stsdf_raycast_host_driver.cpp runs this very source in serial loops.
//
// The library is compiled with -ffp-contract=off: no product-add is fused, and every sum is written out left to right.
#pragma once

#include "stsdf_device.h"
#include "tsdf_raycast_device.h"

namespace thip {

constexpr float kStsdfRayRange = 16777216.0f;  // a voxel index of a sample lies in [-2^24, 2^24)
constexpr int kStsdfRayMaxSteps = 1 << 20;     // the largest step cap of a view

struct StsdfRayArgs {
  const TsdfRayView* views;
  const int32_t* blk_view;  // the block map: the view of every block
  float* out;               // the maps
  int32_t* blk_hits;        // per block the number of hit pixels
  float ul_f;               // (float)ul
  int32_t pad;
};

// A hit: the dense record and the block it lies in.
struct StsdfRayHit {
  TsdfRayHit h;
  int b[3];
  char* base;
};

// The march from dmin: true at a hit.  The lane keeps the last block it looked up (its index triple and its address,
// NULL when it is not open) and searches the directory only when the block changes; the look-up is a pure function of
// the triple, so no bit depends on that.  No address is formed from an index that has not passed the range test, and
// the loop ends after w.n_cap steps whatever the floats do.
__host__ __device__ __forceinline__ bool stsdf_ray_march(const TsdfGrid& g, const StsdfDir& dir, float ul_f,
                                                         const TsdfRayView& w, const float* d, StsdfRayHit* hit) {
  float t = w.dmin, t_prev = w.dmin, f_prev = -1.0f;
  const float t1 = w.dmax;
  float cb0 = kStsdfRayRange, cb1 = kStsdfRayRange, cb2 = kStsdfRayRange;  // no block has this index
  char* base = nullptr;
  for (int step = 0; step < w.n_cap; ++step) {
    if (!(t <= t1)) return false;
    float q[3], B[3];
    for (int k = 0; k < 3; ++k) {
      const float p = w.o[k] + t * d[k];
      q[k] = __builtin_floorf(p / g.vl_f);
    }
    for (int k = 0; k < 3; ++k)
      if (!(q[k] >= -kStsdfRayRange && q[k] < kStsdfRayRange)) return false;  // a NaN, too
    for (int k = 0; k < 3; ++k) B[k] = __builtin_floorf(q[k] / 16.0f);
    if (B[0] != cb0 || B[1] != cb1 || B[2] != cb2) {
      cb0 = B[0], cb1 = B[1], cb2 = B[2];
      base = stsdf_find(dir, (int64_t)B[0], (int64_t)B[1], (int64_t)B[2]);  // |B| <= 2^20 by the range test
    }
    if (base) {
      const int lx = (int)(q[0] - 16.0f * B[0]), ly = (int)(q[1] - 16.0f * B[1]), lz = (int)(q[2] - 16.0f * B[2]);
      const int64_t at = tsdf_index(kStsdfU, lx, ly, lz);  // 0 <= every index < 16: q - 16 floor(q / 16) is exact
      const float* plane = reinterpret_cast<const float*>(base);
      const float f = plane[at], wgt = plane[kStsdfVoxels + at];
      if (f_prev > 0.0f && wgt >= w.wthr && f <= 0.0f) {
        hit->h.t = t, hit->h.t_prev = t_prev, hit->h.f = f, hit->h.f_prev = f_prev;
        hit->b[0] = (int)B[0], hit->b[1] = (int)B[1], hit->b[2] = (int)B[2];
        hit->base = base;
        return true;
      }
      t_prev = t;
      f_prev = f;
      const float delta = f * g.trunc_f;
      t = t + (delta < g.vl_f ? g.vl_f : delta);
    } else {  // not open: nothing observed here; on to the face the ray leaves the block by
      t_prev = t;
      f_prev = 0.0f;
      bool any = false;
      float t_exit = 0.0f;
      for (int k = 0; k < 3; ++k)
        if (d[k] != 0.0f) {
          const float face = (d[k] > 0.0f ? B[k] + 1.0f : B[k]) * ul_f;
          const float e = (face - w.o[k]) / d[k];
          t_exit = !any || e < t_exit ? e : t_exit;
          any = true;
        }
      const float t_next = t + g.vl_f;
      t = any && t_exit > t_next ? t_exit : t_next;
    }
  }
  return false;
}

// The colour at q (world coordinates, NEAR): the dense rule over the corners of the global lattice; a corner counts when
// its block is open and its weight is not 0.  b and own: the block of the hit, which most corners lie in.
__host__ __device__ __forceinline__ void stsdf_ray_color(const TsdfGrid& g, const StsdfDir& dir, const int* b, char* own,
                                                         const double* q, double* color) {
  int64_t idx[3];
  double r[3];
  for (int k = 0; k < 3; ++k) {
    const double a = q[k] / g.vl - 0.5, fl = __builtin_floor(a);
    r[k] = a - fl;
    idx[k] = (int64_t)fl;  // q is NEAR: |q / vl| <= 2^24 + 2
  }
  double num[3] = {0.0, 0.0, 0.0}, den = 0.0;
  for (int corner = 0; corner < 8; ++corner) {
    const int ox = corner >> 2, oy = (corner >> 1) & 1, oz = corner & 1;
    const int64_t cx = idx[0] + ox, cy = idx[1] + oy, cz = idx[2] + oz;
    const int64_t bx = cx >> 4, by = cy >> 4, bz = cz >> 4;  // floor division by kStsdfU
    char* base = own;
    if (bx != b[0] || by != b[1] || bz != b[2]) base = stsdf_find(dir, bx, by, bz);
    if (!base) continue;
    const TsdfFields v = stsdf_fields(base, g.color_type);
    const int64_t at = tsdf_index(kStsdfU, (int)(cx & 15), (int)(cy & 15), (int)(cz & 15));
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
__host__ __device__ __forceinline__ void stsdf_ray_finish(const TsdfGrid& g, const StsdfDir& dir, const TsdfRayView& w,
                                                          const float* d, const StsdfRayHit& hit, float* depth,
                                                          float* vertex, float* normal, float* color) {
  const float ts = (hit.h.t * hit.h.f_prev - hit.h.t_prev * hit.h.f) / (hit.h.f_prev - hit.h.f);
  *depth = ts;
  double q[3];
  bool is_near = true;
  const double reach = 16777218.0 * g.vl;  // (2^24 + 2) vl
  for (int k = 0; k < 3; ++k) {
    q[k] = (double)w.o[k] + (double)ts * (double)d[k];
    is_near = is_near && q[k] >= -reach && q[k] <= reach;
  }
  if (vertex)
    for (int k = 0; k < 3; ++k) vertex[k] = (float)q[k];
  if (normal) {
    double n[3] = {0.0, 0.0, 0.0};
    if (is_near) stsdf_normal_at(g, dir, hit.b, reinterpret_cast<const float*>(hit.base), q, n);
    for (int k = 0; k < 3; ++k) normal[k] = (float)n[k];
  }
  if (color) {
    double c[3] = {0.0, 0.0, 0.0};
    if (is_near) stsdf_ray_color(g, dir, hit.b, hit.base, q, c);
    for (int k = 0; k < 3; ++k) color[k] = tsdf_ray_f32(c[k]);
  }
}

// Everything thread `thread` of block `block` does but the block's hit count: true when its pixel is a hit.  Every
// requested map of every pixel of the image is written, a missed pixel with zeros.  A volume with no open block is
// missed by every pixel without a step.
__host__ __device__ __forceinline__ bool stsdf_ray_thread(const TsdfGrid& g, const StsdfDir& dir, const StsdfRayArgs& a,
                                                          int block, int thread) {
  const TsdfRayView& w = a.views[a.blk_view[block]];
  int pv, pu;
  if (!tsdf_ray_pixel(w, block - w.blk0, thread, &pv, &pu)) return false;
  float d[3];
  StsdfRayHit hit;
  tsdf_ray(w, pv, pu, d);
  const bool is_hit = dir.n > 0 && stsdf_ray_march(g, dir, a.ul_f, w, d, &hit);
  const int64_t px = (int64_t)pv * w.width + pu;
  float* depth = w.depth_off >= 0 ? a.out + w.depth_off + px : nullptr;
  float* vertex = w.vertex_off >= 0 ? a.out + w.vertex_off + 3 * px : nullptr;
  float* normal = w.normal_off >= 0 ? a.out + w.normal_off + 3 * px : nullptr;
  float* color = w.color_off >= 0 ? a.out + w.color_off + 3 * px : nullptr;
  if (is_hit) {  // after the march: the look-ups of a normal and the corners of a colour are a hit lane's alone
    float z;
    stsdf_ray_finish(g, dir, w, d, hit, &z, vertex, normal, color);
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

// ---- launcher (kernels_stsdf_raycast.hip; tests/stsdf_raycast_host_driver.cpp has a serial stand-in) ----
// n_blocks blocks of kTsdfRayBlock threads; blk_hits[b] = the hit pixels of block b.
void launch_stsdf_raycast(hipStream_t s, const TsdfGrid& g, const StsdfDir& dir, const StsdfRayArgs& a, int32_t n_blocks);

}  // namespace thip
