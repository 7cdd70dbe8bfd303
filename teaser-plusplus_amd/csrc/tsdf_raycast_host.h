// tsdf_raycast_host.h -- what the host sides of the two ray casts share (tsdf_raycast.hip: the dense volume;
// stsdf_raycast.hip: the scalable one): the checks of a view, its record, the blocks and the block map of a call, the
// layout of the maps and their way back to the caller's arrays.  Both calls refuse the same things in the same words.
#pragma once

#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "host_common.h"
#include "tsdf_internal.h"
#include "tsdf_raycast_device.h"

namespace thip {

inline std::string view_at(int b) { return " (view " + std::to_string(b) + ")"; }

inline int32_t check_view(HandleBase* h, int b, const teaser_tsdf_view_c& w) {
  if (w.width < 0 || w.height < 0 || w.width > kRgbdMaxSide || w.height > kRgbdMaxSide)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "width and height must lie in [0, 16384]" + view_at(b));
  if (!std::isfinite(w.fx) || !std::isfinite(w.fy) || w.fx == 0.0 || w.fy == 0.0)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "fx and fy must be finite and not zero" + view_at(b));
  if (!std::isfinite(w.cx) || !std::isfinite(w.cy))
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "cx and cy must be finite" + view_at(b));
  if (!finite_all(w.extrinsic, 16))
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "extrinsic has a non-finite entry" + view_at(b));
  if (!std::isfinite(w.depth_min) || !std::isfinite(w.depth_max) || !std::isfinite(w.weight_threshold))
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_min, depth_max and weight_threshold must be finite" + view_at(b));
  if (w.depth_min < 0.0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_min must be >= 0" + view_at(b));
  if (w.depth_max < w.depth_min)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_max must not be below depth_min" + view_at(b));
  if (w.reserved != 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "reserved must be 0" + view_at(b));
  return TEASER_HIP_OK;
}

// The camera of a view: the centre in double, then the float32 constants of the contract.  origin: the volume's (the
// scalable volume has the origin 0).
inline void ray_camera(const double* origin, const teaser_tsdf_view_c& w, TsdfRayView* d) {
  const double* E = w.extrinsic;
  for (int k = 0; k < 3; ++k) {
    const double c = -((E[k] * E[3] + E[4 + k] * E[7]) + E[8 + k] * E[11]);
    d->o[k] = (float)(c - origin[k]);
    for (int j = 0; j < 3; ++j) d->Rt[3 * k + j] = (float)E[4 * j + k];
  }
  d->fx = (float)w.fx, d->fy = (float)w.fy, d->cx = (float)w.cx, d->cy = (float)w.cy;
  d->dmin = (float)w.depth_min, d->dmax = (float)w.depth_max, d->wthr = (float)w.weight_threshold;
  d->width = w.width, d->height = w.height;
}

// A call laid out.  Input buffer: the view records, then (at o_map_in) the block map.  Output buffer: the blocks' hit
// counts, then (at o_maps) the maps, whose offsets are in floats.
struct RayPlan {
  std::vector<TsdfRayView> rec;
  int64_t n_blocks = 0;
  size_t o_maps = 0, o_end = 0, o_map_in = 0, in_bytes = 0;
};

// Checks the views, builds their records and counts the blocks; zeroes hit_counts.  The layout is ray_layout's.
inline int32_t ray_plan(HandleBase* h, int color_type, const double* origin, int32_t n_views, const teaser_tsdf_view_c* views,
                        float* const* color, int64_t* hit_counts, RayPlan* p) {
  p->rec.assign((size_t)n_views, TsdfRayView());
  p->n_blocks = 0;
  for (int b = 0; b < n_views; ++b) {
    const int32_t rc = check_view(h, b, views[b]);
    if (rc != TEASER_HIP_OK) return rc;
    if (color && color[b] && color_type == 0)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "color is asked of a volume without colour" + view_at(b));
    TsdfRayView& d = p->rec[(size_t)b];
    memset(&d, 0, sizeof(d));
    ray_camera(origin, views[b], &d);
    d.tiles_x = (d.width + kTsdfRayTile - 1) / kTsdfRayTile;
    const int64_t tiles = d.width > 0 && d.height > 0 ? (int64_t)d.tiles_x * ((d.height + kTsdfRayTile - 1) / kTsdfRayTile) : 0;
    if (p->n_blocks + tiles > 2147483647)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "the views of one call need more than 2147483647 blocks" + view_at(b));
    d.blk0 = (int32_t)p->n_blocks;
    p->n_blocks += tiles;
  }
  if (hit_counts)
    for (int b = 0; b < n_views; ++b) hit_counts[b] = 0;
  return TEASER_HIP_OK;
}

inline void ray_layout(int32_t n_views, float* const* depth, float* const* vertex, float* const* normal, float* const* color,
                       RayPlan* p) {
  p->o_maps = round_up(sizeof(int32_t) * (size_t)p->n_blocks, 256);
  size_t floats = 0;
  for (int b = 0; b < n_views; ++b) {
    TsdfRayView& d = p->rec[(size_t)b];
    const size_t px = (size_t)d.width * (size_t)d.height;
    const bool want[4] = {depth && depth[b], vertex && vertex[b], normal && normal[b], color && color[b]};
    int64_t* off[4] = {&d.depth_off, &d.vertex_off, &d.normal_off, &d.color_off};
    for (int m = 0; m < 4; ++m) {
      *off[m] = want[m] && px > 0 ? (int64_t)floats : -1;
      if (want[m]) floats += round_up((m == 0 ? 1 : 3) * px, 64);  // a map starts on a 256-byte line
    }
  }
  p->o_end = p->o_maps + sizeof(float) * floats;
  p->o_map_in = round_up(sizeof(TsdfRayView) * (size_t)n_views, 256);
  p->in_bytes = p->o_map_in + sizeof(int32_t) * (size_t)p->n_blocks;
}

inline int32_t ray_view_end(const RayPlan& p, int b) {
  return (size_t)b + 1 < p.rec.size() ? p.rec[(size_t)b + 1].blk0 : (int32_t)p.n_blocks;
}

// The input buffer of the call: in_bytes at stage.
inline void ray_stage(const RayPlan& p, char* stage) {
  memset(stage, 0, p.o_map_in);
  memcpy(stage, p.rec.data(), sizeof(TsdfRayView) * p.rec.size());
  int32_t* map = reinterpret_cast<int32_t*>(stage + p.o_map_in);
  for (int b = 0; b < (int)p.rec.size(); ++b)
    for (int32_t k = p.rec[(size_t)b].blk0, end = ray_view_end(p, b); k < end; ++k) map[k] = b;
}

// Every requested map from the output buffer's copy `back` into its caller's array, and the counts of the views.
inline void ray_hand_out(const RayPlan& p, const char* back, float* const* depth, float* const* vertex, float* const* normal,
                         float* const* color, int64_t* hit_counts) {
  const int32_t* blk_hits = reinterpret_cast<const int32_t*>(back);
  const float* maps = reinterpret_cast<const float*>(back + p.o_maps);
  for (int b = 0; b < (int)p.rec.size(); ++b) {
    const TsdfRayView& d = p.rec[(size_t)b];
    const size_t px = (size_t)d.width * (size_t)d.height;
    if (px == 0) continue;
    if (d.depth_off >= 0) memcpy(depth[b], maps + d.depth_off, sizeof(float) * px);
    if (d.vertex_off >= 0) memcpy(vertex[b], maps + d.vertex_off, sizeof(float) * 3 * px);
    if (d.normal_off >= 0) memcpy(normal[b], maps + d.normal_off, sizeof(float) * 3 * px);
    if (d.color_off >= 0) memcpy(color[b], maps + d.color_off, sizeof(float) * 3 * px);
    if (hit_counts) {
      int64_t sum = 0;
      for (int32_t k = d.blk0, end = ray_view_end(p, b); k < end; ++k) sum += blk_hits[k];
      hit_counts[b] = sum;
    }
  }
}

}  // namespace thip
