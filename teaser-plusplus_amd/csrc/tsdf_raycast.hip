// tsdf_raycast.hip -- host side of the ray cast of the TSDF volume (include/teaser_hip.h, "TSDF ray casting"): the entry
// checks, the cameras, the layout of a call and its one round trip.  Kernel: kernels_tsdf_raycast.hip; device code:
// tsdf_raycast_device.h; design, bounds and the resource report: DESIGN.md section 35.
//
// A call: the view records and the block map go up in one copy; one launch over the blocks of all views writes the
// blocks' hit counts and the requested maps of every pixel into one buffer; one copy brings that buffer back into the
// handle's page-locked buffer, one synchronisation, and the host hands every map to its caller's array and adds the
// counts.  Neither the launch nor the synchronisation depends on the data.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "tsdf_internal.h"
#include "tsdf_raycast_device.h"

using namespace thip;

namespace {

inline std::string view_at(int b) { return " (view " + std::to_string(b) + ")"; }

int32_t check_view(teaser_hip_tsdf* h, int b, const teaser_tsdf_view_c& w) {
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

// The camera of a view: the centre in double, then the float32 constants of the contract.
void camera(const TsdfGrid& g, const teaser_tsdf_view_c& w, TsdfRayView* d) {
  const double* E = w.extrinsic;
  for (int k = 0; k < 3; ++k) {
    const double c = -((E[k] * E[3] + E[4 + k] * E[7]) + E[8 + k] * E[11]);
    d->o[k] = (float)(c - g.origin[k]);
    for (int j = 0; j < 3; ++j) d->Rt[3 * k + j] = (float)E[4 * j + k];
  }
  d->fx = (float)w.fx, d->fy = (float)w.fy, d->cx = (float)w.cx, d->cy = (float)w.cy;
  d->dmin = (float)w.depth_min, d->dmax = (float)w.depth_max, d->wthr = (float)w.weight_threshold;
  d->width = w.width, d->height = w.height;
}

}  // namespace

extern "C" {

int32_t teaser_hip_tsdf_view_default(teaser_tsdf_view_c* w) {
  if (!w) return TEASER_HIP_ERR_BAD_ARG;
  memset(w, 0, sizeof(*w));
  for (int k = 0; k < 4; ++k) w->extrinsic[5 * k] = 1.0;
  w->depth_min = 0.1;
  w->depth_max = 3.0;
  w->weight_threshold = 3.0;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_tsdf_ray_cast_views(teaser_hip_tsdf* h, int32_t n_views, const teaser_tsdf_view_c* views,
                                       float* const* depth, float* const* vertex, float* const* normal,
                                       float* const* color, int64_t* hit_counts) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (n_views < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_views must be >= 0");
  if (n_views == 0) return TEASER_HIP_OK;
  if (!views) return fail(h, TEASER_HIP_ERR_BAD_ARG, "views must not be NULL");
  const TsdfGrid& g = h->g;
  std::vector<TsdfRayView> rec((size_t)n_views);
  // the layout: the blocks' hit counts lie in front of the maps; offsets in floats
  int64_t n_blocks = 0;
  for (int b = 0; b < n_views; ++b) {
    const int32_t rc = check_view(h, b, views[b]);
    if (rc != TEASER_HIP_OK) return rc;
    if (color && color[b] && g.color_type == 0)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "color is asked of a volume without colour" + view_at(b));
    TsdfRayView& d = rec[(size_t)b];
    memset(&d, 0, sizeof(d));
    camera(g, views[b], &d);
    d.tiles_x = (d.width + kTsdfRayTile - 1) / kTsdfRayTile;
    const int64_t tiles = d.width > 0 && d.height > 0 ? (int64_t)d.tiles_x * ((d.height + kTsdfRayTile - 1) / kTsdfRayTile) : 0;
    if (n_blocks + tiles > 2147483647)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "the views of one call need more than 2147483647 blocks" + view_at(b));
    d.blk0 = (int32_t)n_blocks;
    n_blocks += tiles;
  }
  if (hit_counts)
    for (int b = 0; b < n_views; ++b) hit_counts[b] = 0;
  if (n_blocks == 0) return TEASER_HIP_OK;  // no pixel
  const size_t o_maps = round_up(sizeof(int32_t) * (size_t)n_blocks, 256);
  size_t floats = 0;
  for (int b = 0; b < n_views; ++b) {
    TsdfRayView& d = rec[(size_t)b];
    const size_t px = (size_t)d.width * (size_t)d.height;
    const bool want[4] = {depth && depth[b], vertex && vertex[b], normal && normal[b], color && color[b]};
    int64_t* off[4] = {&d.depth_off, &d.vertex_off, &d.normal_off, &d.color_off};
    for (int m = 0; m < 4; ++m) {
      *off[m] = want[m] && px > 0 ? (int64_t)floats : -1;
      if (want[m]) floats += round_up((m == 0 ? 1 : 3) * px, 64);  // a map starts on a 256-byte line
    }
  }
  const size_t o_end = o_maps + sizeof(float) * floats;
  const size_t o_map_in = round_up(sizeof(TsdfRayView) * (size_t)n_views, 256);
  const size_t in_bytes = o_map_in + sizeof(int32_t) * (size_t)n_blocks;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  if (!h->in.ensure(in_bytes) || !h->stage.ensure(in_bytes) || !h->out.ensure(o_end) || !h->back.ensure(o_end))
    return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (TSDF ray cast buffers)");
  char* stage = h->stage.as<char>();
  memset(stage, 0, o_map_in);
  memcpy(stage, rec.data(), sizeof(TsdfRayView) * (size_t)n_views);
  int32_t* map = reinterpret_cast<int32_t*>(stage + o_map_in);
  for (int b = 0; b < n_views; ++b) {
    const int32_t end = b + 1 < n_views ? rec[(size_t)b + 1].blk0 : (int32_t)n_blocks;
    for (int32_t k = rec[(size_t)b].blk0; k < end; ++k) map[k] = b;
  }
  hipStream_t s = h->stream;
  FCHK(h, hipMemcpyAsync(h->in.p, stage, in_bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync (TSDF views)");
  TsdfRayArgs a;
  memset(&a, 0, sizeof(a));
  a.views = h->in.as<TsdfRayView>();
  a.blk_view = reinterpret_cast<const int32_t*>(h->in.as<char>() + o_map_in);
  a.out = reinterpret_cast<float*>(h->out.as<char>() + o_maps);
  a.blk_hits = h->out.as<int32_t>();
  a.L_f = (float)h->vol.length;
  launch_tsdf_raycast(s, g, fields(h), a, (int32_t)n_blocks);
  FCHK(h, hipGetLastError(), "kernel launch (TSDF ray cast)");
  FCHK(h, hipMemcpyAsync(h->back.p, h->out.p, o_end, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (TSDF ray cast)");
  FCHK(h, hipStreamSynchronize(s), "TSDF ray cast");
  const char* back = h->back.as<char>();
  const int32_t* blk_hits = reinterpret_cast<const int32_t*>(back);
  const float* maps = reinterpret_cast<const float*>(back + o_maps);
  for (int b = 0; b < n_views; ++b) {
    const TsdfRayView& d = rec[(size_t)b];
    const size_t px = (size_t)d.width * (size_t)d.height;
    if (px == 0) continue;
    if (d.depth_off >= 0) memcpy(depth[b], maps + d.depth_off, sizeof(float) * px);
    if (d.vertex_off >= 0) memcpy(vertex[b], maps + d.vertex_off, sizeof(float) * 3 * px);
    if (d.normal_off >= 0) memcpy(normal[b], maps + d.normal_off, sizeof(float) * 3 * px);
    if (d.color_off >= 0) memcpy(color[b], maps + d.color_off, sizeof(float) * 3 * px);
    if (hit_counts) {
      const int32_t end = b + 1 < n_views ? rec[(size_t)b + 1].blk0 : (int32_t)n_blocks;
      int64_t sum = 0;
      for (int32_t k = d.blk0; k < end; ++k) sum += blk_hits[k];
      hit_counts[b] = sum;
    }
  }
  return TEASER_HIP_OK;
}

}  // extern "C"
