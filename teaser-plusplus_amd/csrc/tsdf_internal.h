// tsdf_internal.h -- what the host sides of the TSDF volume share (tsdf.hip: the handle, integration, the point clouds and
// the voxels; tsdf_mesh.hip: the triangle mesh): the handle and the views of its one volume.
#pragma once

#include <vector>

#include "host_common.h"
#include "teaser_hip.h"
#include "tsdf_device.h"

struct teaser_hip_tsdf : thip::HandleBase {
  teaser_tsdf_volume_c vol;
  thip::TsdfGrid g;
  void* volume = nullptr;  // tsdf (n floats), weight (n floats), colour (3 n doubles), exactly sized
  size_t volume_bytes = 0;
  thip::DevBuf in, work, out;
  thip::DevBuf mesh;  // the cube bytes, cube records and column sums of the triangle mesh: allocated by its first call
  thip::HostBuf stage, back;
  ~teaser_hip_tsdf() {
    if (volume) (void)hipFree(volume);
  }
};

namespace thip {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- the frames of an integration call: what the dense and the scalable volume (stsdf.hip) check and pack alike ----
inline std::string frame_at(int b) { return " (frame " + std::to_string(b) + ")"; }

inline int32_t check_frame(HandleBase* h, int color_type, int b, const teaser_tsdf_frame_c& f) {
  if (f.width < 0 || f.height < 0 || f.width > kRgbdMaxSide || f.height > kRgbdMaxSide)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "width and height must lie in [0, 16384]" + frame_at(b));
  if (!std::isfinite(f.fx) || !std::isfinite(f.fy) || f.fx == 0.0 || f.fy == 0.0)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "fx and fy must be finite and not zero" + frame_at(b));
  if (!std::isfinite(f.cx) || !std::isfinite(f.cy))
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "cx and cy must be finite" + frame_at(b));
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(f.extrinsic[k]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "extrinsic has a non-finite entry" + frame_at(b));
  if (!std::isfinite(f.depth_scale) || !(f.depth_scale > 0.0))
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_scale must be finite and > 0" + frame_at(b));
  if (!std::isfinite(f.depth_trunc)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_trunc must be finite" + frame_at(b));
  if (f.depth_format < 0 || f.depth_format > 1)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_format must be 0 (uint16) or 1 (float32)" + frame_at(b));
  if (f.color_format < 0 || f.color_format > 3)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "color_format must lie in [0, 3]" + frame_at(b));
  if (color_type == 1 && f.color_format != 1)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "color_format must be 1 (uint8 x 3) for an RGB8 volume" + frame_at(b));
  if (color_type == 2 && f.color_format != 2)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "color_format must be 2 (float32 x 1) for a Gray32 volume" + frame_at(b));
  return TEASER_HIP_OK;
}

// Checks the frames and builds their records: fd[b], with the offsets at which stage_frames packs the rows of the images
// (without padding, every image 16-byte aligned); *in_bytes is the size of that buffer.
inline int32_t plan_frames(HandleBase* h, const TsdfGrid& g, int32_t n_frames, const teaser_tsdf_frame_c* frames,
                           const void* const* depth, const void* const* color, std::vector<TsdfFrame>& fd,
                           size_t* in_bytes_out) {
  const int color_px = g.color_type == 1 ? 3 : 4;
  fd.resize((size_t)n_frames);
  size_t in_bytes = 0;
  for (int b = 0; b < n_frames; ++b) {
    const teaser_tsdf_frame_c& f = frames[b];
    const int32_t rc = check_frame(h, g.color_type, b, f);
    if (rc != TEASER_HIP_OK) return rc;
    TsdfFrame& d = fd[(size_t)b];
    memset(&d, 0, sizeof(d));
    for (int k = 0; k < 12; ++k) d.E[k] = (float)f.extrinsic[k];
    for (int r = 0; r < 3; ++r) d.s[r] = d.E[4 * r + 2] * g.vl_f;
    d.fx = (float)f.fx, d.fy = (float)f.fy, d.cx = (float)f.cx, d.cy = (float)f.cy;
    d.inv_fx = 1.0f / d.fx, d.inv_fy = 1.0f / d.fy;
    d.safe_w = (float)f.width - 0.0001f, d.safe_h = (float)f.height - 0.0001f;
    d.depth_scale = (float)f.depth_scale, d.depth_trunc = f.depth_trunc;
    d.width = f.width, d.height = f.height, d.depth_format = f.depth_format;
    if (f.width == 0 || f.height == 0) continue;  // no pixel: safe_w or safe_h lets nothing through
    const int64_t depth_row = (int64_t)f.width * rgbd_depth_bytes(f.depth_format);
    if (f.depth_row_bytes < depth_row)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_row_bytes is smaller than a row" + frame_at(b));
    if (!depth || !depth[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth is NULL" + frame_at(b));
    d.depth_off = (int64_t)in_bytes;
    in_bytes = round_up(in_bytes + (size_t)(f.height * depth_row), 16);
    if (g.color_type != 0) {
      if (f.color_row_bytes < (int64_t)f.width * color_px)
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "color_row_bytes is smaller than a row" + frame_at(b));
      if (!color || !color[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "color is NULL" + frame_at(b));
      d.color_off = (int64_t)in_bytes;
      in_bytes = round_up(in_bytes + (size_t)f.height * (size_t)f.width * (size_t)color_px, 16);
    }
  }
  *in_bytes_out = in_bytes;
  return TEASER_HIP_OK;
}

inline void stage_frames(const TsdfGrid& g, int32_t n_frames, const teaser_tsdf_frame_c* frames, const void* const* depth,
                         const void* const* color, const std::vector<TsdfFrame>& fd, unsigned char* stage) {
  const int color_px = g.color_type == 1 ? 3 : 4;
  for (int b = 0; b < n_frames; ++b) {
    const teaser_tsdf_frame_c& f = frames[b];
    const TsdfFrame& d = fd[(size_t)b];
    if (f.width == 0 || f.height == 0) continue;
    const size_t depth_row = (size_t)f.width * (size_t)rgbd_depth_bytes(f.depth_format);
    const size_t color_row = (size_t)f.width * (size_t)color_px;
    for (int64_t r = 0; r < f.height; ++r) {
      memcpy(stage + d.depth_off + r * (int64_t)depth_row, (const unsigned char*)depth[b] + r * f.depth_row_bytes, depth_row);
      if (g.color_type != 0)
        memcpy(stage + d.color_off + r * (int64_t)color_row, (const unsigned char*)color[b] + r * f.color_row_bytes, color_row);
    }
  }
}

inline int64_t voxels(const teaser_hip_tsdf* h) { return (int64_t)h->g.R * h->g.R * h->g.R; }

inline TsdfFields fields(const teaser_hip_tsdf* h) {
  const int64_t n = voxels(h);
  char* p = static_cast<char*>(h->volume);
  TsdfFields v;
  v.tsdf = reinterpret_cast<float*>(p);
  v.weight = reinterpret_cast<float*>(p + 4 * (size_t)n);
  v.color = h->g.color_type != 0 ? reinterpret_cast<double*>(p + 8 * (size_t)n) : nullptr;
  v.n = n;
  return v;
}

}  // namespace thip
