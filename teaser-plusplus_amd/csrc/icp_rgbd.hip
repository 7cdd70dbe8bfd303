// icp_rgbd.hip -- host side of the depth-frame calls on the ICP handle (include/teaser_hip.h, "Depth frames"): frames to
// clouds (teaser_hip_icp_unproject_depth_batch) and clouds to frames (teaser_hip_icp_project_depth_batch).  Kernels:
// kernels_rgbd.hip; device code: icp_rgbd_device.h; design, bytes moved, launch counts and the resource report: DESIGN.md
// section 31.
//
// Unprojection: the visited rows of every depth image (and of the colour images that are asked for) are packed without
// padding into one staging array and uploaded in one copy; three launches over the tiles of all frames; counts, points,
// colours and pixel indices come back in the one copy of B_X.  Projection: points and colours are packed as in every
// cloud call; the key image is filled with ones, then the scatter and the resolve; counters and images come back in the
// one copy of B_X.  Neither the launches nor the synchronisation depend on the data or the batch.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_common.h"
#include "icp_host.h"
#include "icp_internal.h"
#include "icp_rgbd_device.h"
#include "teaser_hip.h"

using namespace thip;

namespace {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// What both records hold alike: the image size, the intrinsics, the matrix and the depth scale; `what` names the
// second depth parameter (depth_trunc or depth_max), `mat` the matrix.
int32_t check_camera(teaser_hip_icp* h, int b, int32_t width, int32_t height, double fx, double fy, double cx, double cy,
                     const double* m, const char* mat, double depth_scale, double second, const char* what) {
  if (width < 0 || height < 0 || width > kRgbdMaxSide || height > kRgbdMaxSide)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "width and height must lie in [0, 16384]" + at(b));
  if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.0 || fy == 0.0)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "fx and fy must be finite and not zero" + at(b));
  if (!std::isfinite(cx) || !std::isfinite(cy)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "cx and cy must be finite" + at(b));
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(m[k])) return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string(mat) + " has a non-finite entry" + at(b));
  if (!std::isfinite(depth_scale) || !(depth_scale > 0.0))
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_scale must be finite and > 0" + at(b));
  if (!std::isfinite(second)) return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string(what) + " must be finite" + at(b));
  return TEASER_HIP_OK;
}

}  // namespace

extern "C" {

int32_t teaser_hip_icp_frame_default(teaser_icp_frame_c* f) {
  if (!f) return TEASER_HIP_ERR_BAD_ARG;
  memset(f, 0, sizeof(*f));
  f->stride = 1;
  f->valid_only = 1;
  for (int k = 0; k < 4; ++k) f->camera_pose[5 * k] = 1.0;
  f->depth_scale = 1000.0;
  f->depth_trunc = 1000.0;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_icp_unproject_depth_batch(teaser_hip_icp* h, int32_t batch, const teaser_icp_frame_c* frames,
                                             const void* const* depth, const void* const* color, int32_t* count_out,
                                             double* const* points_out, double* const* colors_out,
                                             int32_t* const* pixel_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (batch < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0");
  if (batch == 0) return TEASER_HIP_OK;
  if (!frames) return fail(h, TEASER_HIP_ERR_BAD_ARG, "frames must not be NULL");
  if (!count_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "count_out must not be NULL");
  int32_t rc = TEASER_HIP_OK;
  std::vector<IcpFrameDesc> fd((size_t)batch);
  int64_t total_vis = 0, total_col = 0, total_pix = 0, n_tiles = 0;
  size_t in_bytes = 0;
  for (int b = 0; b < batch; ++b) {
    const teaser_icp_frame_c& f = frames[b];
    if ((rc = check_camera(h, b, f.width, f.height, f.fx, f.fy, f.cx, f.cy, f.camera_pose, "camera_pose", f.depth_scale,
                           f.depth_trunc, "depth_trunc")) != TEASER_HIP_OK)
      return rc;
    if (f.depth_format < 0 || f.depth_format > 1)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_format must be 0 (uint16) or 1 (float32)" + at(b));
    if (f.color_format < 0 || f.color_format > 3)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "color_format must lie in [0, 3]" + at(b));
    if (f.intensity < 0 || f.intensity > 1 || (f.intensity == 1 && f.color_format != 1))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "intensity must be 0, or 1 with color_format 1" + at(b));
    if (f.valid_only < 0 || f.valid_only > 1) return fail(h, TEASER_HIP_ERR_BAD_ARG, "valid_only must be 0 or 1" + at(b));
    if (f.reserved != 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "reserved must be 0" + at(b));
    if (f.stride < 1) return fail(h, TEASER_HIP_ERR_BAD_ARG, "stride must be >= 1" + at(b));
    const bool want_color = colors_out && colors_out[b];
    if (want_color && f.color_format == 0)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "colors_out is given for a frame without colour" + at(b));
    IcpFrameDesc& d = fd[(size_t)b];
    memset(&d, 0, sizeof(d));
    const int64_t rows = ((int64_t)f.height + f.stride - 1) / f.stride, nj = ((int64_t)f.width + f.stride - 1) / f.stride;
    const int64_t n_vis = rows * nj;
    d.width = f.width, d.height = f.height, d.stride = f.stride;
    d.depth_format = f.depth_format, d.color_format = f.color_format, d.intensity = f.intensity;
    d.valid_only = f.valid_only;
    d.nj = (int32_t)nj, d.n_vis = (int32_t)n_vis;
    d.tile_off = (int32_t)n_tiles, d.n_tiles = (int32_t)((n_vis + kRgbdTile - 1) / kRgbdTile);
    d.point_off = total_vis, d.color_out = -1, d.pixel_out = -1;
    d.fx = f.fx, d.fy = f.fy, d.cx = f.cx, d.cy = f.cy;
    memcpy(d.pose, f.camera_pose, sizeof(d.pose));
    d.depth_trunc = f.depth_trunc, d.depth_scale = (float)f.depth_scale;
    if (n_vis == 0) continue;
    const int64_t depth_row = (int64_t)f.width * rgbd_depth_bytes(f.depth_format);
    if (f.depth_row_bytes < depth_row)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_row_bytes is smaller than a row" + at(b));
    if (!depth || !depth[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth is NULL" + at(b));
    if (!points_out || !points_out[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "points_out is NULL" + at(b));
    d.depth_off = (int64_t)in_bytes;
    in_bytes = round_up(in_bytes + (size_t)(rows * depth_row), 16);
    if (f.color_format != 0) {
      const int64_t color_row = (int64_t)f.width * rgbd_color_bytes(f.color_format);
      if (f.color_row_bytes < color_row)
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "color_row_bytes is smaller than a row" + at(b));
      if (!color || !color[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "color is NULL" + at(b));
      if (want_color) {  // a colour image nobody asks for is not uploaded
        d.color_off = (int64_t)in_bytes;
        in_bytes = round_up(in_bytes + (size_t)(rows * color_row), 16);
        d.color_out = total_col;
        total_col += n_vis;
      }
    }
    if (pixel_out && pixel_out[b]) {
      d.pixel_out = total_pix;
      total_pix += n_vis;
    }
    total_vis += n_vis;
    n_tiles += d.n_tiles;
    if (total_vis > INT32_MAX) return fail(h, TEASER_HIP_ERR_BAD_ARG, "more than 2^31 - 1 visited pixels in one call");
  }
  for (int b = 0; b < batch; ++b) count_out[b] = 0;
  if (total_vis == 0) return TEASER_HIP_OK;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");

  // the visited rows, packed, and the frame of every tile
  h->stage.resize((in_bytes + 7) / 8);
  unsigned char* in = (unsigned char*)h->stage.data();
  std::vector<int32_t> tile_frame((size_t)n_tiles);
  for (int b = 0; b < batch; ++b) {
    const IcpFrameDesc& d = fd[(size_t)b];
    if (d.n_vis == 0) continue;
    const teaser_icp_frame_c& f = frames[b];
    const int64_t rows = d.n_vis / d.nj;
    const size_t depth_row = (size_t)d.width * (size_t)rgbd_depth_bytes(d.depth_format);
    const size_t color_row = (size_t)d.width * (size_t)rgbd_color_bytes(d.color_format);
    for (int64_t r = 0; r < rows; ++r) {
      memcpy(in + d.depth_off + r * (int64_t)depth_row,
             (const unsigned char*)depth[b] + r * d.stride * f.depth_row_bytes, depth_row);
      if (d.color_out >= 0)
        memcpy(in + d.color_off + r * (int64_t)color_row,
               (const unsigned char*)color[b] + r * d.stride * f.color_row_bytes, color_row);
    }
    std::fill(tile_frame.begin() + d.tile_off, tile_frame.begin() + d.tile_off + d.n_tiles, b);
  }

  // B_X: the frames' counts, the points, the colours, the pixel indices
  const size_t o_pts = round_up(sizeof(int32_t) * (size_t)batch, 8), o_col = o_pts + 24 * (size_t)total_vis;
  const size_t o_pix = o_col + 24 * (size_t)total_col, o_end = o_pix + sizeof(int32_t) * (size_t)total_pix;
  size_t bytes[B_COUNT] = {};
  bytes[B_RGBD_DESC] = sizeof(IcpFrameDesc) * (size_t)batch;
  bytes[B_BLK] = sizeof(int32_t) * (size_t)n_tiles;
  bytes[B_RGBD_IN] = in_bytes;
  bytes[B_RGBD_WORK] = sizeof(int32_t) * 2 * (size_t)n_tiles;
  bytes[B_X] = o_end;
  if ((rc = ensure_buffers(h, bytes, "hipMalloc failed (depth-frame buffers)")) != TEASER_HIP_OK) return rc;
  DevBuf* B = h->buf;
  hipStream_t s = h->stream;
  FCHK(h, hipMemcpyAsync(B[B_RGBD_DESC].p, fd.data(), bytes[B_RGBD_DESC], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (inputs)");
  FCHK(h, hipMemcpyAsync(B[B_BLK].p, tile_frame.data(), bytes[B_BLK], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (inputs)");
  FCHK(h, hipMemcpyAsync(B[B_RGBD_IN].p, in, in_bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync (images)");
  char* out = B[B_X].as<char>();
  int32_t* work = B[B_RGBD_WORK].as<int32_t>();
  launch_icp_rgbd_unproject(s, B[B_RGBD_DESC].as<IcpFrameDesc>(), B[B_BLK].as<int32_t>(), (int)n_tiles, batch,
                            B[B_RGBD_IN].as<unsigned char>(), work, work + n_tiles, (int32_t*)out,
                            (double*)(out + o_pts), (double*)(out + o_col), (int32_t*)(out + o_pix));
  if ((rc = copy_back(h, 0, o_end, "depth frames", "kernel launch (depth frames)")) != TEASER_HIP_OK) return rc;
  const char* back = (const char*)h->back.data();
  for (int b = 0; b < batch; ++b) {
    const IcpFrameDesc& d = fd[(size_t)b];
    if (d.n_vis == 0) continue;
    int32_t cnt = 0;
    memcpy(&cnt, back + sizeof(int32_t) * (size_t)b, sizeof(int32_t));
    count_out[b] = cnt;
    memcpy(points_out[b], back + o_pts + 24 * (size_t)d.point_off, 24 * (size_t)cnt);
    if (d.color_out >= 0) memcpy(colors_out[b], back + o_col + 24 * (size_t)d.color_out, 24 * (size_t)cnt);
    if (d.pixel_out >= 0) memcpy(pixel_out[b], back + o_pix + sizeof(int32_t) * (size_t)d.pixel_out, sizeof(int32_t) * (size_t)cnt);
  }
  return TEASER_HIP_OK;
}

int32_t teaser_hip_icp_project_depth_batch(teaser_hip_icp* h, int32_t batch, const double* const* points,
                                           const double* const* colors, const int32_t* n,
                                           const teaser_icp_projection_c* cameras, float* const* depth_out,
                                           float* const* color_out, int32_t* const* index_out, int32_t* n_hit_out) {
  const CallStart c = begin_cloud_call(h, batch, points, n, false);
  if (c.done) return c.rc;
  if (!cameras) return fail(h, TEASER_HIP_ERR_BAD_ARG, "cameras must not be NULL");
  if (!n_hit_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_hit_out must not be NULL");
  int32_t rc = TEASER_HIP_OK;
  std::vector<IcpProjDesc> pd((size_t)batch);
  int64_t p_off = 0, total_px = 0, total_col = 0, total_idx = 0, n_blk = 0, n_tiles = 0;
  bool any_color = false;
  for (int b = 0; b < batch; ++b) {
    const teaser_icp_projection_c& cam = cameras[b];
    if ((rc = check_camera(h, b, cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, cam.extrinsic, "extrinsic",
                           cam.depth_scale, cam.depth_max, "depth_max")) != TEASER_HIP_OK)
      return rc;
    const bool has_color = colors && colors[b];
    if (has_color && n[b] > 0 && !finite_points(colors[b], n[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "colors has a non-finite component" + at(b));
    const bool want_color = color_out && color_out[b];
    if (want_color && !has_color)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "color_out is given for a problem without colours" + at(b));
    const int64_t px = (int64_t)cam.width * cam.height;
    if (px > 0 && (!depth_out || !depth_out[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_out is NULL" + at(b));
    IcpProjDesc& d = pd[(size_t)b];
    memset(&d, 0, sizeof(d));
    d.width = cam.width, d.height = cam.height;
    d.n = px > 0 ? n[b] : 0;  // an image without pixels takes no point
    d.has_color = want_color && px > 0 ? 1 : 0;
    d.blk_off = (int32_t)n_blk, d.tile_off = (int32_t)n_tiles;
    d.p_off = p_off, d.img_off = total_px, d.color_out = -1, d.index_out = -1;
    d.fx = cam.fx, d.fy = cam.fy, d.cx = cam.cx, d.cy = cam.cy;
    memcpy(d.ext, cam.extrinsic, sizeof(d.ext));
    d.depth_scale = cam.depth_scale, d.depth_max = cam.depth_max;
    p_off += n[b];
    if (px == 0) continue;
    if (d.has_color) {
      d.color_out = total_col;
      total_col += px;
      any_color = true;
    }
    if (index_out && index_out[b]) {
      d.index_out = total_idx;
      total_idx += px;
    }
    total_px += px;
    n_blk += (d.n + kRgbdTile - 1) / kRgbdTile;
    n_tiles += (px + kRgbdTile - 1) / kRgbdTile;
    if (total_px > INT32_MAX) return fail(h, TEASER_HIP_ERR_BAD_ARG, "more than 2^31 - 1 pixels in one call");
  }
  for (int b = 0; b < batch; ++b) n_hit_out[b] = 0;
  if (total_px == 0) return TEASER_HIP_OK;
  if (n_blk == 0) {  // no point anywhere: the empty images, without the device
    for (int b = 0; b < batch; ++b) {
      const IcpProjDesc& d = pd[(size_t)b];
      const size_t px = (size_t)d.width * (size_t)d.height;
      if (px == 0) continue;
      std::fill(depth_out[b], depth_out[b] + px, 0.0f);
      if (d.color_out >= 0) std::fill(color_out[b], color_out[b] + 3 * px, 0.0f);
      if (d.index_out >= 0) std::fill(index_out[b], index_out[b] + px, -1);
    }
    return TEASER_HIP_OK;
  }
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");

  std::vector<int32_t> blk_prob((size_t)n_blk), tile_prob((size_t)n_tiles);
  for (int b = 0; b < batch; ++b) {
    const IcpProjDesc& d = pd[(size_t)b];
    const int64_t px = (int64_t)d.width * d.height;
    std::fill(blk_prob.begin() + d.blk_off, blk_prob.begin() + d.blk_off + (d.n + kRgbdTile - 1) / kRgbdTile, b);
    std::fill(tile_prob.begin() + d.tile_off, tile_prob.begin() + d.tile_off + (px + kRgbdTile - 1) / kRgbdTile, b);
  }

  // B_X: the hit counters, the depth images, the index images, the colour images
  const size_t total = (size_t)c.total;
  const size_t o_depth = round_up(sizeof(int32_t) * (size_t)batch, 8), o_idx = o_depth + sizeof(float) * (size_t)total_px;
  const size_t o_col = o_idx + sizeof(int32_t) * (size_t)total_idx, o_end = o_col + 3 * sizeof(float) * (size_t)total_col;
  size_t bytes[B_COUNT] = {};
  bytes[B_RGBD_DESC] = sizeof(IcpProjDesc) * (size_t)batch;
  bytes[B_BLK] = sizeof(int32_t) * (size_t)n_blk;
  bytes[B_TBLK] = sizeof(int32_t) * (size_t)n_tiles;
  bytes[B_Q] = sizeof(double) * 3 * total;
  bytes[B_RGBD_IN] = any_color ? sizeof(double) * 3 * total : 0;
  bytes[B_RGBD_WORK] = sizeof(uint64_t) * (size_t)total_px;
  bytes[B_X] = o_end;
  if ((rc = ensure_buffers(h, bytes, "hipMalloc failed (depth-frame buffers)")) != TEASER_HIP_OK) return rc;
  DevBuf* B = h->buf;
  hipStream_t s = h->stream;
  h->stage.resize(3 * total);
  if ((rc = upload_points(h, batch, points, n, 0, "hipMemcpyAsync (points)")) != TEASER_HIP_OK) return rc;
  if (any_color) {  // the rows of the problems whose colour image is not asked for are never read
    h->cstage.assign(3 * total, 0.0);
    for (int b = 0; b < batch; ++b)
      if (pd[(size_t)b].has_color && n[b] > 0)
        memcpy(&h->cstage[(size_t)(3 * pd[(size_t)b].p_off)], colors[b], 24 * (size_t)n[b]);
    FCHK(h, hipMemcpyAsync(B[B_RGBD_IN].p, h->cstage.data(), bytes[B_RGBD_IN], hipMemcpyHostToDevice, s),
         "hipMemcpyAsync (colours)");
  }
  FCHK(h, hipMemcpyAsync(B[B_RGBD_DESC].p, pd.data(), bytes[B_RGBD_DESC], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (inputs)");
  FCHK(h, hipMemcpyAsync(B[B_BLK].p, blk_prob.data(), bytes[B_BLK], hipMemcpyHostToDevice, s), "hipMemcpyAsync (inputs)");
  FCHK(h, hipMemcpyAsync(B[B_TBLK].p, tile_prob.data(), bytes[B_TBLK], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (inputs)");
  char* out = B[B_X].as<char>();
  FCHK(h, hipMemsetAsync(out, 0, o_depth, s), "hipMemsetAsync");
  FCHK(h, hipMemsetAsync(B[B_RGBD_WORK].p, 0xFF, bytes[B_RGBD_WORK], s), "hipMemsetAsync (key image)");
  launch_icp_rgbd_project(s, B[B_RGBD_DESC].as<IcpProjDesc>(), B[B_BLK].as<int32_t>(), (int)n_blk,
                          B[B_TBLK].as<int32_t>(), (int)n_tiles, B[B_Q].as<double>(), B[B_RGBD_IN].as<double>(),
                          B[B_RGBD_WORK].as<uint64_t>(), (float*)(out + o_depth), (float*)(out + o_col),
                          (int32_t*)(out + o_idx), (int32_t*)out);
  if ((rc = copy_back(h, 0, o_end, "depth projection", "kernel launch (depth projection)")) != TEASER_HIP_OK) return rc;
  const char* back = (const char*)h->back.data();
  memcpy(n_hit_out, back, sizeof(int32_t) * (size_t)batch);
  for (int b = 0; b < batch; ++b) {
    const IcpProjDesc& d = pd[(size_t)b];
    const size_t px = (size_t)d.width * (size_t)d.height;
    if (px == 0) continue;
    memcpy(depth_out[b], back + o_depth + sizeof(float) * (size_t)d.img_off, sizeof(float) * px);
    if (d.index_out >= 0) memcpy(index_out[b], back + o_idx + sizeof(int32_t) * (size_t)d.index_out, sizeof(int32_t) * px);
    if (d.color_out >= 0) memcpy(color_out[b], back + o_col + 3 * sizeof(float) * (size_t)d.color_out, 3 * sizeof(float) * px);
  }
  return TEASER_HIP_OK;
}

}  // extern "C"
