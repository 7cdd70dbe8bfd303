// teaser/rgbd.h -- depth frames on the MI355X: Open3D's PointCloud::CreateFromDepthImage / CreateFromRGBDImage and, the
// other way, t::geometry::PointCloud::ProjectToDepthImage / ProjectToRGBDImage, FP64, over the C ABI
// (include/teaser_hip.h, "Depth frames", where the contract is written out).  Header-only.
//
// Images come in as teaser::DepthFrame, a view that owns nothing: pointers, formats and row strides in bytes (rows may be
// padded).  Clouds and colours are teaser::Matrix3X as in teaser/icp.h (one point per column), transforms teaser::Matrix4.
// `extrinsic` is world-to-camera as in Open3D; the unprojection inverts it on the host (the C ABI takes the camera pose).
// A teaser::FrameConverter holds one ICP handle and is reusable but not re-entrant.  A failed call throws
// teaser::ICPError, the constructor too when no MI355X is visible (there is no CPU path).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "teaser/icp.h"

namespace teaser {

// Open3D's camera::PinholeCameraIntrinsic.
struct PinholeCameraIntrinsic {
  int width = 0, height = 0;
  double fx = 0, fy = 0, cx = 0, cy = 0;
  PinholeCameraIntrinsic() = default;
  PinholeCameraIntrinsic(int w, int h, double fx_, double fy_, double cx_, double cy_)
      : width(w), height(h), fx(fx_), fy(fy_), cx(cx_), cy(cy_) {}
};

// A depth image and, optionally, the colour image beside it.  Row strides of 0 mean "rows without padding".
struct DepthFrame {
  int width = 0, height = 0;
  const void* depth = nullptr;
  int depth_format = 0;  // 0 uint16, 1 float32
  int64_t depth_row_bytes = 0;
  const void* color = nullptr;
  int color_format = 0;  // 0 none, 1 uint8 x 3 (RGB), 2 float32 x 1, 3 float32 x 3
  int64_t color_row_bytes = 0;

  static DepthFrame U16(const uint16_t* d, int w, int h, int64_t row_bytes = 0) {
    DepthFrame f;
    f.width = w, f.height = h, f.depth = d, f.depth_format = 0, f.depth_row_bytes = row_bytes ? row_bytes : 2 * (int64_t)w;
    return f;
  }
  static DepthFrame F32(const float* d, int w, int h, int64_t row_bytes = 0) {
    DepthFrame f;
    f.width = w, f.height = h, f.depth = d, f.depth_format = 1, f.depth_row_bytes = row_bytes ? row_bytes : 4 * (int64_t)w;
    return f;
  }
  DepthFrame& withRGB8(const uint8_t* c, int64_t row_bytes = 0) { return with(c, 1, 3, row_bytes); }
  DepthFrame& withIntensityF32(const float* c, int64_t row_bytes = 0) { return with(c, 2, 4, row_bytes); }
  DepthFrame& withRGBF32(const float* c, int64_t row_bytes = 0) { return with(c, 3, 12, row_bytes); }

 private:
  DepthFrame& with(const void* c, int format, int pixel_bytes, int64_t row_bytes) {
    color = c, color_format = format, color_row_bytes = row_bytes ? row_bytes : (int64_t)pixel_bytes * width;
    return *this;
  }
};

// The arguments of Open3D's calls beside the images.
struct UnprojectOptions {
  Matrix4 extrinsic = Matrix4::Identity();
  double depth_scale = 1000.0;
  double depth_trunc = 1000.0;
  int stride = 1;
  bool convert_rgb_to_intensity = false;
  bool project_valid_depth_only = true;
  bool with_colors = false;  // needs a colour image
  bool with_pixels = false;
};
struct ProjectOptions {
  Matrix4 extrinsic = Matrix4::Identity();
  double depth_scale = 1000.0;
  double depth_max = 3.0;
  bool with_index = false;
};

// One frame's cloud; colours and pixels (row width + column of every point) where asked for.
struct DepthCloud {
  Matrix3X points;
  Matrix3X colors;
  std::vector<int32_t> pixels;
};
// One cloud's images, dense and row-major: depth (0 where empty), colour (3 floats per pixel) where the cloud has colours,
// index (the point seen in every pixel, -1 where empty) where asked for; n_hit counts the non-empty pixels.
struct DepthImage {
  int width = 0, height = 0;
  std::vector<float> depth, color;
  std::vector<int32_t> index;
  int32_t n_hit = 0;
};

namespace detail {
// The inverse of a 4 x 4 matrix by Gauss-Jordan elimination with partial pivoting; throws for a singular one.
inline Matrix4 inverse4(const Matrix4& m) {
  double a[4][8];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) a[r][c] = m(r, c), a[r][4 + c] = r == c ? 1.0 : 0.0;
  for (int k = 0; k < 4; ++k) {
    int p = k;
    for (int r = k + 1; r < 4; ++r)
      if (std::fabs(a[r][k]) > std::fabs(a[p][k])) p = r;
    if (!(std::fabs(a[p][k]) > 0.0)) throw std::invalid_argument("teaser::FrameConverter: the extrinsic is singular");
    for (int c = 0; c < 8; ++c) std::swap(a[k][c], a[p][c]);
    const double inv = 1.0 / a[k][k];
    for (int c = 0; c < 8; ++c) a[k][c] *= inv;
    for (int r = 0; r < 4; ++r) {
      if (r == k) continue;
      const double f = a[r][k];
      for (int c = 0; c < 8; ++c) a[r][c] -= f * a[k][c];
    }
  }
  Matrix4 out = Matrix4::Identity();
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) out(r, c) = a[r][4 + c];
  return out;
}
inline void row_major(const Matrix4& m, double* out) {
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) out[4 * r + c] = m(r, c);
}
inline Matrix3X first_columns(const Matrix3X& m, int64_t n) {
  Matrix3X out(3, n);
  if (n) std::memcpy(out.data(), m.data(), sizeof(double) * 3 * (size_t)n);
  return out;
}
}  // namespace detail

class FrameConverter {
 public:
  explicit FrameConverter(int device = -1) {
    const int32_t rc = teaser_hip_icp_create(device, &h_);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::FrameConverter: teaser_hip_icp_create failed (status " + std::to_string(rc) +
                             (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)" : ")"));
  }
  ~FrameConverter() { teaser_hip_icp_destroy(h_); }
  FrameConverter(const FrameConverter&) = delete;
  FrameConverter& operator=(const FrameConverter&) = delete;

  // Many frames in one launch sequence; result b is identical to frame b converted alone.
  std::vector<DepthCloud> unprojectBatch(const std::vector<DepthFrame>& frames,
                                         const std::vector<PinholeCameraIntrinsic>& intrinsics,
                                         const std::vector<UnprojectOptions>& options) {
    const size_t b = frames.size();
    if (intrinsics.size() != b || options.size() != b)
      throw std::invalid_argument("teaser::FrameConverter: one entry per frame in every argument");
    std::vector<teaser_icp_frame_c> rec(b);
    std::vector<const void*> pd(b), pc(b);
    std::vector<int32_t> count(b, 0);
    std::vector<DepthCloud> full(b), out(b);
    std::vector<double*> pp(b), pco(b);
    std::vector<int32_t*> ppx(b);
    bool any_colors = false, any_pixels = false;
    for (size_t k = 0; k < b; ++k) {
      const DepthFrame& f = frames[k];
      const UnprojectOptions& o = options[k];
      teaser_icp_frame_c& r = rec[k];
      teaser_hip_icp_frame_default(&r);
      r.width = f.width, r.height = f.height;
      r.depth_format = f.depth_format, r.depth_row_bytes = f.depth_row_bytes;
      r.color_format = f.color_format, r.color_row_bytes = f.color_row_bytes;
      r.intensity = o.convert_rgb_to_intensity && f.color_format == 1 ? 1 : 0;
      r.stride = o.stride, r.valid_only = o.project_valid_depth_only ? 1 : 0;
      r.fx = intrinsics[k].fx, r.fy = intrinsics[k].fy, r.cx = intrinsics[k].cx, r.cy = intrinsics[k].cy;
      detail::row_major(detail::inverse4(o.extrinsic), r.camera_pose);
      r.depth_scale = o.depth_scale, r.depth_trunc = o.depth_trunc;
      if (o.stride < 1) throw std::invalid_argument("teaser::FrameConverter: stride must be >= 1");
      if (f.width < 0 || f.height < 0) throw std::invalid_argument("teaser::FrameConverter: a negative image size");
      const int64_t n_vis = (((int64_t)f.height + o.stride - 1) / o.stride) * (((int64_t)f.width + o.stride - 1) / o.stride);
      pd[k] = f.depth, pc[k] = f.color;
      full[k].points = Matrix3X(3, n_vis);
      pp[k] = n_vis ? full[k].points.data() : nullptr;
      pco[k] = nullptr, ppx[k] = nullptr;
      if (o.with_colors && n_vis) {
        full[k].colors = Matrix3X(3, n_vis);
        pco[k] = full[k].colors.data();
        any_colors = true;
      }
      if (o.with_pixels && n_vis) {
        full[k].pixels.resize((size_t)n_vis);
        ppx[k] = full[k].pixels.data();
        any_pixels = true;
      }
    }
    const int32_t rc = teaser_hip_icp_unproject_depth_batch(h_, (int32_t)b, rec.data(), pd.data(), pc.data(), count.data(),
                                                            pp.data(), any_colors ? pco.data() : nullptr,
                                                            any_pixels ? ppx.data() : nullptr);
    check(rc);
    for (size_t k = 0; k < b; ++k) {
      out[k].points = detail::first_columns(full[k].points, count[k]);
      if (pco[k]) out[k].colors = detail::first_columns(full[k].colors, count[k]);
      if (ppx[k]) out[k].pixels.assign(full[k].pixels.begin(), full[k].pixels.begin() + count[k]);
    }
    return out;
  }

  DepthCloud unproject(const DepthFrame& frame, const PinholeCameraIntrinsic& intrinsic,
                       const UnprojectOptions& options = UnprojectOptions()) {
    return std::move(unprojectBatch({frame}, {intrinsic}, {options})[0]);
  }

  // Many clouds in one launch sequence.  colors: empty, or one matrix per cloud; a cloud whose matrix has as many
  // columns as it has points gets its colour image, one without columns none.  The image sizes are the intrinsics'.
  std::vector<DepthImage> projectBatch(const std::vector<Matrix3X>& clouds, const std::vector<Matrix3X>& colors,
                                       const std::vector<PinholeCameraIntrinsic>& intrinsics,
                                       const std::vector<ProjectOptions>& options) {
    const size_t b = clouds.size();
    if ((!colors.empty() && colors.size() != b) || intrinsics.size() != b || options.size() != b)
      throw std::invalid_argument("teaser::FrameConverter: one entry per cloud in every argument");
    std::vector<teaser_icp_projection_c> cam(b);
    std::vector<const double*> pp(b), pc(b);
    std::vector<int32_t> n(b), hit(b, 0);
    std::vector<DepthImage> out(b);
    std::vector<float*> pd(b), pci(b);
    std::vector<int32_t*> pix(b);
    for (size_t k = 0; k < b; ++k) {
      const PinholeCameraIntrinsic& K = intrinsics[k];
      if (K.width < 0 || K.height < 0) throw std::invalid_argument("teaser::FrameConverter: a negative image size");
      const bool has_color = !colors.empty() && colors[k].cols() != 0;
      if (has_color && colors[k].cols() != clouds[k].cols())
        throw std::invalid_argument("teaser::FrameConverter: as many colours as points");
      std::memset(&cam[k], 0, sizeof(cam[k]));
      cam[k].width = K.width, cam[k].height = K.height;
      cam[k].fx = K.fx, cam[k].fy = K.fy, cam[k].cx = K.cx, cam[k].cy = K.cy;
      detail::row_major(options[k].extrinsic, cam[k].extrinsic);
      cam[k].depth_scale = options[k].depth_scale, cam[k].depth_max = options[k].depth_max;
      const size_t px = K.width <= 16384 && K.height <= 16384 ? (size_t)K.width * (size_t)K.height : 0;
      pp[k] = clouds[k].data(), pc[k] = has_color ? colors[k].data() : nullptr;
      n[k] = (int32_t)clouds[k].cols();
      out[k].width = K.width, out[k].height = K.height;
      out[k].depth.assign(px, 0.0f);
      if (has_color) out[k].color.assign(3 * px, 0.0f);
      if (options[k].with_index) out[k].index.assign(px, -1);
      pd[k] = px ? out[k].depth.data() : nullptr;
      pci[k] = px && has_color ? out[k].color.data() : nullptr;
      pix[k] = px && options[k].with_index ? out[k].index.data() : nullptr;
    }
    check(teaser_hip_icp_project_depth_batch(h_, (int32_t)b, pp.data(), pc.data(), n.data(), cam.data(), pd.data(),
                                             pci.data(), pix.data(), hit.data()));
    for (size_t k = 0; k < b; ++k) out[k].n_hit = hit[k];
    return out;
  }

  DepthImage project(const Matrix3X& cloud, const PinholeCameraIntrinsic& intrinsic,
                     const ProjectOptions& options = ProjectOptions(), const Matrix3X& colors = Matrix3X()) {
    return std::move(projectBatch({cloud}, {colors}, {intrinsic}, {options})[0]);
  }

 private:
  void check(int32_t rc) {
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::FrameConverter: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
  }
  teaser_hip_icp* h_ = nullptr;
};

// Open3D's PointCloud::CreateFromDepthImage(depth, intrinsic, extrinsic, depth_scale, depth_trunc, stride,
// project_valid_depth_only): the points of the valid pixels in row-major order.
inline Matrix3X createPointCloudFromDepthImage(const DepthFrame& depth, const PinholeCameraIntrinsic& intrinsic,
                                               const Matrix4& extrinsic = Matrix4::Identity(), double depth_scale = 1000.0,
                                               double depth_trunc = 1000.0, int stride = 1,
                                               bool project_valid_depth_only = true) {
  UnprojectOptions o;
  o.extrinsic = extrinsic, o.depth_scale = depth_scale, o.depth_trunc = depth_trunc, o.stride = stride;
  o.project_valid_depth_only = project_valid_depth_only;
  DepthFrame d = depth;
  d.color = nullptr, d.color_format = 0;
  FrameConverter c;
  return c.unproject(d, intrinsic, o).points;
}

// Open3D's RGBDImage::CreateFromColorAndDepth(color, depth, depth_scale, depth_trunc, convert_rgb_to_intensity) followed
// by PointCloud::CreateFromRGBDImage: points and colours.
inline DepthCloud createPointCloudFromRGBDImage(const DepthFrame& rgbd, const PinholeCameraIntrinsic& intrinsic,
                                                const Matrix4& extrinsic = Matrix4::Identity(), double depth_scale = 1000.0,
                                                double depth_trunc = 3.0, bool convert_rgb_to_intensity = true,
                                                bool project_valid_depth_only = true) {
  UnprojectOptions o;
  o.extrinsic = extrinsic, o.depth_scale = depth_scale, o.depth_trunc = depth_trunc;
  o.convert_rgb_to_intensity = convert_rgb_to_intensity, o.project_valid_depth_only = project_valid_depth_only;
  o.with_colors = true;
  FrameConverter c;
  return c.unproject(rgbd, intrinsic, o);
}

// Open3D's t::geometry::PointCloud::ProjectToDepthImage(width, height, intrinsic, extrinsic, depth_scale, depth_max); the
// image size is the intrinsic's.
inline DepthImage projectToDepthImage(const Matrix3X& points, const PinholeCameraIntrinsic& intrinsic,
                                      const Matrix4& extrinsic = Matrix4::Identity(), double depth_scale = 1000.0,
                                      double depth_max = 3.0) {
  ProjectOptions o;
  o.extrinsic = extrinsic, o.depth_scale = depth_scale, o.depth_max = depth_max;
  FrameConverter c;
  return c.project(points, intrinsic, o);
}

// Open3D's t::geometry::PointCloud::ProjectToRGBDImage: depth and colour, a pixel's colour being that of the point its
// depth comes from.
inline DepthImage projectToRGBDImage(const Matrix3X& points, const Matrix3X& colors, const PinholeCameraIntrinsic& intrinsic,
                                     const Matrix4& extrinsic = Matrix4::Identity(), double depth_scale = 1000.0,
                                     double depth_max = 3.0) {
  ProjectOptions o;
  o.extrinsic = extrinsic, o.depth_scale = depth_scale, o.depth_max = depth_max;
  FrameConverter c;
  return c.project(points, intrinsic, o, colors);
}

}  // namespace teaser
