// teaser/odometry.h -- RGB-D odometry with the surface of Open3D's pipelines::odometry on the MI355X: the motion between
// two RGB-D frames (source to target) and its 6 x 6 information matrix, which is what teaser::PoseGraphEdge and
// teaser::UniformTSDFVolume::integrate take.
//
//   teaser::RGBDOdometryResult r = teaser::computeRGBDOdometry(source, target, intrinsic);   // r.success, r.transformation
//   teaser::RGBDOdometry odo;  auto rs = odo.computeBatch(sources, targets, {intrinsic});    // every pair in ONE launch sequence
//
// Frames are teaser::DepthFrame views (teaser/rgbd.h) with a colour image beside the depth: uint8 x 3 (RGB) or a
// float32 intensity; source and target of a pair agree in size and formats.  The arithmetic is written out in
// include/teaser_hip.h ("RGB-D odometry"): a pair's result is the same alone and at any position of any batch; bit parity
// with an Open3D binary is not claimed.  Errors are teaser::ICPError with the library's status and message; without an
// MI355X the constructor throws (status 3): there is no CPU path.
#pragma once

#include <string>
#include <vector>

#include "teaser/rgbd.h"
#include "teaser/tsdf.h"

namespace teaser {

enum class RGBDOdometryJacobian { ColorTerm = 0, HybridTerm = 1 };

// Open3D's OdometryOption; iteration_number_per_pyramid_level[0] belongs to the COARSEST level.
struct OdometryOption {
  std::vector<int> iteration_number_per_pyramid_level = {20, 10, 5};
  double depth_diff_max = 0.03;
  double depth_min = 0.0;
  double depth_max = 4.0;
  // the conversion of uint16 depth (Open3D's RGBDImage::CreateFromColorAndDepth)
  double depth_scale = 1000.0;
  double depth_trunc = 3.0;
};

struct RGBDOdometryResult {
  bool success = false;
  Matrix4 transformation = Matrix4::Identity();
  Matrix6 information = Matrix6::Zero();
  int count = 0;       // correspondences at the final pose
  int iterations = 0;  // iterations executed
};

class RGBDOdometry {
 public:
  explicit RGBDOdometry(int device = -1) {
    const int32_t rc = teaser_hip_icp_create(device, &h_);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::RGBDOdometry: teaser_hip_icp_create failed (status " + std::to_string(rc) +
                             (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)" : ")"));
  }
  ~RGBDOdometry() { teaser_hip_icp_destroy(h_); }
  RGBDOdometry(const RGBDOdometry&) = delete;
  RGBDOdometry& operator=(const RGBDOdometry&) = delete;

  // Pair b = (sources[b], targets[b]).  intrinsics, odo_init: one for all pairs or one per pair (odo_init may be empty:
  // the identity).  Result b is identical to pair b computed alone.
  std::vector<RGBDOdometryResult> computeBatch(const std::vector<DepthFrame>& sources, const std::vector<DepthFrame>& targets,
                                               const std::vector<PinholeCameraIntrinsic>& intrinsics,
                                               const std::vector<Matrix4>& odo_init = {},
                                               RGBDOdometryJacobian jacobian = RGBDOdometryJacobian::HybridTerm,
                                               const OdometryOption& option = OdometryOption()) {
    const size_t b = sources.size();
    if (targets.size() != b) throw std::invalid_argument("teaser::RGBDOdometry: one target per source");
    if (intrinsics.size() != b && intrinsics.size() != 1)
      throw std::invalid_argument("teaser::RGBDOdometry: one intrinsic for all pairs or one per pair");
    if (!odo_init.empty() && odo_init.size() != b && odo_init.size() != 1)
      throw std::invalid_argument("teaser::RGBDOdometry: no odo_init, one for all pairs or one per pair");
    if (option.iteration_number_per_pyramid_level.empty() ||
        option.iteration_number_per_pyramid_level.size() > TEASER_HIP_ODOMETRY_MAX_LEVELS)
      throw std::invalid_argument("teaser::RGBDOdometry: iteration_number_per_pyramid_level must have 1 to 8 entries");
    teaser_icp_odometry_option_c opt;
    teaser_hip_icp_odometry_option_default(&opt);
    opt.n_levels = (int32_t)option.iteration_number_per_pyramid_level.size();
    for (int k = 0; k < 8; ++k) opt.iterations[k] = k < opt.n_levels ? option.iteration_number_per_pyramid_level[(size_t)k] : 0;
    opt.depth_diff_max = option.depth_diff_max, opt.depth_min = option.depth_min, opt.depth_max = option.depth_max;
    std::vector<RGBDOdometryResult> out(b);
    if (b == 0) return out;
    std::vector<teaser_icp_odometry_pair_c> pairs(b);
    std::vector<const void*> ptr[4];
    for (size_t k = 0; k < b; ++k) {
      const DepthFrame &s = sources[k], &t = targets[k];
      if (s.depth_format != t.depth_format || s.color_format != t.color_format)
        throw std::invalid_argument("teaser::RGBDOdometry: source and target differ in format (pair " + std::to_string(k) + ")");
      const PinholeCameraIntrinsic& K = intrinsics[intrinsics.size() == 1 ? 0 : k];
      teaser_icp_odometry_pair_c& p = pairs[k];
      std::memset(&p, 0, sizeof(p));
      p.width = s.width, p.height = s.height, p.target_width = t.width, p.target_height = t.height;
      p.depth_format = s.depth_format, p.color_format = s.color_format, p.jacobian = (int32_t)jacobian;
      p.source_depth_row_bytes = s.depth_row_bytes, p.source_color_row_bytes = s.color_row_bytes;
      p.target_depth_row_bytes = t.depth_row_bytes, p.target_color_row_bytes = t.color_row_bytes;
      p.fx = K.fx, p.fy = K.fy, p.cx = K.cx, p.cy = K.cy;
      detail::row_major(odo_init.empty() ? Matrix4::Identity() : odo_init[odo_init.size() == 1 ? 0 : k], p.odo_init);
      p.depth_scale = option.depth_scale, p.depth_trunc = option.depth_trunc;
      ptr[0].push_back(s.depth), ptr[1].push_back(s.color), ptr[2].push_back(t.depth), ptr[3].push_back(t.color);
    }
    std::vector<teaser_icp_odometry_result_c> res(b);
    const int32_t rc = teaser_hip_icp_rgbd_odometry_batch(h_, (int32_t)b, pairs.data(), &opt, ptr[0].data(), ptr[1].data(),
                                                          ptr[2].data(), ptr[3].data(), res.data(), nullptr);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::RGBDOdometry: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
    for (size_t k = 0; k < b; ++k) {
      out[k].success = res[k].success != 0, out[k].count = res[k].count, out[k].iterations = res[k].iterations;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) out[k].transformation(r, c) = res[k].transformation[4 * r + c];
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) out[k].information(r, c) = res[k].information[6 * r + c];
    }
    return out;
  }

  RGBDOdometryResult compute(const DepthFrame& source, const DepthFrame& target, const PinholeCameraIntrinsic& intrinsic,
                             const Matrix4& odo_init = Matrix4::Identity(),
                             RGBDOdometryJacobian jacobian = RGBDOdometryJacobian::HybridTerm,
                             const OdometryOption& option = OdometryOption()) {
    return computeBatch({source}, {target}, {intrinsic}, {odo_init}, jacobian, option)[0];
  }

 private:
  teaser_hip_icp* h_ = nullptr;
};

// Open3D's ComputeRGBDOdometry(source, target, intrinsic, odo_init, jacobian, option) on a handle of its own; keep a
// teaser::RGBDOdometry for more than one call.
inline RGBDOdometryResult computeRGBDOdometry(const DepthFrame& source, const DepthFrame& target,
                                              const PinholeCameraIntrinsic& intrinsic,
                                              const Matrix4& odo_init = Matrix4::Identity(),
                                              RGBDOdometryJacobian jacobian = RGBDOdometryJacobian::HybridTerm,
                                              const OdometryOption& option = OdometryOption()) {
  RGBDOdometry odo;
  return odo.compute(source, target, intrinsic, odo_init, jacobian, option);
}

// ---- depth odometry (include/teaser_hip.h, "Depth odometry") ----------------------------------------------------------
// Point-to-plane odometry on DEPTH frames alone (Open3D's t::pipelines::odometry::RGBDOdometryMultiScale with
// Method::PointToPlane) and frame-to-model tracking against a TSDF volume of either class:
//
//   teaser::DepthOdometryResult r = teaser::computeDepthOdometry(source, target, intrinsic);
//   teaser::Matrix4 pose = teaser::trackFrameToModel(volume, frame, intrinsic, camera_to_world_init).camera_to_world;
//
// Frames are teaser::DepthFrame views whose colour, if any, is not read.

// iterations[0] belongs to the COARSEST level; the other fields are Open3D's OdometryConvergenceCriteria and
// OdometryLossParams as depth odometry reads them.
struct DepthOdometryOption {
  std::vector<int> iterations = {10, 5, 3};
  double relative_rmse = 1e-6, relative_fitness = 1e-6;
  double depth_outlier_trunc = 0.07, depth_huber_delta = 0.05;
  double depth_scale = 1000.0;  // uint16 depth
  double depth_min = 0.0, depth_max = 3.0;
};

struct DepthOdometryResult {
  bool success = false;
  Matrix4 transformation = Matrix4::Identity();
  Matrix6 information = Matrix6::Zero();
  double fitness = 0.0, inlier_rmse = 0.0;  // of the last executed iteration
  int count = 0;                            // correspondences of the last executed iteration
  int iterations = 0;                       // iterations executed
  int converged_levels = 0;                 // bit l: level l converged
};

class DepthOdometry {
 public:
  explicit DepthOdometry(int device = -1) {
    const int32_t rc = teaser_hip_icp_create(device, &h_);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::DepthOdometry: teaser_hip_icp_create failed (status " + std::to_string(rc) +
                             (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)" : ")"));
  }
  ~DepthOdometry() { teaser_hip_icp_destroy(h_); }
  DepthOdometry(const DepthOdometry&) = delete;
  DepthOdometry& operator=(const DepthOdometry&) = delete;

  // Pair b = (sources[b], targets[b]).  intrinsics, init: one for all pairs or one per pair (init may be empty: the
  // identity).  Result b is identical to pair b computed alone.
  std::vector<DepthOdometryResult> computeBatch(const std::vector<DepthFrame>& sources, const std::vector<DepthFrame>& targets,
                                                const std::vector<PinholeCameraIntrinsic>& intrinsics,
                                                const std::vector<Matrix4>& init = {},
                                                const DepthOdometryOption& option = DepthOdometryOption()) {
    const size_t b = sources.size();
    if (targets.size() != b) throw std::invalid_argument("teaser::DepthOdometry: one target per source");
    if (intrinsics.size() != b && intrinsics.size() != 1)
      throw std::invalid_argument("teaser::DepthOdometry: one intrinsic for all pairs or one per pair");
    if (!init.empty() && init.size() != b && init.size() != 1)
      throw std::invalid_argument("teaser::DepthOdometry: no init, one for all pairs or one per pair");
    if (option.iterations.empty() || option.iterations.size() > TEASER_HIP_ODOMETRY_MAX_LEVELS)
      throw std::invalid_argument("teaser::DepthOdometry: iterations must have 1 to 8 entries");
    teaser_icp_depth_odometry_option_c opt;
    teaser_hip_icp_depth_odometry_option_default(&opt);
    opt.n_levels = (int32_t)option.iterations.size();
    for (int k = 0; k < 8; ++k) opt.iterations[k] = k < opt.n_levels ? option.iterations[(size_t)k] : 0;
    opt.depth_outlier_trunc = option.depth_outlier_trunc, opt.depth_huber_delta = option.depth_huber_delta;
    opt.depth_min = option.depth_min, opt.depth_max = option.depth_max;
    opt.relative_rmse = option.relative_rmse, opt.relative_fitness = option.relative_fitness;
    std::vector<DepthOdometryResult> out(b);
    if (b == 0) return out;
    std::vector<teaser_icp_depth_odometry_pair_c> pairs(b);
    std::vector<const void*> ptr[2];
    for (size_t k = 0; k < b; ++k) {
      const DepthFrame &s = sources[k], &t = targets[k];
      if (s.depth_format != t.depth_format || s.width != t.width || s.height != t.height)
        throw std::invalid_argument("teaser::DepthOdometry: source and target differ in size or format (pair " + std::to_string(k) + ")");
      const PinholeCameraIntrinsic& K = intrinsics[intrinsics.size() == 1 ? 0 : k];
      teaser_icp_depth_odometry_pair_c& p = pairs[k];
      std::memset(&p, 0, sizeof(p));
      p.width = s.width, p.height = s.height, p.depth_format = s.depth_format;
      p.source_depth_row_bytes = s.depth_row_bytes, p.target_depth_row_bytes = t.depth_row_bytes;
      p.fx = K.fx, p.fy = K.fy, p.cx = K.cx, p.cy = K.cy;
      detail::row_major(init.empty() ? Matrix4::Identity() : init[init.size() == 1 ? 0 : k], p.init);
      p.depth_scale = option.depth_scale;
      ptr[0].push_back(s.depth), ptr[1].push_back(t.depth);
    }
    std::vector<teaser_icp_depth_odometry_result_c> res(b);
    const int32_t rc = teaser_hip_icp_depth_odometry_pairs(h_, (int32_t)b, pairs.data(), &opt, ptr[0].data(), ptr[1].data(), res.data(), nullptr);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::DepthOdometry: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
    for (size_t k = 0; k < b; ++k) {
      out[k].success = res[k].success != 0, out[k].count = res[k].count, out[k].iterations = res[k].iterations;
      out[k].converged_levels = res[k].converged_levels, out[k].fitness = res[k].fitness, out[k].inlier_rmse = res[k].inlier_rmse;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) out[k].transformation(r, c) = res[k].transformation[4 * r + c];
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) out[k].information(r, c) = res[k].information[6 * r + c];
    }
    return out;
  }

  DepthOdometryResult compute(const DepthFrame& source, const DepthFrame& target, const PinholeCameraIntrinsic& intrinsic,
                              const Matrix4& init = Matrix4::Identity(), const DepthOdometryOption& option = DepthOdometryOption()) {
    return computeBatch({source}, {target}, {intrinsic}, {init}, option)[0];
  }

 private:
  teaser_hip_icp* h_ = nullptr;
};

// One pair on a handle of its own; keep a teaser::DepthOdometry for more than one call.
inline DepthOdometryResult computeDepthOdometry(const DepthFrame& source, const DepthFrame& target,
                                                const PinholeCameraIntrinsic& intrinsic, const Matrix4& init = Matrix4::Identity(),
                                                const DepthOdometryOption& option = DepthOdometryOption()) {
  DepthOdometry odo;
  return odo.compute(source, target, intrinsic, init, option);
}

// What trackFrameToModel returns: the tracked pose of the frame, the odometry's result and the ray-cast depth of the
// model the frame was tracked against (float32 metres, row-major, 0 where the model has no surface).
struct TrackingResult {
  Matrix4 camera_to_world = Matrix4::Identity();
  DepthOdometryResult result;
  std::vector<float> model_depth;
};

// Frame-to-model tracking (Open3D's t::pipelines::slam::Model::TrackFrameToModel) against a teaser::UniformTSDFVolume
// or a teaser::ScalableTSDFVolume of any colour type.  The model's depth map is ray cast at the initial pose -- rayCast
// takes the world-to-camera extrinsic, so it is given the inverse of camera_to_world_init -- with the frame's intrinsic
// and size; depth odometry runs with the input frame as SOURCE, the model view as TARGET and the identity as init; the
// frame's pose is camera_to_world_init T.  A uint16 frame is turned into float32 metres first (both images of a pair
// share the format).  The ray-cast map comes back to the host and goes up again with the frame.
template <class Volume>
TrackingResult trackFrameToModel(Volume& volume, DepthOdometry& odometry, const DepthFrame& frame,
                                 const PinholeCameraIntrinsic& intrinsic, const Matrix4& camera_to_world_init,
                                 const DepthOdometryOption& option = DepthOdometryOption(), double weight_threshold = 1.0) {
  TSDFRayCastOptions ro;
  ro.depth_min = option.depth_min > 0.1 ? option.depth_min : 0.1, ro.depth_max = option.depth_max, ro.weight_threshold = weight_threshold;
  ro.vertex_map = ro.normal_map = ro.color = false;
  TrackingResult out;
  out.model_depth = volume.rayCast(intrinsic, detail::inverse4(camera_to_world_init), frame.width, frame.height, ro).depth;
  std::vector<float> metres;
  DepthFrame source = frame;
  if (frame.depth_format == 0) {
    metres.resize((size_t)frame.width * (size_t)frame.height);
    const float scale = (float)option.depth_scale;
    for (int i = 0; i < frame.height; ++i)
      for (int j = 0; j < frame.width; ++j) {
        uint16_t d;
        std::memcpy(&d, (const unsigned char*)frame.depth + (int64_t)i * frame.depth_row_bytes + 2 * (int64_t)j, 2);
        metres[(size_t)i * (size_t)frame.width + (size_t)j] = (float)d / scale;
      }
    source = DepthFrame::F32(metres.data(), frame.width, frame.height);
  }
  out.result = odometry.compute(source, DepthFrame::F32(out.model_depth.data(), frame.width, frame.height), intrinsic,
                                Matrix4::Identity(), option);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double v = 0.0;
      for (int m = 0; m < 4; ++m) v += camera_to_world_init(r, m) * out.result.transformation(m, c);
      out.camera_to_world(r, c) = v;
    }
  return out;
}

}  // namespace teaser
