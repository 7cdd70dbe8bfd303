// teaser/tsdf.h -- TSDF volume integration on the MI355X with the surface of open3d::pipelines::integration::
// UniformTSDFVolume: depth frames and their camera poses in, one fused cloud out, over the C ABI (include/teaser_hip.h,
// "TSDF volume", where the contract is written out), and of ScalableTSDFVolume ("Scalable TSDF volume").  Header-only.
//
// The volume lives on the device as long as the object: frames go up, only the extracted surface comes back.  Images
// come in as teaser::DepthFrame (teaser/rgbd.h), a view that owns nothing; `extrinsic` is world-to-camera as in Open3D.
// Clouds are teaser::Matrix3X (one point per column).  An object is reusable but not re-entrant.  A failed call throws
// teaser::TSDFError, the constructor too when no MI355X is visible (there is no CPU path).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "teaser/handle.h"
#include "teaser/rgbd.h"
#include "teaser_hip.h"

namespace teaser {

enum class TSDFVolumeColorType { NoColor = 0, RGB8 = 1, Gray32 = 2 };

class TSDFError : public std::runtime_error {
 public:
  TSDFError(int32_t status, const std::string& what) : std::runtime_error(what), status_(status) {}
  int32_t status() const { return status_; }

 private:
  int32_t status_;
};

// What the extractions return; normals and colors have no columns where they do not exist.
struct TSDFPointCloud {
  Matrix3X points, normals, colors;
};

// What extractTriangleMesh returns: one vertex per column; vertex_colors and vertex_normals have no columns where they
// do not exist; triangles holds three vertex indices per triangle.
struct TSDFTriangleMesh {
  Matrix3X vertices, vertex_colors, vertex_normals;
  std::vector<int32_t> triangles;
};

// The options of a ray cast: the z-depth range of a ray, the weight a voxel needs to count as surface (Open3D's 3.0)
// and the maps wanted beside the depth.
struct TSDFRayCastOptions {
  double depth_min = 0.1, depth_max = 3.0, weight_threshold = 3.0;
  bool vertex_map = true, normal_map = true, color = true;
};

// What rayCast returns: row-major float32 maps, depth height x width (the z-depth, 0 where no surface was met), the
// others height x width x 3; a map that was not asked for, and the colour of a volume without a colour type, is empty.
struct TSDFRayCastResult {
  int width = 0, height = 0;
  std::vector<float> depth, vertex_map, normal_map, color;
  int64_t hits = 0;  // the pixels that met a surface
};

namespace detail {

// The records, results and pointers of one ray-cast call, which both volume classes hand to their entry point.
struct RayCastCall {
  std::vector<teaser_tsdf_view_c> rec;
  std::vector<TSDFRayCastResult> out;
  std::vector<float*> pd, pv, pn, pc;
  std::vector<int64_t> hits;

  RayCastCall(const char* who, const std::vector<PinholeCameraIntrinsic>& intrinsics, const std::vector<Matrix4>& extrinsics,
              const std::vector<int>& widths, const std::vector<int>& heights, const TSDFRayCastOptions& options, bool colored) {
    const size_t b = extrinsics.size();
    if ((intrinsics.size() != 1 && intrinsics.size() != b) || (widths.size() != 1 && widths.size() != b) ||
        (heights.size() != 1 && heights.size() != b))
      throw std::invalid_argument(std::string(who) + ": one intrinsic, width and height (or one per view)");
    rec.resize(b), out.resize(b), pd.resize(b), pv.resize(b), pn.resize(b), pc.resize(b), hits.assign(b, 0);
    for (size_t k = 0; k < b; ++k) {
      const PinholeCameraIntrinsic& K = intrinsics[intrinsics.size() == 1 ? 0 : k];
      teaser_tsdf_view_c& r = rec[k];
      teaser_hip_tsdf_view_default(&r);
      r.width = widths[widths.size() == 1 ? 0 : k], r.height = heights[heights.size() == 1 ? 0 : k];
      r.fx = K.fx, r.fy = K.fy, r.cx = K.cx, r.cy = K.cy;
      row_major(extrinsics[k], r.extrinsic);
      r.depth_min = options.depth_min, r.depth_max = options.depth_max, r.weight_threshold = options.weight_threshold;
      TSDFRayCastResult& o = out[k];
      o.width = r.width, o.height = r.height;
      const size_t px = r.width > 0 && r.height > 0 ? (size_t)r.width * (size_t)r.height : 0;
      o.depth.assign(px, 0.0f);
      if (options.vertex_map) o.vertex_map.assign(3 * px, 0.0f);
      if (options.normal_map) o.normal_map.assign(3 * px, 0.0f);
      if (colored) o.color.assign(3 * px, 0.0f);
      pd[k] = px ? o.depth.data() : nullptr;
      pv[k] = px && options.vertex_map ? o.vertex_map.data() : nullptr;
      pn[k] = px && options.normal_map ? o.normal_map.data() : nullptr;
      pc[k] = px && colored ? o.color.data() : nullptr;
    }
  }

  std::vector<TSDFRayCastResult> results() {
    for (size_t k = 0; k < out.size(); ++k) out[k].hits = hits[k];
    return std::move(out);
  }
};

}  // namespace detail

class UniformTSDFVolume {
 public:
  UniformTSDFVolume(double length, int resolution, double sdf_trunc, TSDFVolumeColorType color_type,
                    double origin_x = 0.0, double origin_y = 0.0, double origin_z = 0.0, int device = -1)
      : length_(length), resolution_(resolution), color_type_(color_type) {
    teaser_tsdf_volume_c v;
    teaser_hip_tsdf_volume_default(&v);
    v.length = length, v.resolution = resolution, v.sdf_trunc = sdf_trunc, v.color_type = (int32_t)color_type;
    v.origin[0] = origin_x, v.origin[1] = origin_y, v.origin[2] = origin_z;
    const int32_t rc = h_.create(v, device);
    if (rc != TEASER_HIP_OK)
      throw TSDFError(rc, "teaser::UniformTSDFVolume: teaser_hip_tsdf_create failed (status " + std::to_string(rc) +
                              (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)"
                                                              : std::string("): ") + teaser_hip_tsdf_last_error(nullptr)));
  }

  double voxelLength() const { return length_ / resolution_; }
  int resolution() const { return resolution_; }

  // Open3D's Integrate(image, intrinsic, extrinsic), the RGBD image given as the frame's parts.
  void integrate(const DepthFrame& frame, const PinholeCameraIntrinsic& intrinsic, const Matrix4& extrinsic,
                 double depth_scale = 1000.0, double depth_trunc = 3.0) {
    integrateBatch({frame}, {intrinsic}, {extrinsic}, depth_scale, depth_trunc);
  }

  // The frames, in the order given, in one call: a voxel ends with the bits one integrate() per frame leaves.
  // intrinsics: one for all or one per frame.
  void integrateBatch(const std::vector<DepthFrame>& frames, const std::vector<PinholeCameraIntrinsic>& intrinsics,
                      const std::vector<Matrix4>& extrinsics, double depth_scale = 1000.0, double depth_trunc = 3.0) {
    const size_t b = frames.size();
    if ((intrinsics.size() != 1 && intrinsics.size() != b) || extrinsics.size() != b)
      throw std::invalid_argument("teaser::UniformTSDFVolume: one intrinsic (or one per frame) and one extrinsic per frame");
    std::vector<teaser_tsdf_frame_c> rec(b);
    std::vector<const void*> pd(b), pc(b);
    for (size_t k = 0; k < b; ++k) {
      const DepthFrame& f = frames[k];
      const PinholeCameraIntrinsic& K = intrinsics[intrinsics.size() == 1 ? 0 : k];
      teaser_tsdf_frame_c& r = rec[k];
      r = teaser_tsdf_frame_c{};
      r.width = f.width, r.height = f.height, r.depth_format = f.depth_format, r.color_format = f.color_format;
      r.depth_row_bytes = f.depth_row_bytes, r.color_row_bytes = f.color_row_bytes;
      r.fx = K.fx, r.fy = K.fy, r.cx = K.cx, r.cy = K.cy;
      detail::row_major(extrinsics[k], r.extrinsic);
      r.depth_scale = depth_scale, r.depth_trunc = depth_trunc;
      pd[k] = f.depth, pc[k] = f.color;
    }
    check(teaser_hip_tsdf_integrate_batch(h_, (int32_t)b, rec.data(), pd.data(), pc.data()));
  }

  // Open3D's ExtractPointCloud: points, normals (unless with_normals is false) and, for a volume with a colour type,
  // colours, in Open3D's order.
  TSDFPointCloud extractPointCloud(bool with_normals = true) {
    const bool colored = color_type_ != TSDFVolumeColorType::NoColor;
    int64_t count = 0;
    check(teaser_hip_tsdf_extract_point_cloud(h_, 0, nullptr, nullptr, nullptr, &count));
    TSDFPointCloud out;
    out.points = Matrix3X(3, count);
    if (with_normals) out.normals = Matrix3X(3, count);
    if (colored) out.colors = Matrix3X(3, count);
    if (count > 0)
      check(teaser_hip_tsdf_extract_point_cloud(h_, count, out.points.data(), with_normals ? out.normals.data() : nullptr,
                                                colored ? out.colors.data() : nullptr, &count));
    return out;
  }

  // Open3D's ExtractVoxelPointCloud: every observed voxel's centre, (tsdf + 1) / 2 as its colour.
  TSDFPointCloud extractVoxelPointCloud() {
    int64_t count = 0;
    check(teaser_hip_tsdf_extract_voxel_point_cloud(h_, 0, nullptr, nullptr, &count));
    TSDFPointCloud out;
    out.points = Matrix3X(3, count);
    out.colors = Matrix3X(3, count);
    if (count > 0)
      check(teaser_hip_tsdf_extract_voxel_point_cloud(h_, count, out.points.data(), out.colors.data(), &count));
    return out;
  }

  // Open3D's ExtractTriangleMesh (marching cubes): vertices and triangles in the order of Open3D's loop, vertex colours
  // for a volume with a colour type.  with_vertex_normals adds the TSDF gradient at every vertex (the normal rule of the
  // point cloud), which Open3D's call does not give.
  TSDFTriangleMesh extractTriangleMesh(bool with_vertex_normals = false) {
    const bool colored = color_type_ != TSDFVolumeColorType::NoColor;
    int64_t nv = 0, nt = 0;
    check(teaser_hip_tsdf_extract_triangle_mesh(h_, 0, nullptr, nullptr, nullptr, 0, nullptr, &nv, &nt));
    TSDFTriangleMesh out;
    out.vertices = Matrix3X(3, nv);
    if (colored) out.vertex_colors = Matrix3X(3, nv);
    if (with_vertex_normals) out.vertex_normals = Matrix3X(3, nv);
    out.triangles.resize(3 * (size_t)nt);
    if (nv > 0 || nt > 0)
      check(teaser_hip_tsdf_extract_triangle_mesh(h_, nv, out.vertices.data(), colored ? out.vertex_colors.data() : nullptr,
                                                  with_vertex_normals ? out.vertex_normals.data() : nullptr, nt,
                                                  out.triangles.data(), &nv, &nt));
    return out;
  }

  // The fused model seen from a camera (Open3D's VoxelBlockGrid::RayCast for the dense volume): per pixel the z-depth
  // of the first surface its ray meets, the world point, the normal and the colour.  The rules: include/teaser_hip.h,
  // "TSDF ray casting".
  TSDFRayCastResult rayCast(const PinholeCameraIntrinsic& intrinsic, const Matrix4& extrinsic, int width, int height,
                            const TSDFRayCastOptions& options = TSDFRayCastOptions()) {
    return rayCastBatch({intrinsic}, {extrinsic}, {width}, {height}, options)[0];
  }

  // All views in one call: one launch, one synchronisation.  intrinsics, widths, heights: one for all or one per view.
  std::vector<TSDFRayCastResult> rayCastBatch(const std::vector<PinholeCameraIntrinsic>& intrinsics,
                                              const std::vector<Matrix4>& extrinsics, const std::vector<int>& widths,
                                              const std::vector<int>& heights,
                                              const TSDFRayCastOptions& options = TSDFRayCastOptions()) {
    detail::RayCastCall c("teaser::UniformTSDFVolume", intrinsics, extrinsics, widths, heights, options,
                          options.color && color_type_ != TSDFVolumeColorType::NoColor);
    check(teaser_hip_tsdf_ray_cast_views(h_, (int32_t)c.rec.size(), c.rec.data(), c.pd.data(), c.pv.data(), c.pn.data(),
                                         c.pc.data(), c.hits.data()));
    return c.results();
  }

  // resolution^3 x 2 floats (tsdf, weight) in Open3D's voxel order (x R + y) R + z.
  std::vector<float> extractVolumeTSDF() {
    std::vector<float> out(2 * voxels());
    check(teaser_hip_tsdf_download(h_, out.data(), nullptr));
    return out;
  }
  // resolution^3 x 3 doubles in Open3D's voxel order (a volume with a colour type only).
  std::vector<double> extractVolumeColor() {
    std::vector<double> out(3 * voxels());
    check(teaser_hip_tsdf_download(h_, nullptr, out.data()));
    return out;
  }
  void injectVolumeTSDF(const std::vector<float>& tsdf_weight) {
    if (tsdf_weight.size() != 2 * voxels()) throw std::invalid_argument("teaser::UniformTSDFVolume: tsdf_weight has another size");
    check(teaser_hip_tsdf_upload(h_, tsdf_weight.data(), nullptr));
  }
  void injectVolumeColor(const std::vector<double>& color) {
    if (color.size() != 3 * voxels()) throw std::invalid_argument("teaser::UniformTSDFVolume: color has another size");
    check(teaser_hip_tsdf_upload(h_, nullptr, color.data()));
  }
  void reset() { check(teaser_hip_tsdf_reset(h_)); }

 private:
  size_t voxels() const { return (size_t)resolution_ * (size_t)resolution_ * (size_t)resolution_; }
  void check(int32_t rc) {
    if (rc != TEASER_HIP_OK)
      throw TSDFError(rc, "teaser::UniformTSDFVolume: status " + std::to_string(rc) + ": " + teaser_hip_tsdf_last_error(h_));
  }
  double length_;
  int resolution_;
  TSDFVolumeColorType color_type_;
  detail::LazyTsdf h_;
};

// Open3D's ScalableTSDFVolume: only the blocks of 16^3 voxels that depth frames have come near are stored (include/
// teaser_hip.h, "Scalable TSDF volume"), and rayCast / rayCastBatch render them into cameras ("Scalable TSDF ray
// casting") with the dense class's options and result.  extractTriangleMesh runs marching cubes over them ("Scalable
// TSDF triangle mesh").
class ScalableTSDFVolume {
 public:
  // What the last integrate call reported: (frame, block) pairs touched, blocks opened, and (frame, point) pairs with
  // a block outside the index range.
  struct Counts {
    int64_t touched = 0, opened = 0, out_of_range = 0;
  };

  ScalableTSDFVolume(double voxel_length, double sdf_trunc, TSDFVolumeColorType color_type, int volume_unit_resolution = 16,
                     int depth_sampling_stride = 4, int device = -1)
      : voxel_length_(voxel_length), color_type_(color_type) {
    teaser_stsdf_volume_c v;
    teaser_hip_stsdf_volume_default(&v);
    v.voxel_length = voxel_length, v.sdf_trunc = sdf_trunc, v.color_type = (int32_t)color_type;
    v.volume_unit_resolution = volume_unit_resolution, v.depth_sampling_stride = depth_sampling_stride;
    const int32_t rc = h_.create(v, device);
    if (rc != TEASER_HIP_OK)
      throw TSDFError(rc, "teaser::ScalableTSDFVolume: teaser_hip_stsdf_create failed (status " + std::to_string(rc) +
                              (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)"
                                                              : std::string("): ") + teaser_hip_stsdf_last_error(nullptr)));
  }

  double voxelLength() const { return voxel_length_; }
  const Counts& lastCounts() const { return counts_; }

  void integrate(const DepthFrame& frame, const PinholeCameraIntrinsic& intrinsic, const Matrix4& extrinsic,
                 double depth_scale = 1000.0, double depth_trunc = 3.0) {
    integrateBatch({frame}, {intrinsic}, {extrinsic}, depth_scale, depth_trunc);
  }

  // The frames, in the order given, in one call: the blocks end with the bits one integrate() per frame leaves.
  void integrateBatch(const std::vector<DepthFrame>& frames, const std::vector<PinholeCameraIntrinsic>& intrinsics,
                      const std::vector<Matrix4>& extrinsics, double depth_scale = 1000.0, double depth_trunc = 3.0) {
    const size_t b = frames.size();
    if ((intrinsics.size() != 1 && intrinsics.size() != b) || extrinsics.size() != b)
      throw std::invalid_argument("teaser::ScalableTSDFVolume: one intrinsic (or one per frame) and one extrinsic per frame");
    std::vector<teaser_tsdf_frame_c> rec(b);
    std::vector<const void*> pd(b), pc(b);
    for (size_t k = 0; k < b; ++k) {
      const DepthFrame& f = frames[k];
      const PinholeCameraIntrinsic& K = intrinsics[intrinsics.size() == 1 ? 0 : k];
      teaser_tsdf_frame_c& r = rec[k];
      r = teaser_tsdf_frame_c{};
      r.width = f.width, r.height = f.height, r.depth_format = f.depth_format, r.color_format = f.color_format;
      r.depth_row_bytes = f.depth_row_bytes, r.color_row_bytes = f.color_row_bytes;
      r.fx = K.fx, r.fy = K.fy, r.cx = K.cx, r.cy = K.cy;
      detail::row_major(extrinsics[k], r.extrinsic);
      r.depth_scale = depth_scale, r.depth_trunc = depth_trunc;
      pd[k] = f.depth, pc[k] = f.color;
    }
    counts_ = Counts();
    check(teaser_hip_stsdf_integrate_frames(h_, (int32_t)b, rec.data(), pd.data(), pc.data(), &counts_.touched, &counts_.opened,
                                           &counts_.out_of_range));
  }

  // Points, normals (unless with_normals is false) and, for a volume with a colour type, colours: blocks in ascending
  // (bx, by, bz), Open3D's order inside a block.
  TSDFPointCloud extractPointCloud(bool with_normals = true) {
    const bool colored = color_type_ != TSDFVolumeColorType::NoColor;
    int64_t count = 0;
    check(teaser_hip_stsdf_extract_point_cloud(h_, 0, nullptr, nullptr, nullptr, &count));
    TSDFPointCloud out;
    out.points = Matrix3X(3, count);
    if (with_normals) out.normals = Matrix3X(3, count);
    if (colored) out.colors = Matrix3X(3, count);
    if (count > 0)
      check(teaser_hip_stsdf_extract_point_cloud(h_, count, out.points.data(), with_normals ? out.normals.data() : nullptr,
                                                 colored ? out.colors.data() : nullptr, &count));
    return out;
  }

  TSDFPointCloud extractVoxelPointCloud() {
    int64_t count = 0;
    check(teaser_hip_stsdf_extract_voxel_point_cloud(h_, 0, nullptr, nullptr, &count));
    TSDFPointCloud out;
    out.points = Matrix3X(3, count);
    out.colors = Matrix3X(3, count);
    if (count > 0)
      check(teaser_hip_stsdf_extract_voxel_point_cloud(h_, count, out.points.data(), out.colors.data(), &count));
    return out;
  }

  // Open3D's ExtractTriangleMesh (marching cubes) over the open blocks and across their faces: blocks in ascending
  // (bx, by, bz), the cubes of a block in (x, y, z) order, vertex colours for a volume with a colour type.
  // with_vertex_normals adds the TSDF gradient at every vertex (the normal rule of the point cloud).  A count call, then
  // a fill call; PLYWriter::writeMesh takes the result as it is.
  TSDFTriangleMesh extractTriangleMesh(bool with_vertex_normals = false) {
    const bool colored = color_type_ != TSDFVolumeColorType::NoColor;
    int64_t nv = 0, nt = 0;
    check(teaser_hip_stsdf_extract_triangle_mesh(h_, 0, nullptr, nullptr, nullptr, 0, nullptr, &nv, &nt));
    TSDFTriangleMesh out;
    out.vertices = Matrix3X(3, nv);
    if (colored) out.vertex_colors = Matrix3X(3, nv);
    if (with_vertex_normals) out.vertex_normals = Matrix3X(3, nv);
    out.triangles.resize(3 * (size_t)nt);
    if (nv > 0 || nt > 0)
      check(teaser_hip_stsdf_extract_triangle_mesh(h_, nv, out.vertices.data(), colored ? out.vertex_colors.data() : nullptr,
                                                   with_vertex_normals ? out.vertex_normals.data() : nullptr, nt,
                                                   out.triangles.data(), &nv, &nt));
    return out;
  }

  // The fused model seen from a camera (Open3D's VoxelBlockGrid::RayCast): per pixel the z-depth of the first surface
  // its ray meets in the open blocks, the world point, the normal and the colour.  The rules: include/teaser_hip.h,
  // "Scalable TSDF ray casting".
  TSDFRayCastResult rayCast(const PinholeCameraIntrinsic& intrinsic, const Matrix4& extrinsic, int width, int height,
                            const TSDFRayCastOptions& options = TSDFRayCastOptions()) {
    return rayCastBatch({intrinsic}, {extrinsic}, {width}, {height}, options)[0];
  }

  // All views in one call: one launch, one synchronisation.  intrinsics, widths, heights: one for all or one per view.
  std::vector<TSDFRayCastResult> rayCastBatch(const std::vector<PinholeCameraIntrinsic>& intrinsics,
                                              const std::vector<Matrix4>& extrinsics, const std::vector<int>& widths,
                                              const std::vector<int>& heights,
                                              const TSDFRayCastOptions& options = TSDFRayCastOptions()) {
    detail::RayCastCall c("teaser::ScalableTSDFVolume", intrinsics, extrinsics, widths, heights, options,
                          options.color && color_type_ != TSDFVolumeColorType::NoColor);
    check(teaser_hip_stsdf_ray_cast_views(h_, (int32_t)c.rec.size(), c.rec.data(), c.pd.data(), c.pv.data(), c.pn.data(),
                                          c.pc.data(), c.hits.data()));
    return c.results();
  }

  int64_t blockCount() {
    int64_t n = 0;
    check(teaser_hip_stsdf_block_count(h_, &n));
    return n;
  }
  // (bx, by, bz) of every open block, three int32 per block, in ascending order.
  std::vector<int32_t> blockKeys() {
    int64_t n = blockCount();
    std::vector<int32_t> keys(3 * (size_t)n);
    if (n > 0) check(teaser_hip_stsdf_block_keys(h_, n, keys.data(), &n));
    return keys;
  }
  void reset() { check(teaser_hip_stsdf_reset(h_)); }

 private:
  void check(int32_t rc) {
    if (rc != TEASER_HIP_OK)
      throw TSDFError(rc, "teaser::ScalableTSDFVolume: status " + std::to_string(rc) + ": " + teaser_hip_stsdf_last_error(h_));
  }
  double voxel_length_;
  TSDFVolumeColorType color_type_;
  Counts counts_;
  detail::LazyStsdf h_;
};

}  // namespace teaser
