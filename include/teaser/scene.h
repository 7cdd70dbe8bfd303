// teaser/scene.h -- a ray-casting scene for triangle meshes on the MI355X with the surface of open3d::t::geometry::
// RaycastingScene: meshes in, then the first surface a ray meets, occlusion tests and the closest point of the surface to
// a point, over the C ABI (include/teaser_hip.h, "Ray casting scene", where the contract is written out).  Header-only.
//
// Rays are six float32 each (origin, direction; the direction is used as given, so t counts in units of its length),
// points three.  Results are row-major float32 / uint32 arrays; a miss has t_hit = +inf and the ids
// RaycastingScene::INVALID_ID.  An object is reusable but not re-entrant.  A failed call throws teaser::SceneError, the
// constructor too when no MI355X is visible (there is no CPU path).  Not offered: signed distance and occupancy,
// count_intersections / list_intersections, other primitives, refitting, mesh sampling.
#pragma once

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "teaser/handle.h"
#include "teaser/rgbd.h"
#include "teaser/tsdf.h"
#include "teaser_hip.h"

namespace teaser {

class SceneError : public std::runtime_error {
 public:
  SceneError(int32_t status, const std::string& what) : std::runtime_error(what), status_(status) {}
  int32_t status() const { return status_; }

 private:
  int32_t status_;
};

// What castRays and castViews return: one entry per ray (per pixel, row-major); uvs two and normals three per ray.
struct SceneRayResult {
  int width = 0, height = 0;  // of a view; castRays: width = the number of rays, height = 1
  std::vector<float> t_hit, primitive_uvs, primitive_normals;
  std::vector<uint32_t> geometry_ids, primitive_ids;
};

// What computeClosestPoints returns.
struct SceneClosestResult {
  std::vector<float> points, distance, primitive_uvs, primitive_normals;
  std::vector<uint32_t> geometry_ids, primitive_ids;
};

class RaycastingScene {
 public:
  static constexpr uint32_t INVALID_ID = 0xFFFFFFFFu;

  explicit RaycastingScene(int device = -1) {
    const int32_t rc = teaser_hip_scene_create(device, &h_);
    if (rc != TEASER_HIP_OK) {
      h_ = nullptr;
      throw SceneError(rc, "teaser::RaycastingScene: teaser_hip_scene_create failed (status " + std::to_string(rc) +
                               (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)" : ")"));
    }
  }
  RaycastingScene(const RaycastingScene&) = delete;
  RaycastingScene& operator=(const RaycastingScene&) = delete;
  ~RaycastingScene() {
    if (h_) teaser_hip_scene_destroy(h_);
  }

  // vertices: three float32 per vertex; triangles: three indices per triangle.  Returns the geometry id 0, 1, 2, ...
  uint32_t addTriangles(const std::vector<float>& vertices, const std::vector<uint32_t>& triangles) {
    uint32_t id = 0;
    check(teaser_hip_scene_add_triangles(h_, vertices.empty() ? nullptr : vertices.data(), (int64_t)(vertices.size() / 3),
                                         triangles.empty() ? nullptr : triangles.data(), (int64_t)(triangles.size() / 3), &id),
          "addTriangles");
    return id;
  }
  // The mesh of extractTriangleMesh, its vertices rounded to float32.
  uint32_t addTriangles(const TSDFTriangleMesh& mesh) {
    std::vector<float> v((size_t)(3 * mesh.vertices.cols()));
    for (int64_t k = 0; k < (int64_t)mesh.vertices.cols(); ++k)
      for (int r = 0; r < 3; ++r) v[(size_t)(3 * k + r)] = (float)mesh.vertices(r, k);
    std::vector<uint32_t> t(mesh.triangles.size());
    for (size_t k = 0; k < t.size(); ++k) {
      if (mesh.triangles[k] < 0) throw SceneError(TEASER_HIP_ERR_BAD_ARG, "teaser::RaycastingScene::addTriangles: a negative index");
      t[k] = (uint32_t)mesh.triangles[k];
    }
    return addTriangles(v, t);
  }
  void commit() { check(teaser_hip_scene_commit(h_), "commit"); }
  int64_t triangleCount() const {
    int64_t n = 0;
    check(teaser_hip_scene_triangle_count(h_, &n), "triangleCount");
    return n;
  }

  SceneRayResult castRays(const std::vector<float>& rays) {
    const size_t n = rays.size() / 6;
    SceneRayResult r;
    r.width = (int)n, r.height = 1;
    r.t_hit.resize(n), r.geometry_ids.resize(n), r.primitive_ids.resize(n), r.primitive_uvs.resize(2 * n), r.primitive_normals.resize(3 * n);
    check(teaser_hip_scene_cast_rays(h_, n ? rays.data() : nullptr, (int64_t)n, r.t_hit.data(), r.geometry_ids.data(),
                                     r.primitive_ids.data(), r.primitive_uvs.data(), r.primitive_normals.data()),
          "castRays");
    return r;
  }

  std::vector<uint8_t> testOcclusions(const std::vector<float>& rays, double tnear = 0.0,
                                      double tfar = std::numeric_limits<double>::infinity()) {
    const size_t n = rays.size() / 6;
    std::vector<uint8_t> occ(n, 0);
    check(teaser_hip_scene_test_occlusions(h_, n ? rays.data() : nullptr, (int64_t)n, tnear, tfar, occ.data()), "testOcclusions");
    return occ;
  }

  SceneClosestResult computeClosestPoints(const std::vector<float>& points) {
    const size_t n = points.size() / 3;
    SceneClosestResult r;
    r.points.resize(3 * n), r.distance.resize(n), r.geometry_ids.resize(n), r.primitive_ids.resize(n);
    r.primitive_uvs.resize(2 * n), r.primitive_normals.resize(3 * n);
    check(teaser_hip_scene_closest_points(h_, n ? points.data() : nullptr, (int64_t)n, r.points.data(), r.distance.data(),
                                          r.geometry_ids.data(), r.primitive_ids.data(), r.primitive_uvs.data(),
                                          r.primitive_normals.data()),
          "computeClosestPoints");
    return r;
  }

  // The distances alone: nothing else is computed or copied.
  std::vector<float> computeDistance(const std::vector<float>& points) {
    const size_t n = points.size() / 3;
    std::vector<float> d(n);
    check(teaser_hip_scene_closest_points(h_, n ? points.data() : nullptr, (int64_t)n, nullptr, d.data(), nullptr, nullptr, nullptr, nullptr),
          "computeDistance");
    return d;
  }

  // One result per extrinsic (world to camera), the rays generated on the device, all views in one call; equal to
  // castRays(createRaysPinhole(...)) bit for bit.  The width and height are the intrinsic's.
  std::vector<SceneRayResult> castViews(const PinholeCameraIntrinsic& K, const std::vector<Matrix4>& extrinsics,
                                        double pixel_offset = 0.5) {
    const size_t b = extrinsics.size();
    std::vector<teaser_scene_view_c> rec(b);
    std::vector<SceneRayResult> out(b);
    std::vector<float*> pt(b), puv(b), pn(b);
    std::vector<uint32_t*> pg(b), pp(b);
    for (size_t k = 0; k < b; ++k) {
      teaser_scene_view_c& r = rec[k];
      teaser_hip_scene_view_default(&r);
      r.width = K.width, r.height = K.height, r.fx = K.fx, r.fy = K.fy, r.cx = K.cx, r.cy = K.cy;
      detail::row_major(extrinsics[k], r.extrinsic);
      r.pixel_offset = pixel_offset;
      const size_t px = K.width > 0 && K.height > 0 ? (size_t)K.width * (size_t)K.height : 0;
      SceneRayResult& o = out[k];
      o.width = K.width, o.height = K.height;
      o.t_hit.resize(px), o.geometry_ids.resize(px), o.primitive_ids.resize(px), o.primitive_uvs.resize(2 * px), o.primitive_normals.resize(3 * px);
      pt[k] = o.t_hit.data(), pg[k] = o.geometry_ids.data(), pp[k] = o.primitive_ids.data();
      puv[k] = o.primitive_uvs.data(), pn[k] = o.primitive_normals.data();
    }
    check(teaser_hip_scene_cast_views(h_, rec.data(), (int32_t)b, pt.data(), pg.data(), pp.data(), puv.data(), pn.data()), "castViews");
    return out;
  }

  // Open3D's create_rays_pinhole on the host, by the formulas of the header ("Views"): height x width x 6 float32.
  static std::vector<float> createRaysPinhole(const PinholeCameraIntrinsic& K, const Matrix4& extrinsic, double pixel_offset = 0.5) {
    double E[16];
    detail::row_major(extrinsic, E);
    const size_t px = K.width > 0 && K.height > 0 ? (size_t)K.width * (size_t)K.height : 0;
    std::vector<float> rays(6 * px);
    float o[3];
    for (int k = 0; k < 3; ++k) o[k] = (float)-((E[k] * E[3] + E[4 + k] * E[7]) + E[8 + k] * E[11]);
    for (int v = 0; v < K.height; ++v)
      for (int u = 0; u < K.width; ++u) {
        const double a = (((double)u + pixel_offset) - K.cx) / K.fx, b = (((double)v + pixel_offset) - K.cy) / K.fy;
        float* r = &rays[6 * ((size_t)v * (size_t)K.width + (size_t)u)];
        for (int k = 0; k < 3; ++k) {
          const double p = E[k] * a, q = E[4 + k] * b;  // two roundings each; on a target with fused product-adds compile with -ffp-contract=off
          r[k] = o[k], r[3 + k] = (float)((p + q) + E[8 + k]);
        }
      }
    return rays;
  }

 private:
  void check(int32_t rc, const char* what) const {
    if (rc != TEASER_HIP_OK)
      throw SceneError(rc, std::string("teaser::RaycastingScene::") + what + ": " + teaser_hip_scene_last_error(h_));
  }
  teaser_hip_scene* h_ = nullptr;
};

}  // namespace teaser
