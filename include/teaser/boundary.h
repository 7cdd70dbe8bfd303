// teaser/boundary.h -- boundary points on the MI355X: Open3D's PointCloud::ComputeBoundaryPoints (the angle criterion of
// PCL's BoundaryEstimation) with KDTreeSearchParamHybrid or KDTreeSearchParamKNN, FP64, over the C ABI
// (include/teaser_hip.h, "Boundary points", where the contract is written out).  Header-only.
//
// Clouds and normals are teaser::Matrix3X as in teaser/icp.h (one point per column), the search a teaser::NormalSearch
// (NormalSearch::Hybrid(radius, max_nn) or NormalSearch::KNN(k), not oriented, max_nn in [2, 100]).  A
// teaser::BoundaryDetector holds one ICP handle and is reusable but not re-entrant.  A failed call throws
// teaser::ICPError, the constructor too when no MI355X is visible (there is no CPU path).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "teaser/icp.h"

namespace teaser {

// Open3D's arguments: the search (radius, max_nn) and the angle threshold in degrees, [0, 360].
struct BoundaryParams {
  NormalSearch search = NormalSearch::Hybrid(0.1, 30);
  double angle_threshold = 90.0;
  BoundaryParams() = default;
  BoundaryParams(double radius, int max_nn = 30, double angle_threshold_deg = 90.0)
      : search(NormalSearch::Hybrid(radius, max_nn)), angle_threshold(angle_threshold_deg) {}
  BoundaryParams(const NormalSearch& s, double angle_threshold_deg = 90.0) : search(s), angle_threshold(angle_threshold_deg) {}
};

// One cloud's result.  mask[i] is 1 for a boundary point; the mask is the result, nothing is compacted on the device.
struct BoundaryResult {
  std::vector<uint8_t> mask;
  int32_t n_boundary = 0;        // the number of ones, counted on the device
  std::vector<double> max_gap;   // radians, when asked for; NaN where the normal gives no tangent frame
  std::vector<int32_t> counts;   // the length of every point's neighbour list (the point included), when asked for
  Matrix3X normals;              // the normals the cloud was computed with, when asked for
  std::vector<int64_t> indices() const {
    std::vector<int64_t> out;
    for (size_t i = 0; i < mask.size(); ++i)
      if (mask[i]) out.push_back((int64_t)i);
    return out;
  }
};

class BoundaryDetector {
 public:
  explicit BoundaryDetector(int device = -1) {
    const int32_t rc = teaser_hip_icp_create(device, &h_);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::BoundaryDetector: teaser_hip_icp_create failed (status " + std::to_string(rc) +
                             (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)" : ")"));
  }
  ~BoundaryDetector() { teaser_hip_icp_destroy(h_); }
  BoundaryDetector(const BoundaryDetector&) = delete;
  BoundaryDetector& operator=(const BoundaryDetector&) = delete;

  // Many clouds in one launch sequence; result c is identical to cloud c computed alone.  normals: one matrix per
  // cloud; a cloud whose matrix has no columns although the cloud has points gets its normals estimated on the device
  // first, by normal_search[c] (any orientation) -- the bits of ICP::estimateNormalsBatch followed by this call.
  std::vector<BoundaryResult> computeBatch(const std::vector<Matrix3X>& clouds, const std::vector<Matrix3X>& normals,
                                           const std::vector<BoundaryParams>& params,
                                           const std::vector<NormalSearch>& normal_search = {},
                                           bool return_max_gap = false, bool return_counts = false,
                                           bool return_normals = false) {
    const size_t b = clouds.size();
    if (normals.size() != b || params.size() != b || (!normal_search.empty() && normal_search.size() != b))
      throw std::invalid_argument("teaser::BoundaryDetector: one entry per cloud in every argument");
    std::vector<const double*> pp(b), pn(b);
    std::vector<int32_t> n(b), nb(b, 0);
    std::vector<double> thr(b);
    std::vector<teaser_icp_normal_search_c> rec(b), nrec(b);
    std::vector<BoundaryResult> out(b);
    std::vector<uint8_t*> pm(b);
    std::vector<double*> pg(b), po(b);
    std::vector<int32_t*> pc(b);
    for (size_t c = 0; c < b; ++c) {
      const int64_t cols = clouds[c].cols();
      if (normals[c].cols() != 0 && normals[c].cols() != cols)
        throw std::invalid_argument("teaser::BoundaryDetector: as many normals as points");
      pp[c] = clouds[c].data();
      pn[c] = normals[c].cols() != 0 ? normals[c].data() : nullptr;
      n[c] = (int32_t)cols;
      rec[c] = params[c].search.rec;
      thr[c] = params[c].angle_threshold;
      nrec[c] = normal_search.empty() ? NormalSearch().rec : normal_search[c].rec;
      out[c].mask.resize((size_t)cols);
      if (return_max_gap) out[c].max_gap.resize((size_t)cols);
      if (return_counts) out[c].counts.resize((size_t)cols);
      if (return_normals) out[c].normals = Matrix3X(3, cols);
      pm[c] = out[c].mask.data();
      pg[c] = out[c].max_gap.data();
      pc[c] = out[c].counts.data();
      po[c] = return_normals ? out[c].normals.data() : nullptr;
    }
    const int32_t rc = teaser_hip_icp_boundary_points_batch(
        h_, (int32_t)b, pp.data(), pn.data(), n.data(), rec.data(), nrec.data(), thr.data(), pm.data(), nb.data(),
        return_max_gap ? pg.data() : nullptr, return_counts ? pc.data() : nullptr, return_normals ? po.data() : nullptr);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::BoundaryDetector: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
    for (size_t c = 0; c < b; ++c) out[c].n_boundary = nb[c];
    return out;
  }

  BoundaryResult compute(const Matrix3X& cloud, const Matrix3X& normals, const BoundaryParams& params,
                         bool return_max_gap = false) {
    return std::move(computeBatch({cloud}, {normals}, {params}, {}, return_max_gap)[0]);
  }

  // teaser_hip_icp_set_option / _get_option: "fpfh_list_bytes", "knn_ring_cap" (include/teaser_hip.h); no value changes
  // a result
  void setOption(const std::string& name, int64_t value) {
    if (teaser_hip_icp_set_option(h_, name.c_str(), value) != TEASER_HIP_OK)
      throw ICPError(TEASER_HIP_ERR_BAD_ARG, std::string("teaser::BoundaryDetector: ") + teaser_hip_icp_last_error(h_));
  }
  int64_t getOption(const std::string& name) const {
    int64_t v = 0;
    if (teaser_hip_icp_get_option(h_, name.c_str(), &v) != TEASER_HIP_OK)
      throw ICPError(TEASER_HIP_ERR_BAD_ARG, std::string("teaser::BoundaryDetector: ") + teaser_hip_icp_last_error(h_));
    return v;
  }

 private:
  teaser_hip_icp* h_ = nullptr;
};

// Open3D's cloud.ComputeBoundaryPoints(radius, max_nn, angle_threshold) on a cloud with normals.
inline BoundaryResult computeBoundaryPoints(const Matrix3X& points, const Matrix3X& normals, const BoundaryParams& params) {
  BoundaryDetector d;
  return d.compute(points, normals, params);
}

}  // namespace teaser
