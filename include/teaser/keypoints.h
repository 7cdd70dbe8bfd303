// teaser/keypoints.h -- ISS keypoint detection on the MI355X (Open3D's compute_iss_keypoints, PCL's ISSKeypoint3D)
// over the C ABI (include/teaser_hip.h, "ISS keypoints", where the contract is written out).  Header-only.
//
// Clouds are teaser::Matrix3X as in teaser/icp.h.  A teaser::ISSKeypoints object holds one ICP handle and is reusable
// but not re-entrant; the batched form takes many clouds in one launch sequence, each cloud's result identical to the
// same cloud run alone.  Keypoint indices come in ascending order.  A failed call throws teaser::ICPError, the
// constructor too when no MI355X is visible (there is no CPU path).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "teaser/icp.h"

namespace teaser {

// Open3D's parameters and defaults; a radius of 0 (in either field) takes both radii from the cloud's resolution.
struct ISSParams {
  double salient_radius = 0.0;
  double non_max_radius = 0.0;
  double gamma_21 = 0.975;
  double gamma_32 = 0.975;
  int min_neighbors = 5;
};

struct ISSResult {
  std::vector<int> indices;      // the keypoints, ascending
  std::vector<double> saliency;  // per point: the smallest eigenvalue where both ratio tests pass, else 0
  std::vector<int32_t> counts;   // n x 2: neighbours inside salient_radius and inside non_max_radius (point included)
  double resolution = 0;         // NaN when the radii were given
  double salient_radius = 0, non_max_radius = 0;  // as used
};

class ISSKeypoints {
 public:
  explicit ISSKeypoints(int device = -1) {
    const int32_t rc = teaser_hip_icp_create(device, &h_);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::ISSKeypoints: teaser_hip_icp_create failed (status " + std::to_string(rc) +
                             (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)" : ")"));
  }
  ~ISSKeypoints() { teaser_hip_icp_destroy(h_); }
  ISSKeypoints(const ISSKeypoints&) = delete;
  ISSKeypoints& operator=(const ISSKeypoints&) = delete;

  std::vector<ISSResult> computeBatch(const std::vector<Matrix3X>& clouds, const std::vector<ISSParams>& params) {
    const size_t b = clouds.size();
    if (params.size() != b) throw std::invalid_argument("teaser::ISSKeypoints: one ISSParams per cloud");
    std::vector<const double*> p(b);
    std::vector<int32_t> n(b), kept(b);
    std::vector<teaser_icp_iss_params_c> rec(b);
    std::vector<ISSResult> res(b);
    std::vector<std::vector<uint8_t>> keep(b);
    std::vector<uint8_t*> pk(b);
    std::vector<double*> ps(b);
    std::vector<int32_t*> pc(b);
    std::vector<double> radii(3 * b);
    for (size_t c = 0; c < b; ++c) {
      p[c] = clouds[c].data();
      n[c] = (int32_t)clouds[c].cols();
      teaser_hip_icp_iss_params_default(&rec[c]);
      rec[c].salient_radius = params[c].salient_radius;
      rec[c].non_max_radius = params[c].non_max_radius;
      rec[c].gamma_21 = params[c].gamma_21;
      rec[c].gamma_32 = params[c].gamma_32;
      rec[c].min_neighbors = params[c].min_neighbors;
      keep[c].resize((size_t)n[c] + 1);
      res[c].saliency.resize((size_t)n[c]);
      res[c].counts.resize(2 * (size_t)n[c]);
      pk[c] = keep[c].data();
      ps[c] = n[c] ? res[c].saliency.data() : nullptr;
      pc[c] = n[c] ? res[c].counts.data() : nullptr;
    }
    const int32_t rc = teaser_hip_icp_iss_keypoints_batch(h_, (int32_t)b, p.data(), n.data(), rec.data(), pk.data(),
                                                          kept.data(), ps.data(), pc.data(), radii.data());
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::ISSKeypoints: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
    for (size_t c = 0; c < b; ++c) {
      res[c].indices.reserve((size_t)(kept[c] > 0 ? kept[c] : 0));
      for (int32_t i = 0; i < n[c]; ++i)
        if (keep[c][(size_t)i]) res[c].indices.push_back(i);
      res[c].resolution = radii[3 * c];
      res[c].salient_radius = radii[3 * c + 1];
      res[c].non_max_radius = radii[3 * c + 2];
    }
    return res;
  }

  ISSResult compute(const Matrix3X& cloud, const ISSParams& params = ISSParams()) {
    return computeBatch({cloud}, {params})[0];
  }

 private:
  teaser_hip_icp* h_ = nullptr;
};

// Open3D's free-function forms: the keypoint indices in ascending order.  Each call creates a handle -- keep a
// teaser::ISSKeypoints for repeated calls, or for the saliencies, counts and radii.
inline std::vector<int> computeISSKeypoints(const Matrix3X& cloud, const ISSParams& params = ISSParams()) {
  ISSKeypoints k;
  return k.compute(cloud, params).indices;
}
inline std::vector<std::vector<int>> computeISSKeypointsBatch(const std::vector<Matrix3X>& clouds,
                                                              const std::vector<ISSParams>& params) {
  ISSKeypoints k;
  std::vector<std::vector<int>> out;
  for (ISSResult& r : k.computeBatch(clouds, params)) out.push_back(std::move(r.indices));
  return out;
}

}  // namespace teaser
