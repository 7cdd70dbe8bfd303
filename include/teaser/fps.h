// teaser/fps.h -- farthest-point down-sampling on the MI355X (Open3D's PointCloud::FarthestPointDownSample) over the C
// ABI (include/teaser_hip.h, "Farthest-point down-sampling", where the contract is written out).  Header-only.
//
// Clouds are teaser::Matrix3X as in teaser/icp.h.  A teaser::FarthestPointSampler object holds one ICP handle and is
// reusable but not re-entrant; the batched form takes many clouds in one call, each cloud's result identical to the
// same cloud run alone.  The samples come in the order of selection, the first being start_index; the loop runs as
// stated also for num_samples == n.  A failed call throws teaser::ICPError, the constructor too when no MI355X is
// visible (there is no CPU path).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "teaser/icp.h"

namespace teaser {

struct FarthestPointParams {
  int num_samples = 0;  // 0 .. n
  int start_index = 0;  // the first sample (0 .. n - 1 when num_samples > 0)
};

struct FarthestPointResult {
  std::vector<int> indices;        // the samples in the order of selection
  std::vector<double> sel_dist;    // per sample: its squared distance to the nearest earlier sample, +inf for the first
  std::vector<double> final_dist;  // per point: its squared distance to the nearest sample (empty when num_samples = 0)
};

class FarthestPointSampler {
 public:
  explicit FarthestPointSampler(int device = -1) {
    const int32_t rc = teaser_hip_icp_create(device, &h_);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::FarthestPointSampler: teaser_hip_icp_create failed (status " + std::to_string(rc) +
                             (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)" : ")"));
  }
  ~FarthestPointSampler() { teaser_hip_icp_destroy(h_); }
  FarthestPointSampler(const FarthestPointSampler&) = delete;
  FarthestPointSampler& operator=(const FarthestPointSampler&) = delete;

  std::vector<FarthestPointResult> sampleBatch(const std::vector<Matrix3X>& clouds,
                                               const std::vector<FarthestPointParams>& params) {
    const size_t b = clouds.size();
    if (params.size() != b) throw std::invalid_argument("teaser::FarthestPointSampler: one FarthestPointParams per cloud");
    static_assert(sizeof(int) == sizeof(int32_t), "indices are written in place");
    std::vector<const double*> p(b);
    std::vector<int32_t> n(b);
    std::vector<teaser_icp_fps_params_c> rec(b);
    std::vector<FarthestPointResult> res(b);
    std::vector<int32_t*> pi(b);
    std::vector<double*> ps(b), pf(b);
    for (size_t c = 0; c < b; ++c) {
      p[c] = clouds[c].data();
      n[c] = (int32_t)clouds[c].cols();
      rec[c].num_samples = params[c].num_samples;
      rec[c].start_index = params[c].start_index;
      const size_t k = params[c].num_samples > 0 ? (size_t)params[c].num_samples : 0;
      res[c].indices.resize(k);
      res[c].sel_dist.resize(k);
      res[c].final_dist.resize(k ? (size_t)n[c] : 0);
      pi[c] = k ? reinterpret_cast<int32_t*>(res[c].indices.data()) : nullptr;
      ps[c] = k ? res[c].sel_dist.data() : nullptr;
      pf[c] = k ? res[c].final_dist.data() : nullptr;
    }
    const int32_t rc = teaser_hip_icp_farthest_point_down_sample_batch(h_, (int32_t)b, p.data(), n.data(), rec.data(),
                                                                       pi.data(), ps.data(), pf.data());
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::FarthestPointSampler: status " + std::to_string(rc) + ": " +
                             teaser_hip_icp_last_error(h_));
    return res;
  }

  FarthestPointResult sample(const Matrix3X& cloud, int num_samples, int start_index = 0) {
    FarthestPointParams p;
    p.num_samples = num_samples, p.start_index = start_index;
    return sampleBatch({cloud}, {p})[0];
  }

  // teaser_hip_icp_set_option / _get_option: "fps_resident_max" (include/teaser_hip.h); no value changes a result
  void setOption(const char* name, int64_t value) {
    const int32_t rc = teaser_hip_icp_set_option(h_, name, value);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::FarthestPointSampler: status " + std::to_string(rc) + ": " +
                             teaser_hip_icp_last_error(h_));
  }
  int64_t getOption(const char* name) {
    int64_t v = 0;
    const int32_t rc = teaser_hip_icp_get_option(h_, name, &v);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::FarthestPointSampler: status " + std::to_string(rc) + ": " +
                             teaser_hip_icp_last_error(h_));
    return v;
  }

 private:
  teaser_hip_icp* h_ = nullptr;
};

// The points at `indices` of a cloud, in that order.
inline Matrix3X selectByIndex(const Matrix3X& cloud, const std::vector<int>& indices) {
  Matrix3X out(3, (int64_t)indices.size());
  for (size_t k = 0; k < indices.size(); ++k)
    for (int r = 0; r < 3; ++r) out(r, (int64_t)k) = cloud(r, indices[k]);
  return out;
}

// Open3D's form: the num_samples points, in the order of selection.  Each call creates a handle -- keep a
// teaser::FarthestPointSampler for repeated calls, for batches, or for the indices and the distances.
inline Matrix3X farthestPointDownSample(const Matrix3X& points, int num_samples, int start_index = 0) {
  FarthestPointSampler s;
  return selectByIndex(points, s.sample(points, num_samples, start_index).indices);
}

}  // namespace teaser
