// teaser/plane.h -- dominant-plane segmentation on the GPU with the surface of open3d::geometry::PointCloud::
// SegmentPlane, plus a batched form.  The contract is written out in include/teaser_hip.h, "Plane segmentation": a trial
// is a function of (seed, trial index) alone, every sum has a fixed order and the loop is Open3D's as one thread runs
// it, so a result depends neither on the batch nor on the launch sizes nor on the run.  It departs from Open3D in three
// stated places: sampling with replacement, a double-valued stopping bound, the fixed summation order.
// Header-only over the C ABI; there is no CPU path (no MI355X: PlaneError with TEASER_HIP_ERR_NO_DEVICE).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "teaser/handle.h"
#include "teaser/icp.h"
#include "teaser_hip.h"

namespace teaser {

// One problem's settings; the defaults are Open3D's.
struct PlaneOption {
  double distance_threshold = 0.0;  // required
  int ransac_n = 3;
  int num_iterations = 100;
  double probability = 0.99999999;
  uint64_t seed = 0;  // 0: from the clock
};

// Open3D's (plane_model, inliers) plus the mask, the winning trial's score and the trial counters of the contract.
struct PlaneResult {
  double plane_model[4] = {0, 0, 0, 0};  // a x + b y + c z + d = 0
  std::vector<int> inliers;              // ascending
  std::vector<uint8_t> mask;             // one byte per point
  double fitness = 0;
  double inlier_rmse = 0;
  int64_t best_trial = -1, trials = 0, valid_trials = 0;
  teaser_plane_result_c record{};
};

class PlaneError : public std::runtime_error {
 public:
  PlaneError(int32_t status, const std::string& what) : std::runtime_error(what), status_(status) {}
  int32_t status() const { return status_; }

 private:
  int32_t status_;
};

class PlaneSegmenter {
 public:
  // Every cloud in one call; result b is the bits cloud b gives alone.  option: one for all, or one per problem.
  std::vector<PlaneResult> segmentPlaneBatch(const std::vector<Matrix3X>& clouds, const std::vector<PlaneOption>& option) {
    const size_t B = clouds.size();
    if (option.size() != 1 && option.size() != B)
      throw std::invalid_argument("segmentPlaneBatch: one option, or one per problem");
    std::vector<const double*> pp(B);
    std::vector<int32_t> n(B);
    std::vector<std::vector<int32_t>> inl(B);
    std::vector<int32_t*> pi(B);
    std::vector<uint8_t*> pm(B);
    std::vector<teaser_plane_params_c> prm(B);
    std::vector<PlaneResult> out(B);
    for (size_t b = 0; b < B; ++b) {
      const PlaneOption& o = option[option.size() == 1 ? 0 : b];
      teaser_hip_plane_params_default(&prm[b]);
      prm[b].distance_threshold = o.distance_threshold;
      prm[b].ransac_n = o.ransac_n;
      prm[b].num_iterations = o.num_iterations;
      prm[b].probability = o.probability;
      prm[b].seed = o.seed;
      pp[b] = clouds[b].data();
      n[b] = (int32_t)clouds[b].cols();
      inl[b].assign((size_t)clouds[b].cols() + 1, 0);
      out[b].mask.assign((size_t)clouds[b].cols() + 1, 0);
      pi[b] = inl[b].data();
      pm[b] = out[b].mask.data();
    }
    std::vector<teaser_plane_result_c> rec(B);
    h_.create("teaser::PlaneSegmenter");
    const int32_t rc = teaser_hip_plane_segment_batch(h_, (int32_t)B, pp.data(), n.data(), prm.data(), rec.data(),
                                                      pi.data(), pm.data());
    if (rc != TEASER_HIP_OK) throw PlaneError(rc, std::string("segmentPlane: ") + teaser_hip_plane_last_error(h_));
    for (size_t b = 0; b < B; ++b) {
      PlaneResult& r = out[b];
      r.record = rec[b];
      for (int k = 0; k < 4; ++k) r.plane_model[k] = rec[b].plane[k];
      r.fitness = rec[b].fitness;
      r.inlier_rmse = rec[b].inlier_rmse;
      r.best_trial = rec[b].best_trial;
      r.trials = rec[b].trials;
      r.valid_trials = rec[b].valid_trials;
      r.inliers.assign(inl[b].begin(), inl[b].begin() + rec[b].n_inliers);
      r.mask.resize((size_t)clouds[b].cols());
    }
    return out;
  }

  PlaneResult segmentPlane(const Matrix3X& cloud, const PlaneOption& option) {
    return segmentPlaneBatch({cloud}, {option})[0];
  }

 private:
  detail::LazyPlane h_;
};

// Open3D's argument order plus the seed; a temporary PlaneSegmenter serves the call.
inline PlaneResult segmentPlane(const Matrix3X& cloud, double distance_threshold, int ransac_n = 3,
                                int num_iterations = 100, double probability = 0.99999999, uint64_t seed = 0) {
  PlaneOption o;
  o.distance_threshold = distance_threshold;
  o.ransac_n = ransac_n;
  o.num_iterations = num_iterations;
  o.probability = probability;
  o.seed = seed;
  PlaneSegmenter s;
  return s.segmentPlane(cloud, o);
}

inline std::vector<PlaneResult> segmentPlaneBatch(const std::vector<Matrix3X>& clouds,
                                                  const std::vector<PlaneOption>& option) {
  PlaneSegmenter s;
  return s.segmentPlaneBatch(clouds, option);
}

}  // namespace teaser
