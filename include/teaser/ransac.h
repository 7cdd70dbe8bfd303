// teaser/ransac.h -- RANSAC registration on correspondences on the GPU with the surface of
// open3d::pipelines::registration: RANSACConvergenceCriteria, CorrespondenceCheckerBasedOnEdgeLength,
// CorrespondenceCheckerBasedOnDistance and RegistrationRANSACBasedOnCorrespondence, plus a batched form.  The contract
// is written out in include/teaser_hip.h, "RANSAC registration on correspondences": a trial is a function of
// (seed, trial index) alone and the loop is Open3D's as one thread runs it, so a result depends neither on the batch
// nor on the launch sizes nor on the run.  Not offered, and refused by name: with_scaling, point-to-plane estimation
// inside RANSAC, the normal-angle checker.
// Header-only over the C ABI; there is no CPU path (no MI355X: RANSACError with TEASER_HIP_ERR_NO_DEVICE).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "teaser/handle.h"
#include "teaser/icp.h"
#include "teaser_hip.h"

namespace teaser {

// Open3D's RANSACConvergenceCriteria.
struct RANSACConvergenceCriteria {
  int max_iteration = 100000;
  double confidence = 0.999;
  RANSACConvergenceCriteria() = default;
  RANSACConvergenceCriteria(int max_iteration_, double confidence_)
      : max_iteration(max_iteration_), confidence(confidence_) {}
};

// Open3D's checkers; a problem takes at most one of each kind.
struct CorrespondenceCheckerBasedOnEdgeLength {
  double similarity_threshold = 0.9;
  CorrespondenceCheckerBasedOnEdgeLength() = default;
  explicit CorrespondenceCheckerBasedOnEdgeLength(double s) : similarity_threshold(s) {}
};
struct CorrespondenceCheckerBasedOnDistance {
  double distance_threshold;
  explicit CorrespondenceCheckerBasedOnDistance(double d) : distance_threshold(d) {}
};

// (source index, target index), used in the caller's order; repeats allowed.
using CorrespondenceSet = std::vector<std::pair<int, int>>;

// One problem's settings.  with_scaling exists to be refused by name (TransformationEstimationPointToPoint(true)).
struct RANSACOption {
  double max_correspondence_distance = 0.0;  // required
  int ransac_n = 3;
  RANSACConvergenceCriteria criteria;
  uint64_t seed = 0;  // 0: from the clock
  const CorrespondenceCheckerBasedOnEdgeLength* edge_length = nullptr;
  const CorrespondenceCheckerBasedOnDistance* distance = nullptr;
  bool with_scaling = false;
};

// Open3D's RegistrationResult plus the trial counters of the contract.
struct RANSACResult {
  Matrix4 transformation;
  double fitness = 0;
  double inlier_rmse = 0;
  CorrespondenceSet correspondence_set;  // the inlier pairs, in input order
  int64_t best_trial = -1, trials = 0, valid_trials = 0;
  teaser_ransac_result_c record{};
};

class RANSACError : public std::runtime_error {
 public:
  RANSACError(int32_t status, const std::string& what) : std::runtime_error(what), status_(status) {}
  int32_t status() const { return status_; }

 private:
  int32_t status_;
};

class RANSAC {
 public:
  // Every problem in one call; result b is the bits problem b gives alone.  option: one for all, or one per problem.
  std::vector<RANSACResult> registrationRANSACBasedOnCorrespondenceBatch(const std::vector<Matrix3X>& src,
                                                                        const std::vector<Matrix3X>& dst,
                                                                        const std::vector<CorrespondenceSet>& corres,
                                                                        const std::vector<RANSACOption>& option) {
    const size_t B = src.size();
    if (dst.size() != B || corres.size() != B || (option.size() != 1 && option.size() != B))
      throw std::invalid_argument("registrationRANSACBasedOnCorrespondenceBatch: src, dst, corres of one length and "
                                  "one option, or one per problem");
    std::vector<const double*> ps(B), pd(B);
    std::vector<const int32_t*> pc(B);
    std::vector<int32_t> ns(B), nd(B), nc(B);
    std::vector<std::vector<int32_t>> flat(B), inl(B);
    std::vector<int32_t*> pi(B);
    std::vector<teaser_ransac_params_c> prm(B);
    for (size_t b = 0; b < B; ++b) {
      const RANSACOption& o = option[option.size() == 1 ? 0 : b];
      teaser_hip_ransac_params_default(&prm[b]);
      prm[b].max_correspondence_distance = o.max_correspondence_distance;
      prm[b].ransac_n = o.ransac_n;
      prm[b].max_iteration = o.criteria.max_iteration;
      prm[b].confidence = o.criteria.confidence;
      prm[b].seed = o.seed;
      prm[b].with_scaling = o.with_scaling ? 1 : 0;
      if (o.edge_length) {
        if (!(o.edge_length->similarity_threshold > 0))
          throw std::invalid_argument("CorrespondenceCheckerBasedOnEdgeLength: similarity_threshold must be > 0");
        prm[b].edge_length_threshold = o.edge_length->similarity_threshold;
      }
      if (o.distance) {
        if (!(o.distance->distance_threshold > 0))
          throw std::invalid_argument("CorrespondenceCheckerBasedOnDistance: distance_threshold must be > 0");
        prm[b].distance_threshold = o.distance->distance_threshold;
      }
      ps[b] = src[b].data();
      pd[b] = dst[b].data();
      ns[b] = (int32_t)src[b].cols();
      nd[b] = (int32_t)dst[b].cols();
      nc[b] = (int32_t)corres[b].size();
      flat[b].reserve(2 * corres[b].size() + 2);
      for (const auto& c : corres[b]) {
        flat[b].push_back(c.first);
        flat[b].push_back(c.second);
      }
      inl[b].assign(2 * corres[b].size() + 2, 0);
      pc[b] = flat[b].data();
      pi[b] = inl[b].data();
    }
    std::vector<teaser_ransac_result_c> rec(B);
    h_.create("teaser::RANSAC");
    const int32_t rc = teaser_hip_ransac_correspondence_batch(h_, (int32_t)B, ps.data(), ns.data(), pd.data(), nd.data(),
                                                              pc.data(), nc.data(), prm.data(), rec.data(), pi.data());
    if (rc != TEASER_HIP_OK)
      throw RANSACError(rc, std::string("registrationRANSACBasedOnCorrespondence: ") + teaser_hip_ransac_last_error(h_));
    std::vector<RANSACResult> out(B);
    for (size_t b = 0; b < B; ++b) {
      RANSACResult& r = out[b];
      r.record = rec[b];
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) r.transformation(i, j) = rec[b].transformation[4 * i + j];
      r.fitness = rec[b].fitness;
      r.inlier_rmse = rec[b].inlier_rmse;
      r.best_trial = rec[b].best_trial;
      r.trials = rec[b].trials;
      r.valid_trials = rec[b].valid_trials;
      for (int k = 0; k < rec[b].n_correspondences; ++k)
        r.correspondence_set.emplace_back(inl[b][(size_t)(2 * k)], inl[b][(size_t)(2 * k + 1)]);
    }
    return out;
  }

  RANSACResult registrationRANSACBasedOnCorrespondence(const Matrix3X& src, const Matrix3X& dst,
                                                       const CorrespondenceSet& corres, const RANSACOption& option) {
    return registrationRANSACBasedOnCorrespondenceBatch({src}, {dst}, {corres}, {option})[0];
  }

 private:
  detail::LazyRansac h_;
};

// Open3D's argument order; a temporary RANSAC object serves the call.
inline RANSACResult registrationRANSACBasedOnCorrespondence(const Matrix3X& src, const Matrix3X& dst,
                                                            const CorrespondenceSet& corres,
                                                            double max_correspondence_distance, int ransac_n = 3,
                                                            const CorrespondenceCheckerBasedOnEdgeLength* edge_length = nullptr,
                                                            const CorrespondenceCheckerBasedOnDistance* distance = nullptr,
                                                            const RANSACConvergenceCriteria& criteria = RANSACConvergenceCriteria(),
                                                            uint64_t seed = 0) {
  RANSACOption o;
  o.max_correspondence_distance = max_correspondence_distance;
  o.ransac_n = ransac_n;
  o.criteria = criteria;
  o.seed = seed;
  o.edge_length = edge_length;
  o.distance = distance;
  RANSAC r;
  return r.registrationRANSACBasedOnCorrespondence(src, dst, corres, o);
}

inline std::vector<RANSACResult> registrationRANSACBasedOnCorrespondenceBatch(const std::vector<Matrix3X>& src,
                                                                             const std::vector<Matrix3X>& dst,
                                                                             const std::vector<CorrespondenceSet>& corres,
                                                                             const std::vector<RANSACOption>& option) {
  RANSAC r;
  return r.registrationRANSACBasedOnCorrespondenceBatch(src, dst, corres, option);
}

}  // namespace teaser
