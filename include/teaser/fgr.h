// teaser/fgr.h -- Fast Global Registration on correspondences on the GPU with the surface of
// open3d::pipelines::registration: FastGlobalRegistrationOption and FastGlobalRegistrationBasedOnCorrespondence, plus a
// batched form.  The contract is written out in include/teaser_hip.h, "Fast Global Registration on correspondences":
// every sum has a fixed order, so a result depends neither on the batch nor on the route nor on the run.
// Header-only over the C ABI; there is no CPU path (no MI355X: FGRError with TEASER_HIP_ERR_NO_DEVICE).
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

// Open3D's FastGlobalRegistrationOption, same fields and defaults, plus seed (the tuple test's draw; 0: from the
// clock).  maximum_tuple_count is NOT applied: the project's tuple test keeps every passing triple.
struct FastGlobalRegistrationOption {
  double division_factor = 1.4;
  bool use_absolute_scale = false;
  bool decrease_mu = true;
  double maximum_correspondence_distance = 0.025;
  int iteration_number = 64;
  double tuple_scale = 0.95;
  int maximum_tuple_count = 1000;
  bool tuple_test = true;
  uint64_t seed = 0;
};

// Open3D's RegistrationResult (filled by evaluateRegistration at the FGR pose and maximum_correspondence_distance, as
// Open3D does) plus the record of the contract and the pairs the solve ran on.
struct FGRResult {
  Matrix4 transformation;
  double fitness = 0;
  double inlier_rmse = 0;
  std::vector<std::pair<int, int>> correspondence_set;
  std::vector<std::pair<int, int>> fgr_corres;  // after the tuple test
  teaser_fgr_result_c record{};
};

class FGRError : public std::runtime_error {
 public:
  FGRError(int32_t status, const std::string& what) : std::runtime_error(what), status_(status) {}
  int32_t status() const { return status_; }

 private:
  int32_t status_;
};

class FGR {
 public:
  using CorrespondenceSet = std::vector<std::pair<int, int>>;

  // Every problem in one call; result b is the bits problem b gives alone.  option: one for all, or one per problem.
  std::vector<FGRResult> registrationFGRBasedOnCorrespondenceBatch(const std::vector<Matrix3X>& src,
                                                                  const std::vector<Matrix3X>& dst,
                                                                  const std::vector<CorrespondenceSet>& corres,
                                                                  const std::vector<FastGlobalRegistrationOption>& option) {
    const size_t B = src.size();
    if (dst.size() != B || corres.size() != B || (option.size() != 1 && option.size() != B))
      throw std::invalid_argument("registrationFGRBasedOnCorrespondenceBatch: src, dst, corres of one length and one "
                                  "option, or one per problem");
    if (B == 0) return {};
    auto opt = [&](size_t b) -> const FastGlobalRegistrationOption& { return option[option.size() == 1 ? 0 : b]; };
    std::vector<std::vector<int32_t>> flat(B);
    for (size_t b = 0; b < B; ++b) {
      flat[b].reserve(2 * corres[b].size() + 2);
      for (const auto& c : corres[b]) {
        flat[b].push_back(c.first);
        flat[b].push_back(c.second);
      }
    }
    tupleTest(src, dst, opt, flat);
    std::vector<const double*> ps(B), pd(B);
    std::vector<const int32_t*> pc(B);
    std::vector<int32_t> ns(B), nd(B), nc(B);
    std::vector<teaser_fgr_params_c> prm(B);
    for (size_t b = 0; b < B; ++b) {
      const FastGlobalRegistrationOption& o = opt(b);
      teaser_hip_fgr_params_default(&prm[b]);
      prm[b].division_factor = o.division_factor;
      prm[b].maximum_correspondence_distance = o.maximum_correspondence_distance;
      prm[b].use_absolute_scale = o.use_absolute_scale ? 1 : 0;
      prm[b].decrease_mu = o.decrease_mu ? 1 : 0;
      prm[b].iteration_number = o.iteration_number;
      ps[b] = src[b].data();
      pd[b] = dst[b].data();
      ns[b] = (int32_t)src[b].cols();
      nd[b] = (int32_t)dst[b].cols();
      nc[b] = (int32_t)(flat[b].size() / 2);
      flat[b].push_back(0);  // never an empty vector's data()
      pc[b] = flat[b].data();
    }
    std::vector<teaser_fgr_result_c> rec(B);
    h_.create("teaser::FGR");
    const int32_t rc = teaser_hip_fgr_correspondence_batch(h_, (int32_t)B, ps.data(), ns.data(), pd.data(), nd.data(),
                                                           pc.data(), nc.data(), prm.data(), rec.data());
    if (rc != TEASER_HIP_OK)
      throw FGRError(rc, std::string("registrationFGRBasedOnCorrespondence: ") + teaser_hip_fgr_last_error(h_));
    std::vector<Matrix4> T(B);
    std::vector<double> radius(B);
    for (size_t b = 0; b < B; ++b) {
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) T[b](i, j) = rec[b].transformation[4 * i + j];
      radius[b] = opt(b).maximum_correspondence_distance;
    }
    const std::vector<ICPResult> ev = icp_.evaluateRegistrationBatch(src, dst, radius, T);
    std::vector<FGRResult> out(B);
    for (size_t b = 0; b < B; ++b) {
      FGRResult& r = out[b];
      r.record = rec[b];
      r.transformation = T[b];
      r.fitness = ev[b].fitness;
      r.inlier_rmse = ev[b].inlier_rmse;
      r.correspondence_set = ev[b].correspondence_set;
      for (int32_t k = 0; k < nc[b]; ++k) r.fgr_corres.emplace_back(flat[b][(size_t)(2 * k)], flat[b][(size_t)(2 * k + 1)]);
    }
    return out;
  }

  FGRResult registrationFGRBasedOnCorrespondence(const Matrix3X& src, const Matrix3X& dst,
                                                 const CorrespondenceSet& corres,
                                                 const FastGlobalRegistrationOption& option) {
    return registrationFGRBasedOnCorrespondenceBatch({src}, {dst}, {corres}, {option})[0];
  }

 private:
  // option.tuple_test: the batched tuple test (teaser_hip_features_tuple_test_batch) on the problems that ask for it.
  template <class Opt>
  void tupleTest(const std::vector<Matrix3X>& src, const std::vector<Matrix3X>& dst, Opt opt,
                 std::vector<std::vector<int32_t>>& flat) {
    std::vector<size_t> which;
    for (size_t b = 0; b < flat.size(); ++b)
      if (opt(b).tuple_test && !flat[b].empty()) which.push_back(b);
    if (which.empty()) return;
    const size_t W = which.size();
    std::vector<std::vector<float>> fs(W), fd(W);
    std::vector<const float*> ps(W), pd(W);
    std::vector<int32_t*> pp(W);
    std::vector<int32_t> ns(W), nd(W);
    std::vector<int64_t> np(W);
    std::vector<float> scale(W);
    std::vector<uint64_t> seed(W);
    for (size_t w = 0; w < W; ++w) {
      const size_t b = which[w];
      fs[w].assign(src[b].data(), src[b].data() + 3 * src[b].cols());
      fd[w].assign(dst[b].data(), dst[b].data() + 3 * dst[b].cols());
      fs[w].push_back(0.0f);
      fd[w].push_back(0.0f);
      ps[w] = fs[w].data();
      pd[w] = fd[w].data();
      ns[w] = (int32_t)src[b].cols();
      nd[w] = (int32_t)dst[b].cols();
      pp[w] = flat[b].data();
      np[w] = (int64_t)(flat[b].size() / 2);
      scale[w] = (float)opt(b).tuple_scale;
      seed[w] = opt(b).seed;
    }
    fh_.create("teaser::FGR");
    const int32_t rc = teaser_hip_features_tuple_test_batch(fh_, (int32_t)W, ps.data(), ns.data(), pd.data(), nd.data(),
                                                            scale.data(), seed.data(), pp.data(), np.data());
    if (rc != TEASER_HIP_OK)
      throw FGRError(rc, std::string("registrationFGRBasedOnCorrespondence (tuple test): ") +
                             teaser_hip_features_last_error(fh_));
    for (size_t w = 0; w < W; ++w) flat[which[w]].resize((size_t)(2 * np[w]));
  }

  detail::LazyFeatures fh_;
  detail::LazyFgr h_;
  ICP icp_;
};

// Open3D's argument order; a temporary FGR object serves the call.
inline FGRResult registrationFGRBasedOnCorrespondence(const Matrix3X& src, const Matrix3X& dst,
                                                      const std::vector<std::pair<int, int>>& corres,
                                                      const FastGlobalRegistrationOption& option =
                                                          FastGlobalRegistrationOption()) {
  FGR f;
  return f.registrationFGRBasedOnCorrespondence(src, dst, corres, option);
}

inline std::vector<FGRResult> registrationFGRBasedOnCorrespondenceBatch(
    const std::vector<Matrix3X>& src, const std::vector<Matrix3X>& dst,
    const std::vector<std::vector<std::pair<int, int>>>& corres,
    const std::vector<FastGlobalRegistrationOption>& option) {
  FGR f;
  return f.registrationFGRBasedOnCorrespondenceBatch(src, dst, corres, option);
}

}  // namespace teaser
