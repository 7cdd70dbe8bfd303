// teaser/matcher.h -- drop-in for the reference's teaser/include/teaser/matcher.h (teaser::Matcher,
// reference matcher.h:20-61, teaser/src/matcher.cc:21-301) over the MI355X C ABI (teaser_hip_match_features).
//
// The reference searches two FLANN kd-trees (exact L2 1-NN in 33 dimensions, matcher.cc:140-170); here both
// searches are brute-force distance tiles on the GPU, the index bookkeeping (initial matching, cross check,
// swap, sort + unique: matcher.cc:155-296) is the same.  The tuple constraint (matcher.cc:223-283) is host
// arithmetic behind teaser_hip_tuple_test for one pair and one launch sequence for all pairs of a batched call
// (tupleTestBatch, teaser_hip_features_tuple_test_batch: the same results for the same seed): like the reference it
// draws its triples from a generator seeded with the clock unless a seed is given (the result is not reproducible, by
// the reference's construction); the reference's normalizePoints (matcher.cc:57-116) moves and scales both clouds
// alike, which the ratio test cannot see.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "teaser/fpfh.h"
#include "teaser/geometry.h"
#include "teaser/handle.h"
#include "teaser_hip.h"

namespace teaser {

class Matcher {
 public:
  Matcher() = default;
  Matcher(const Matcher&) = delete;
  Matcher& operator=(const Matcher&) = delete;

  // matcher.h:40-44: (source index, target index) pairs, sorted, unique
  std::vector<std::pair<int, int>> calculateCorrespondences(const PointCloud& source_points,
                                                            const PointCloud& target_points,
                                                            const FPFHCloud& source_features,
                                                            const FPFHCloud& target_features,
                                                            bool use_absolute_scale = true, bool use_crosscheck = true,
                                                            bool use_tuple_test = true, float tuple_scale = 0) {
    (void)use_absolute_scale;
    h_.create("teaser::Matcher");
    static_assert(sizeof(std::pair<int, int>) == 8, "packed pairs expected");
    std::vector<std::pair<int, int>> out(source_features.size() + target_features.size() + 1);
    int64_t cnt = (int64_t)out.size();
    const int32_t rc = teaser_hip_match_features(
        h_, reinterpret_cast<const float*>(source_features.data()), (int32_t)source_features.size(),
        reinterpret_cast<const float*>(target_features.data()), (int32_t)target_features.size(), 33,
        use_crosscheck ? 1 : 0, reinterpret_cast<int32_t*>(out.data()), &cnt);
    if (rc != TEASER_HIP_OK)
      throw std::runtime_error(std::string("teaser_hip_match_features status ") + std::to_string(rc) + ": " +
                               teaser_hip_last_error(h_));
    if (use_tuple_test && tuple_scale != 0) {  // matcher.cc:223
      static_assert(sizeof(PointXYZ) == 12, "teaser::PointXYZ is three floats");
      const int32_t rt = teaser_hip_tuple_test(
          h_, reinterpret_cast<const float*>(source_points.data()), (int32_t)source_points.size(),
          reinterpret_cast<const float*>(target_points.data()), (int32_t)target_points.size(), tuple_scale, /*seed=*/0,
          reinterpret_cast<int32_t*>(out.data()), &cnt);
      if (rt != TEASER_HIP_OK) throw std::runtime_error("teaser_hip_tuple_test status " + std::to_string(rt));
    }
    out.resize((size_t)cnt);
    return out;
  }

  // The tuple constraint (matcher.cc:223-283) on the correspondences of many pairs in one launch sequence
  // (teaser_hip_features_tuple_test_batch; contract in teaser_hip.h, "tuple_test_batch"): per pair the surviving
  // correspondences, sorted and unique -- for tuple_seed != 0 exactly what teaser_hip_tuple_test returns for that pair
  // and seed; tuple_seed = 0 seeds from the clock like the reference.  tuple_scale <= 0 returns the lists untouched.
  std::vector<std::vector<std::pair<int, int>>> tupleTestBatch(
      const std::vector<PointCloud>& source_points, const std::vector<PointCloud>& target_points,
      std::vector<std::vector<std::pair<int, int>>> correspondences, float tuple_scale, uint64_t tuple_seed = 0) {
    const size_t batch = correspondences.size();
    if (source_points.size() != batch || target_points.size() != batch)
      throw std::invalid_argument("teaser::Matcher::tupleTestBatch: lists of different lengths");
    fh_.create("teaser::Matcher");
    static_assert(sizeof(std::pair<int, int>) == 8, "packed pairs expected");
    static_assert(sizeof(PointXYZ) == 12, "teaser::PointXYZ is three floats");
    std::vector<const float*> ps(batch), pt(batch);
    std::vector<int32_t*> pairs(batch);
    std::vector<int32_t> ns(batch), nt(batch);
    std::vector<int64_t> cnt(batch);
    const std::vector<float> scale(batch, tuple_scale);
    const std::vector<uint64_t> seed(batch, tuple_seed);
    for (size_t b = 0; b < batch; ++b) {
      ns[b] = (int32_t)source_points[b].size();
      nt[b] = (int32_t)target_points[b].size();
      ps[b] = reinterpret_cast<const float*>(source_points[b].data());
      pt[b] = reinterpret_cast<const float*>(target_points[b].data());
      pairs[b] = reinterpret_cast<int32_t*>(correspondences[b].data());
      cnt[b] = (int64_t)correspondences[b].size();
    }
    const int32_t rc = teaser_hip_features_tuple_test_batch(fh_, (int32_t)batch, ps.data(), ns.data(), pt.data(),
                                                            nt.data(), scale.data(), seed.data(), pairs.data(),
                                                            cnt.data());
    if (rc != TEASER_HIP_OK)
      throw std::runtime_error(std::string("teaser_hip_features_tuple_test_batch status ") + std::to_string(rc) + ": " +
                               teaser_hip_features_last_error(fh_));
    for (size_t b = 0; b < batch; ++b) correspondences[b].resize((size_t)cnt[b]);
    return correspondences;
  }

  // calculateCorrespondences for many pairs in one launch sequence (teaser_hip_features_match_batch; no counterpart
  // in the reference): per pair the list one call per pair returns.  The tuple test, when asked for, is one more
  // launch sequence for all pairs (tupleTestBatch).
  std::vector<std::vector<std::pair<int, int>>> calculateCorrespondencesBatch(
      const std::vector<PointCloud>& source_points, const std::vector<PointCloud>& target_points,
      const std::vector<FPFHCloud>& source_features, const std::vector<FPFHCloud>& target_features,
      bool use_absolute_scale = true, bool use_crosscheck = true, bool use_tuple_test = true, float tuple_scale = 0) {
    (void)use_absolute_scale;
    const size_t batch = source_features.size();
    const bool tuple = use_tuple_test && tuple_scale != 0;
    if (target_features.size() != batch || (tuple && (source_points.size() != batch || target_points.size() != batch)))
      throw std::invalid_argument("teaser::Matcher::calculateCorrespondencesBatch: lists of different lengths");
    fh_.create("teaser::Matcher");
    std::vector<std::vector<std::pair<int, int>>> out(batch);
    std::vector<const float*> fs(batch), ft(batch);
    std::vector<int32_t*> pairs(batch);
    std::vector<int32_t> ns(batch), nt(batch);
    std::vector<int64_t> cap(batch), cnt(batch, 0);
    for (size_t b = 0; b < batch; ++b) {
      ns[b] = (int32_t)source_features[b].size();
      nt[b] = (int32_t)target_features[b].size();
      out[b].resize((size_t)ns[b] + (size_t)nt[b] + 1);
      cap[b] = (int64_t)out[b].size();
      fs[b] = reinterpret_cast<const float*>(source_features[b].data());
      ft[b] = reinterpret_cast<const float*>(target_features[b].data());
      pairs[b] = reinterpret_cast<int32_t*>(out[b].data());
    }
    const int32_t rc = teaser_hip_features_match_batch(fh_, (int32_t)batch, fs.data(), ns.data(), ft.data(), nt.data(),
                                                       33, use_crosscheck ? 1 : 0, pairs.data(), cap.data(),
                                                       cnt.data());
    if (rc != TEASER_HIP_OK)
      throw std::runtime_error(std::string("teaser_hip_features_match_batch status ") + std::to_string(rc) + ": " +
                               teaser_hip_features_last_error(fh_));
    for (size_t b = 0; b < batch; ++b) out[b].resize((size_t)cnt[b]);
    if (tuple) return tupleTestBatch(source_points, target_points, std::move(out), tuple_scale, /*tuple_seed=*/0);
    return out;
  }

  // The k nearest target descriptors of every source point (no counterpart in the reference library; its tutorial,
  // examples/teaser_python_fpfh_icp/helpers.py:19-43, does this with a host KD-tree): the sorted (source index,
  // target index) pairs (i, j) with j among the k nearest of i -- with `mutual` only those where i is also among
  // the k nearest of j.  k in [1, TEASER_HIP_FEATURES_KNN_MAX]; semantics in teaser_hip.h ("k nearest").
  // k = 1, mutual = true equals calculateCorrespondences(..., use_crosscheck = true, use_tuple_test = false).
  // tuple_scale != 0 applies the tuple constraint to the pairs (tupleTestBatch); it needs the points of both clouds.
  std::vector<std::pair<int, int>> calculateKnnCorrespondences(const FPFHCloud& source_features,
                                                               const FPFHCloud& target_features, int k,
                                                               bool mutual = true, float tuple_scale = 0,
                                                               uint64_t tuple_seed = 0,
                                                               const PointCloud& source_points = PointCloud(),
                                                               const PointCloud& target_points = PointCloud()) {
    if (tuple_scale == 0) return calculateKnnCorrespondencesBatch({source_features}, {target_features}, k, mutual)[0];
    return calculateKnnCorrespondencesBatch({source_features}, {target_features}, k, mutual, tuple_scale, tuple_seed,
                                            {source_points}, {target_points})[0];
  }

  // calculateKnnCorrespondences for many pairs in one launch sequence (teaser_hip_features_match_knn_batch, then
  // tupleTestBatch when tuple_scale != 0).
  std::vector<std::vector<std::pair<int, int>>> calculateKnnCorrespondencesBatch(
      const std::vector<FPFHCloud>& source_features, const std::vector<FPFHCloud>& target_features, int k,
      bool mutual = true, float tuple_scale = 0, uint64_t tuple_seed = 0,
      const std::vector<PointCloud>& source_points = std::vector<PointCloud>(),
      const std::vector<PointCloud>& target_points = std::vector<PointCloud>()) {
    const size_t batch = source_features.size();
    if (target_features.size() != batch ||
        (tuple_scale != 0 && (source_points.size() != batch || target_points.size() != batch)))
      throw std::invalid_argument("teaser::Matcher::calculateKnnCorrespondencesBatch: lists of different lengths");
    if (k < 1 || k > TEASER_HIP_FEATURES_KNN_MAX)
      throw std::invalid_argument("teaser::Matcher::calculateKnnCorrespondencesBatch: k must be in [1, " +
                                  std::to_string(TEASER_HIP_FEATURES_KNN_MAX) + "]");
    fh_.create("teaser::Matcher");
    static_assert(sizeof(std::pair<int, int>) == 8, "packed pairs expected");
    std::vector<std::vector<std::pair<int, int>>> out(batch);
    std::vector<const float*> fs(batch), ft(batch);
    std::vector<int32_t*> pairs(batch);
    std::vector<int32_t> ns(batch), nt(batch);
    std::vector<int64_t> cap(batch), cnt(batch, 0);
    for (size_t b = 0; b < batch; ++b) {
      ns[b] = (int32_t)source_features[b].size();
      nt[b] = (int32_t)target_features[b].size();
      out[b].resize((size_t)ns[b] * (size_t)(nt[b] < k ? nt[b] : k) + 1);
      cap[b] = (int64_t)out[b].size();
      fs[b] = reinterpret_cast<const float*>(source_features[b].data());
      ft[b] = reinterpret_cast<const float*>(target_features[b].data());
      pairs[b] = reinterpret_cast<int32_t*>(out[b].data());
    }
    const int32_t rc = teaser_hip_features_match_knn_batch(fh_, (int32_t)batch, fs.data(), ns.data(), ft.data(),
                                                           nt.data(), 33, k, mutual ? 1 : 0, pairs.data(), cap.data(),
                                                           cnt.data());
    if (rc != TEASER_HIP_OK)
      throw std::runtime_error(std::string("teaser_hip_features_match_knn_batch status ") + std::to_string(rc) + ": " +
                               teaser_hip_features_last_error(fh_));
    for (size_t b = 0; b < batch; ++b) out[b].resize((size_t)cnt[b]);
    if (tuple_scale != 0) return tupleTestBatch(source_points, target_points, std::move(out), tuple_scale, tuple_seed);
    return out;
  }

 private:
  detail::LazyFeatures fh_;  // (declared first: destroyed after the solver)
  detail::LazySolver h_;
};

}  // namespace teaser
