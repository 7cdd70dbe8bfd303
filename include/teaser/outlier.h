// teaser/outlier.h -- point-cloud cleaning on the MI355X: Open3D's remove_statistical_outlier and
// remove_radius_outlier, and the self k-NN search (no radius) the statistical rule is built on, over the C ABI
// (include/teaser_hip.h, "Self k-NN" and "Outlier removal", where the contracts are written out).
// Header-only.
//
// Clouds are teaser::Matrix3X as in teaser/icp.h.  A teaser::OutlierRemoval object holds one ICP handle and is
// reusable but not re-entrant; every call has a batched form (many clouds, one launch sequence, each cloud's result
// identical to the same cloud run alone) and a single-cloud form.  Kept indices come in ascending order.  A failed
// call throws teaser::ICPError, the constructor too when no MI355X is visible (there is no CPU path).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "teaser/icp.h"

namespace teaser {

struct StatisticalOutlierResult {
  std::vector<int> indices;  // the kept points, ascending
  std::vector<double> avg;   // per point: the mean distance to its nb_neighbors nearest (itself included)
  double mean = 0, std_dev = 0, threshold = 0;
};

struct RadiusOutlierResult {
  std::vector<int> indices;     // the kept points, ascending
  std::vector<int32_t> counts;  // per point: the points of the cloud (itself included) closer than the radius
};

struct SelfKnnResult {
  int k = 0;
  std::vector<int32_t> indices;    // n x k row-major, ascending (squared distance, index); unused slots -1
  std::vector<double> distances2;  // n x k squared distances; unused slots +inf
};

class OutlierRemoval {
 public:
  explicit OutlierRemoval(int device = -1) {
    const int32_t rc = teaser_hip_icp_create(device, &h_);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::OutlierRemoval: teaser_hip_icp_create failed (status " + std::to_string(rc) +
                             (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)" : ")"));
  }
  ~OutlierRemoval() { teaser_hip_icp_destroy(h_); }
  OutlierRemoval(const OutlierRemoval&) = delete;
  OutlierRemoval& operator=(const OutlierRemoval&) = delete;

  std::vector<StatisticalOutlierResult> removeStatisticalOutliersBatch(const std::vector<Matrix3X>& clouds,
                                                                       const std::vector<int>& nb_neighbors,
                                                                       const std::vector<double>& std_ratio) {
    const size_t b = clouds.size();
    if (nb_neighbors.size() != b || std_ratio.size() != b)
      throw std::invalid_argument("teaser::OutlierRemoval: one entry per cloud in every argument");
    Inputs in(clouds, nb_neighbors);
    std::vector<StatisticalOutlierResult> res(b);
    std::vector<std::vector<uint8_t>> keep(b);
    std::vector<uint8_t*> pk(b);
    std::vector<double*> pa(b);
    std::vector<int32_t> kept(b);
    std::vector<double> stats(3 * b);
    for (size_t c = 0; c < b; ++c) {
      keep[c].resize((size_t)in.n[c] + 1);
      res[c].avg.resize((size_t)in.n[c]);
      pk[c] = keep[c].data();
      pa[c] = in.n[c] ? res[c].avg.data() : nullptr;
    }
    check(teaser_hip_icp_remove_statistical_outliers_batch(h_, (int32_t)b, in.p.data(), in.n.data(), in.k.data(),
                                                           std_ratio.data(), pk.data(), kept.data(), pa.data(),
                                                           stats.data()));
    for (size_t c = 0; c < b; ++c) {
      res[c].indices = compact(keep[c], in.n[c], kept[c]);
      res[c].mean = stats[3 * c];
      res[c].std_dev = stats[3 * c + 1];
      res[c].threshold = stats[3 * c + 2];
    }
    return res;
  }

  StatisticalOutlierResult removeStatisticalOutliers(const Matrix3X& cloud, int nb_neighbors, double std_ratio) {
    return removeStatisticalOutliersBatch({cloud}, {nb_neighbors}, {std_ratio})[0];
  }

  std::vector<RadiusOutlierResult> removeRadiusOutliersBatch(const std::vector<Matrix3X>& clouds,
                                                             const std::vector<int>& nb_points,
                                                             const std::vector<double>& radius) {
    const size_t b = clouds.size();
    if (nb_points.size() != b || radius.size() != b)
      throw std::invalid_argument("teaser::OutlierRemoval: one entry per cloud in every argument");
    Inputs in(clouds, nb_points);
    std::vector<RadiusOutlierResult> res(b);
    std::vector<std::vector<uint8_t>> keep(b);
    std::vector<uint8_t*> pk(b);
    std::vector<int32_t*> pc(b);
    std::vector<int32_t> kept(b);
    for (size_t c = 0; c < b; ++c) {
      keep[c].resize((size_t)in.n[c] + 1);
      res[c].counts.resize((size_t)in.n[c]);
      pk[c] = keep[c].data();
      pc[c] = in.n[c] ? res[c].counts.data() : nullptr;
    }
    check(teaser_hip_icp_remove_radius_outliers_batch(h_, (int32_t)b, in.p.data(), in.n.data(), in.k.data(),
                                                      radius.data(), pk.data(), kept.data(), pc.data()));
    for (size_t c = 0; c < b; ++c) res[c].indices = compact(keep[c], in.n[c], kept[c]);
    return res;
  }

  RadiusOutlierResult removeRadiusOutliers(const Matrix3X& cloud, int nb_points, double radius) {
    return removeRadiusOutliersBatch({cloud}, {nb_points}, {radius})[0];
  }

  std::vector<SelfKnnResult> selfKnnBatch(const std::vector<Matrix3X>& clouds, const std::vector<int>& k) {
    const size_t b = clouds.size();
    if (k.size() != b) throw std::invalid_argument("teaser::OutlierRemoval: one k per cloud");
    Inputs in(clouds, k);
    std::vector<SelfKnnResult> res(b);
    std::vector<int32_t*> pi(b);
    std::vector<double*> pd(b);
    for (size_t c = 0; c < b; ++c) {
      const size_t slots = (size_t)in.n[c] * (size_t)(k[c] > 0 ? k[c] : 0);
      res[c].k = k[c];
      res[c].indices.resize(slots + 1);  // + 1: a non-NULL pointer for the library's check whatever k is
      res[c].distances2.resize(slots + 1);
      pi[c] = res[c].indices.data();
      pd[c] = res[c].distances2.data();
    }
    check(teaser_hip_icp_self_knn_batch(h_, (int32_t)b, in.p.data(), in.n.data(), in.k.data(), pi.data(), pd.data()));
    for (size_t c = 0; c < b; ++c) {
      res[c].indices.pop_back();
      res[c].distances2.pop_back();
    }
    return res;
  }

  SelfKnnResult selfKnn(const Matrix3X& cloud, int k) { return selfKnnBatch({cloud}, {k})[0]; }

  // teaser_hip_icp_set_option / _get_option: "knn_ring_cap", "knn_fallbacks" (include/teaser_hip.h)
  void setOption(const std::string& name, int64_t value) { check(teaser_hip_icp_set_option(h_, name.c_str(), value)); }
  int64_t getOption(const std::string& name) const {
    int64_t v = 0;
    check(teaser_hip_icp_get_option(h_, name.c_str(), &v));
    return v;
  }

 private:
  struct Inputs {  // the C arrays of a batch of clouds and one integer per cloud
    std::vector<const double*> p;
    std::vector<int32_t> n, k;
    Inputs(const std::vector<Matrix3X>& clouds, const std::vector<int>& per_cloud)
        : p(clouds.size()), n(clouds.size()), k(clouds.size()) {
      for (size_t c = 0; c < clouds.size(); ++c) {
        p[c] = clouds[c].data();
        n[c] = (int32_t)clouds[c].cols();
        k[c] = per_cloud[c];
      }
    }
  };

  void check(int32_t rc) const {
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::OutlierRemoval: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
  }

  static std::vector<int> compact(const std::vector<uint8_t>& keep, int32_t n, int32_t kept) {
    std::vector<int> ind;
    ind.reserve((size_t)(kept > 0 ? kept : 0));
    for (int32_t i = 0; i < n; ++i)
      if (keep[(size_t)i]) ind.push_back(i);
    return ind;
  }

  teaser_hip_icp* h_ = nullptr;
};

// Open3D's free-function forms; each creates a handle per call -- keep a teaser::OutlierRemoval for repeated calls.
inline StatisticalOutlierResult removeStatisticalOutliers(const Matrix3X& cloud, int nb_neighbors, double std_ratio) {
  OutlierRemoval o;
  return o.removeStatisticalOutliers(cloud, nb_neighbors, std_ratio);
}
inline std::vector<StatisticalOutlierResult> removeStatisticalOutliers(const std::vector<Matrix3X>& clouds,
                                                                       const std::vector<int>& nb_neighbors,
                                                                       const std::vector<double>& std_ratio) {
  OutlierRemoval o;
  return o.removeStatisticalOutliersBatch(clouds, nb_neighbors, std_ratio);
}
inline RadiusOutlierResult removeRadiusOutliers(const Matrix3X& cloud, int nb_points, double radius) {
  OutlierRemoval o;
  return o.removeRadiusOutliers(cloud, nb_points, radius);
}
inline std::vector<RadiusOutlierResult> removeRadiusOutliers(const std::vector<Matrix3X>& clouds,
                                                             const std::vector<int>& nb_points,
                                                             const std::vector<double>& radius) {
  OutlierRemoval o;
  return o.removeRadiusOutliersBatch(clouds, nb_points, radius);
}
inline SelfKnnResult selfKnn(const Matrix3X& cloud, int k) {
  OutlierRemoval o;
  return o.selfKnn(cloud, k);
}
inline std::vector<SelfKnnResult> selfKnn(const std::vector<Matrix3X>& clouds, const std::vector<int>& k) {
  OutlierRemoval o;
  return o.selfKnnBatch(clouds, k);
}

}  // namespace teaser
