// teaser/cluster.h -- DBSCAN clustering on the MI355X (Open3D's PointCloud::ClusterDBSCAN) over the C ABI
// (include/teaser_hip.h, "DBSCAN clustering", where the contract is written out).  Header-only.
//
// Clouds are teaser::Matrix3X as in teaser/icp.h.  A teaser::DBSCAN object holds one ICP handle and is reusable but not
// re-entrant; the batched form takes many clouds in one launch sequence, each cloud's result identical to the same cloud
// run alone.  Labels are Open3D's: -1 for noise, clusters numbered from 0 in the order its loop opens them.  A failed
// call throws teaser::ICPError, the constructor too when no MI355X is visible (there is no CPU path).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "teaser/icp.h"

namespace teaser {

struct DBSCANParams {
  double eps = 0.0;    // the neighbourhood radius (strict: d2 < eps * eps)
  int min_points = 1;  // neighbours, the point included, that make a core point (>= 1)
};

struct DBSCANResult {
  std::vector<int> labels;      // per point: its cluster, -1 for noise
  int n_clusters = 0;
  std::vector<int32_t> counts;  // per point: neighbours inside eps, the point included
  std::vector<int32_t> roots;   // per point: the smallest core index of its component, -1 for a point that is not core
};

class DBSCAN {
 public:
  explicit DBSCAN(int device = -1) {
    const int32_t rc = teaser_hip_icp_create(device, &h_);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::DBSCAN: teaser_hip_icp_create failed (status " + std::to_string(rc) +
                             (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)" : ")"));
  }
  ~DBSCAN() { teaser_hip_icp_destroy(h_); }
  DBSCAN(const DBSCAN&) = delete;
  DBSCAN& operator=(const DBSCAN&) = delete;

  std::vector<DBSCANResult> clusterBatch(const std::vector<Matrix3X>& clouds, const std::vector<DBSCANParams>& params) {
    const size_t b = clouds.size();
    if (params.size() != b) throw std::invalid_argument("teaser::DBSCAN: one DBSCANParams per cloud");
    static_assert(sizeof(int) == sizeof(int32_t), "labels are written in place");
    std::vector<const double*> p(b);
    std::vector<int32_t> n(b), ncl(b);
    std::vector<teaser_icp_dbscan_params_c> rec(b);
    std::vector<DBSCANResult> res(b);
    std::vector<int32_t*> pl(b), pc(b), pr(b);
    for (size_t c = 0; c < b; ++c) {
      p[c] = clouds[c].data();
      n[c] = (int32_t)clouds[c].cols();
      rec[c].eps = params[c].eps;
      rec[c].min_points = params[c].min_points;
      rec[c].reserved = 0;
      res[c].labels.resize((size_t)n[c]);
      res[c].counts.resize((size_t)n[c]);
      res[c].roots.resize((size_t)n[c]);
      pl[c] = n[c] ? reinterpret_cast<int32_t*>(res[c].labels.data()) : nullptr;
      pc[c] = n[c] ? res[c].counts.data() : nullptr;
      pr[c] = n[c] ? res[c].roots.data() : nullptr;
    }
    const int32_t rc = teaser_hip_icp_cluster_dbscan_batch(h_, (int32_t)b, p.data(), n.data(), rec.data(), pl.data(),
                                                           ncl.data(), pc.data(), pr.data());
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::DBSCAN: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
    for (size_t c = 0; c < b; ++c) res[c].n_clusters = ncl[c];
    return res;
  }

  DBSCANResult cluster(const Matrix3X& cloud, const DBSCANParams& params) { return clusterBatch({cloud}, {params})[0]; }

 private:
  teaser_hip_icp* h_ = nullptr;
};

// Open3D's form: the labels.  Each call creates a handle -- keep a teaser::DBSCAN for repeated calls, or for the
// counts, the roots and the number of clusters.
inline std::vector<int> clusterDBSCAN(const Matrix3X& cloud, double eps, int min_points) {
  DBSCAN d;
  DBSCANParams p;
  p.eps = eps, p.min_points = min_points;
  return d.cluster(cloud, p).labels;
}
inline std::vector<std::vector<int>> clusterDBSCANBatch(const std::vector<Matrix3X>& clouds,
                                                        const std::vector<DBSCANParams>& params) {
  DBSCAN d;
  std::vector<std::vector<int>> out;
  for (DBSCANResult& r : d.clusterBatch(clouds, params)) out.push_back(std::move(r.labels));
  return out;
}

}  // namespace teaser
