// teaser/search.h -- nearest-neighbour search between two clouds on the MI355X: Open3D's KDTreeFlann /
// core.nns.NearestNeighborSearch (k-NN, uncapped radius and hybrid search of a query set in a data cloud) and the two
// point-cloud distances built on it, over the C ABI (include/teaser_hip.h, "Neighbour search", where the contract is
// written out).  Header-only.
//
// Clouds are teaser::Matrix3X as in teaser/icp.h.  A teaser::NearestNeighborSearch is constructed on a data cloud (or,
// for the batch forms, on several), holds one ICP handle and is reusable but not re-entrant.  Distances are squared,
// neighbours come in ascending (squared distance, index).  A failed call throws teaser::ICPError, the constructor too
// when no MI355X is visible (there is no CPU path).
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "teaser/icp.h"

namespace teaser {

struct KnnSearchResult {
  int k = 0;                       // slots per query: k of knnSearch, max_nn of hybridSearch
  std::vector<int32_t> indices;    // n_query x k row-major; unused slots -1
  std::vector<double> distances2;  // n_query x k squared distances; unused slots +inf
  std::vector<int32_t> counts;     // hybridSearch: the number of neighbours written per query
};

struct RadiusSearchResult {
  std::vector<int32_t> indices;     // the rows one after the other
  std::vector<double> distances2;   // likewise
  std::vector<int64_t> row_splits;  // n_query + 1: the neighbours of query i are [row_splits[i], row_splits[i + 1])
};

class NearestNeighborSearch {
 public:
  explicit NearestNeighborSearch(const Matrix3X& data, int device = -1) : NearestNeighborSearch(std::vector<Matrix3X>{data}, device) {}
  explicit NearestNeighborSearch(const std::vector<Matrix3X>& data, int device = -1) : data_(data) {
    const int32_t rc = teaser_hip_icp_create(device, &h_);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::NearestNeighborSearch: teaser_hip_icp_create failed (status " + std::to_string(rc) +
                             (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)" : ")"));
  }
  ~NearestNeighborSearch() { teaser_hip_icp_destroy(h_); }
  NearestNeighborSearch(const NearestNeighborSearch&) = delete;
  NearestNeighborSearch& operator=(const NearestNeighborSearch&) = delete;

  // One query set per data cloud of the constructor, one parameter per problem.
  std::vector<KnnSearchResult> knnSearchBatch(const std::vector<Matrix3X>& queries, const std::vector<int>& k) {
    Inputs in(data_, queries, k);
    std::vector<KnnSearchResult> res = rows(in);
    check(teaser_hip_icp_knn_search_batch(h_, in.b, in.pd.data(), in.nd.data(), in.pq.data(), in.nq.data(), in.k.data(),
                                          in.pi.data(), in.pf.data()));
    return trim(res, false);
  }
  std::vector<KnnSearchResult> hybridSearchBatch(const std::vector<Matrix3X>& queries, const std::vector<double>& radius,
                                                 const std::vector<int>& max_nn) {
    Inputs in(data_, queries, max_nn);
    if (radius.size() != data_.size()) throw std::invalid_argument("teaser::NearestNeighborSearch: one radius per problem");
    std::vector<KnnSearchResult> res = rows(in);
    check(teaser_hip_icp_hybrid_search_batch(h_, in.b, in.pd.data(), in.nd.data(), in.pq.data(), in.nq.data(),
                                             radius.data(), in.k.data(), in.pi.data(), in.pf.data(), in.pc.data()));
    return trim(res, true);
  }
  // Counts, then fills arrays of the exact size: two calls of the library.
  std::vector<RadiusSearchResult> radiusSearchBatch(const std::vector<Matrix3X>& queries,
                                                    const std::vector<double>& radius) {
    Inputs in(data_, queries, std::vector<int>(data_.size(), 1));
    if (radius.size() != data_.size()) throw std::invalid_argument("teaser::NearestNeighborSearch: one radius per problem");
    const size_t b = data_.size();
    std::vector<std::vector<int32_t>> counts(b);
    std::vector<int64_t> total(b, 0);
    for (size_t c = 0; c < b; ++c) {
      counts[c].resize((size_t)in.nq[c] + 1);
      in.pc[c] = counts[c].data();
    }
    check(teaser_hip_icp_radius_search_batch(h_, in.b, in.pd.data(), in.nd.data(), in.pq.data(), in.nq.data(),
                                             radius.data(), nullptr, in.pc.data(), nullptr, nullptr, total.data()));
    std::vector<RadiusSearchResult> res(b);
    for (size_t c = 0; c < b; ++c) {
      res[c].indices.resize((size_t)total[c] + 1);
      res[c].distances2.resize((size_t)total[c] + 1);
      in.pi[c] = res[c].indices.data();
      in.pf[c] = res[c].distances2.data();
    }
    const std::vector<int64_t> capacity = total;
    check(teaser_hip_icp_radius_search_batch(h_, in.b, in.pd.data(), in.nd.data(), in.pq.data(), in.nq.data(),
                                             radius.data(), capacity.data(), in.pc.data(), in.pi.data(), in.pf.data(),
                                             total.data()));
    for (size_t c = 0; c < b; ++c) {
      if (total[c] != capacity[c]) throw std::logic_error("teaser::NearestNeighborSearch: the count changed between the calls");
      res[c].indices.pop_back();
      res[c].distances2.pop_back();
      res[c].row_splits.assign((size_t)in.nq[c] + 1, 0);
      for (int32_t i = 0; i < in.nq[c]; ++i) res[c].row_splits[(size_t)i + 1] = res[c].row_splits[(size_t)i] + counts[c][(size_t)i];
    }
    return res;
  }

  // The single-problem forms (an object constructed on one data cloud).
  KnnSearchResult knnSearch(const Matrix3X& queries, int k) { return knnSearchBatch({queries}, {k})[0]; }
  KnnSearchResult hybridSearch(const Matrix3X& queries, double radius, int max_nn) {
    return hybridSearchBatch({queries}, {radius}, {max_nn})[0];
  }
  RadiusSearchResult radiusSearch(const Matrix3X& queries, double radius) {
    return radiusSearchBatch({queries}, {radius})[0];
  }

  // teaser_hip_icp_set_option / _get_option: "knn_ring_cap", "knn_fallbacks" (include/teaser_hip.h)
  void setOption(const std::string& name, int64_t value) { check(teaser_hip_icp_set_option(h_, name.c_str(), value)); }
  int64_t getOption(const std::string& name) const {
    int64_t v = 0;
    check(teaser_hip_icp_get_option(h_, name.c_str(), &v));
    return v;
  }

 private:
  struct Inputs {  // the C arrays of a batch of problems and one integer per problem
    int32_t b;
    std::vector<const double*> pd, pq;
    std::vector<int32_t> nd, nq, k;
    std::vector<int32_t*> pi, pc;
    std::vector<double*> pf;
    Inputs(const std::vector<Matrix3X>& data, const std::vector<Matrix3X>& queries, const std::vector<int>& per_problem)
        : b((int32_t)data.size()), pd(data.size()), pq(data.size()), nd(data.size()), nq(data.size()), k(data.size()),
          pi(data.size()), pc(data.size()), pf(data.size()) {
      if (queries.size() != data.size() || per_problem.size() != data.size())
        throw std::invalid_argument("teaser::NearestNeighborSearch: one query set and one parameter per data cloud");
      for (size_t c = 0; c < data.size(); ++c) {
        pd[c] = data[c].data();
        nd[c] = (int32_t)data[c].cols();
        pq[c] = queries[c].data();
        nq[c] = (int32_t)queries[c].cols();
        k[c] = per_problem[c];
      }
    }
  };

  // n_query x k outputs (+ 1: a non-NULL pointer for the library's check whatever k is)
  static std::vector<KnnSearchResult> rows(Inputs& in) {
    std::vector<KnnSearchResult> res((size_t)in.b);
    for (size_t c = 0; c < res.size(); ++c) {
      const size_t slots = (size_t)in.nq[c] * (size_t)(in.k[c] > 0 ? in.k[c] : 0);
      res[c].k = in.k[c];
      res[c].indices.resize(slots + 1);
      res[c].distances2.resize(slots + 1);
      res[c].counts.resize((size_t)in.nq[c] + 1);
      in.pi[c] = res[c].indices.data();
      in.pf[c] = res[c].distances2.data();
      in.pc[c] = res[c].counts.data();
    }
    return res;
  }
  static std::vector<KnnSearchResult> trim(std::vector<KnnSearchResult>& res, bool counts) {
    for (KnnSearchResult& r : res) {
      r.indices.pop_back();
      r.distances2.pop_back();
      r.counts.pop_back();
      if (!counts) r.counts.clear();
    }
    return std::move(res);
  }

  void check(int32_t rc) const {
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::NearestNeighborSearch: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
  }

  std::vector<Matrix3X> data_;
  teaser_hip_icp* h_ = nullptr;
};

// Open3D's source.compute_point_cloud_distance(target): per source point the distance to the nearest target point
// (the square root of the k = 1 squared distance; +inf when target is empty).
inline std::vector<double> computePointCloudDistance(const Matrix3X& source, const Matrix3X& target) {
  NearestNeighborSearch nns(target);
  const KnnSearchResult r = nns.knnSearch(source, 1);
  std::vector<double> d(r.distances2.size());
  for (size_t i = 0; i < d.size(); ++i) d[i] = std::sqrt(r.distances2[i]);
  return d;
}

// Open3D's cloud.compute_nearest_neighbor_distance(): per point the distance to its nearest other point (the square
// root of slot 1 of self k-NN with k = 2); zeros for fewer than two points.
inline std::vector<double> computeNearestNeighborDistance(const Matrix3X& cloud) {
  const size_t n = (size_t)cloud.cols();
  std::vector<double> d(n, 0.0);
  if (n < 2) return d;
  teaser_hip_icp* h = nullptr;
  int32_t rc = teaser_hip_icp_create(-1, &h);
  if (rc != TEASER_HIP_OK) throw ICPError(rc, "teaser::computeNearestNeighborDistance: teaser_hip_icp_create failed");
  std::vector<int32_t> idx(2 * n);
  std::vector<double> d2(2 * n);
  const double* p = cloud.data();
  const int32_t nn = (int32_t)n, k = 2;
  int32_t* pi = idx.data();
  double* pd = d2.data();
  rc = teaser_hip_icp_self_knn_batch(h, 1, &p, &nn, &k, &pi, &pd);
  const std::string err = rc != TEASER_HIP_OK ? teaser_hip_icp_last_error(h) : "";
  teaser_hip_icp_destroy(h);
  if (rc != TEASER_HIP_OK) throw ICPError(rc, "teaser::computeNearestNeighborDistance: " + err);
  for (size_t i = 0; i < n; ++i) d[i] = std::sqrt(d2[2 * i + 1]);
  return d;
}

}  // namespace teaser
