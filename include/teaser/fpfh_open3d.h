// teaser/fpfh_open3d.h -- FPFH in Open3D's form on the MI355X: Open3D's compute_fpfh_feature on GIVEN normals with
// KDTreeSearchParamHybrid or KDTreeSearchParamKNN, FP64, over the C ABI (include/teaser_hip.h, "FPFH (Open3D form)",
// where the contract is written out).  Header-only.  This is not the descriptor of teaser/fpfh.h, which is PCL's.
//
// Clouds and normals are teaser::Matrix3X as in teaser/icp.h (one point per column), the search a teaser::NormalSearch
// (NormalSearch::Hybrid(radius, max_nn) or NormalSearch::KNN(k), not oriented, max_nn in [2, 100]).  A
// teaser::FPFHOpen3D holds one ICP handle and is reusable but not re-entrant.  A failed call throws teaser::ICPError, the
// constructor too when no MI355X is visible (there is no CPU path).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "teaser/icp.h"

namespace teaser {

// One cloud's descriptors: point i's 33 doubles are data[33 i .. 33 i + 32] -- the memory of Open3D's column-major
// 33 x n Feature.data.
struct FPFHOpen3DFeature {
  static constexpr int kDim = 33;
  int64_t n = 0;
  std::vector<double> data;  // n x 33 FPFH rows
  std::vector<double> spfh;  // n x 33 SPFH rows, when asked for
  Matrix3X normals;          // the normals the cloud was computed with, when asked for
  const double* row(int64_t i) const { return data.data() + kDim * i; }
};

class FPFHOpen3D {
 public:
  explicit FPFHOpen3D(int device = -1) {
    const int32_t rc = teaser_hip_icp_create(device, &h_);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::FPFHOpen3D: teaser_hip_icp_create failed (status " + std::to_string(rc) +
                             (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)" : ")"));
  }
  ~FPFHOpen3D() { teaser_hip_icp_destroy(h_); }
  FPFHOpen3D(const FPFHOpen3D&) = delete;
  FPFHOpen3D& operator=(const FPFHOpen3D&) = delete;

  // Many clouds in one launch sequence; result c is identical to cloud c computed alone.  normals: one matrix per
  // cloud; a cloud whose matrix has no columns although the cloud has points gets its normals estimated on the device
  // first, by normal_search[c] (any orientation) -- the bits of ICP::estimateNormalsBatch followed by this call.
  std::vector<FPFHOpen3DFeature> computeBatch(const std::vector<Matrix3X>& clouds, const std::vector<Matrix3X>& normals,
                                              const std::vector<NormalSearch>& search,
                                              const std::vector<NormalSearch>& normal_search = {},
                                              bool return_spfh = false, bool return_normals = false) {
    const size_t b = clouds.size();
    if (normals.size() != b || search.size() != b || (!normal_search.empty() && normal_search.size() != b))
      throw std::invalid_argument("teaser::FPFHOpen3D: one entry per cloud in every argument");
    std::vector<const double*> pp(b), pn(b);
    std::vector<int32_t> n(b);
    std::vector<teaser_icp_normal_search_c> rec(b), nrec(b);
    std::vector<FPFHOpen3DFeature> out(b);
    std::vector<double*> pf(b), ps(b), po(b);
    for (size_t c = 0; c < b; ++c) {
      const int64_t cols = clouds[c].cols();
      if (normals[c].cols() != 0 && normals[c].cols() != cols)
        throw std::invalid_argument("teaser::FPFHOpen3D: as many normals as points");
      pp[c] = clouds[c].data();
      pn[c] = normals[c].cols() != 0 ? normals[c].data() : nullptr;
      n[c] = (int32_t)cols;
      rec[c] = search[c].rec;
      nrec[c] = normal_search.empty() ? NormalSearch().rec : normal_search[c].rec;
      out[c].n = cols;
      out[c].data.resize((size_t)(FPFHOpen3DFeature::kDim * cols));
      if (return_spfh) out[c].spfh.resize(out[c].data.size());
      if (return_normals) out[c].normals = Matrix3X(3, cols);
      pf[c] = out[c].data.data();
      ps[c] = out[c].spfh.data();
      po[c] = return_normals ? out[c].normals.data() : nullptr;
    }
    const int32_t rc = teaser_hip_icp_fpfh_batch(h_, (int32_t)b, pp.data(), pn.data(), n.data(), rec.data(), nrec.data(),
                                                 pf.data(), return_spfh ? ps.data() : nullptr,
                                                 return_normals ? po.data() : nullptr);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::FPFHOpen3D: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
    return out;
  }

  FPFHOpen3DFeature compute(const Matrix3X& cloud, const Matrix3X& normals, const NormalSearch& search) {
    return std::move(computeBatch({cloud}, {normals}, {search})[0]);
  }

  // The extract_fpfh helper of Open3D's global-registration scripts in one call: normals by Hybrid(2 v, 30), features by
  // Hybrid(5 v, 100).
  FPFHOpen3DFeature extractFPFH(const Matrix3X& cloud, double voxel_size, bool return_normals = false) {
    return std::move(computeBatch({cloud}, {Matrix3X(3, 0)}, {NormalSearch::Hybrid(5 * voxel_size, 100)},
                                  {NormalSearch::Hybrid(2 * voxel_size, 30)}, false, return_normals)[0]);
  }

  // teaser_hip_icp_set_option / _get_option: "fpfh_list_bytes", "knn_ring_cap" (include/teaser_hip.h); no value changes
  // a result
  void setOption(const std::string& name, int64_t value) {
    if (teaser_hip_icp_set_option(h_, name.c_str(), value) != TEASER_HIP_OK)
      throw ICPError(TEASER_HIP_ERR_BAD_ARG, std::string("teaser::FPFHOpen3D: ") + teaser_hip_icp_last_error(h_));
  }
  int64_t getOption(const std::string& name) const {
    int64_t v = 0;
    if (teaser_hip_icp_get_option(h_, name.c_str(), &v) != TEASER_HIP_OK)
      throw ICPError(TEASER_HIP_ERR_BAD_ARG, std::string("teaser::FPFHOpen3D: ") + teaser_hip_icp_last_error(h_));
    return v;
  }

 private:
  teaser_hip_icp* h_ = nullptr;
};

// Open3D's compute_fpfh_feature(cloud with normals, search).
inline FPFHOpen3DFeature computeFPFHFeature(const Matrix3X& points, const Matrix3X& normals, const NormalSearch& search) {
  FPFHOpen3D f;
  return f.compute(points, normals, search);
}

inline std::vector<FPFHOpen3DFeature> computeFPFHFeatureBatch(const std::vector<Matrix3X>& points,
                                                              const std::vector<Matrix3X>& normals,
                                                              const std::vector<NormalSearch>& search) {
  FPFHOpen3D f;
  return f.computeBatch(points, normals, search);
}

}  // namespace teaser
