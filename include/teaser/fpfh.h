// teaser/fpfh.h -- drop-in for the reference's teaser/include/teaser/fpfh.h (teaser::FPFHEstimation,
// reference fpfh.h:22-90, teaser/src/fpfh.cc:15-43) over the MI355X C ABI (teaser_hip_compute_fpfh).
//
// The reference class is a pass-through to PCL (pcl::NormalEstimationOMP + pcl::FPFHEstimationOMP) and its
// types are PCL's (pcl::PointCloud<pcl::FPFHSignature33>::Ptr).  PCL is not a dependency here: the same
// names are small value types with the members the reference's callers touch (`histogram[33]`, size(),
// iteration, operator[], `->` on the returned pointer), the arithmetic runs on the GPU with PCL's
// semantics (csrc/kernels_features.hip), pinned to the reference's bunny fixture.
#pragma once

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "teaser/geometry.h"
#include "teaser/handle.h"
#include "teaser_hip.h"

namespace teaser {

struct FPFHSignature33 {  // pcl::FPFHSignature33
  float histogram[33];
  static int descriptorSize() { return 33; }
};
struct Normal {  // pcl::Normal (the fields the callers read)
  float normal_x, normal_y, normal_z;
};
using FPFHCloud = std::vector<FPFHSignature33>;      // pcl::PointCloud<pcl::FPFHSignature33>
using FPFHCloudPtr = std::shared_ptr<FPFHCloud>;     // ...::Ptr
using NormalCloud = std::vector<Normal>;             // pcl::PointCloud<pcl::Normal>

class FPFHEstimation {
 public:
  FPFHEstimation() = default;
  FPFHEstimation(const FPFHEstimation&) = delete;
  FPFHEstimation& operator=(const FPFHEstimation&) = delete;

  // fpfh.h:40-42, fpfh.cc:15-43: normals with a radius search (viewpoint at the origin), then FPFH.
  // Throws std::runtime_error when no MI355X is visible (no CPU path) or the call fails.
  FPFHCloudPtr computeFPFHFeatures(const PointCloud& input_cloud, double normal_search_radius = 0.03,
                                   double fpfh_search_radius = 0.05) {
    static_assert(sizeof(PointXYZ) == 12 && sizeof(FPFHSignature33) == 132 && sizeof(Normal) == 12, "packed");
    h_.create("teaser::FPFHEstimation");
    const int32_t n = (int32_t)input_cloud.size();
    FPFHCloudPtr out = std::make_shared<FPFHCloud>((size_t)n);
    normals_.assign((size_t)n, Normal());
    const int32_t rc = teaser_hip_compute_fpfh(h_, reinterpret_cast<const float*>(input_cloud.data()), n,
                                               normal_search_radius, fpfh_search_radius,
                                               reinterpret_cast<float*>(out->data()),
                                               reinterpret_cast<float*>(normals_.data()));
    if (rc != TEASER_HIP_OK)
      throw std::runtime_error(std::string("teaser_hip_compute_fpfh status ") + std::to_string(rc) + ": " +
                               teaser_hip_last_error(h_));
    return out;
  }
  // fpfh.h:56: the normals used by the last computeFPFHFeatures
  NormalCloud getNormals() { return normals_; }

  // computeFPFHFeatures for many clouds in one launch sequence (teaser_hip_features_fpfh_batch; no counterpart in
  // the reference): one FPFHCloud per input cloud, each bit-identical to the single-cloud call.  Clouds of mixed
  // sizes and empty clouds are allowed.
  std::vector<FPFHCloud> computeFPFHFeaturesBatch(const std::vector<PointCloud>& input_clouds,
                                                  double normal_search_radius = 0.03,
                                                  double fpfh_search_radius = 0.05) {
    fh_.create("teaser::FPFHEstimation");
    const size_t batch = input_clouds.size();
    std::vector<FPFHCloud> out(batch);
    batch_normals_.assign(batch, NormalCloud());
    std::vector<const float*> pts(batch);
    std::vector<float*> feat(batch), nrm(batch);
    std::vector<int32_t> n(batch);
    const std::vector<double> rn(batch, normal_search_radius), rf(batch, fpfh_search_radius);
    for (size_t b = 0; b < batch; ++b) {
      n[b] = (int32_t)input_clouds[b].size();
      out[b].resize((size_t)n[b]);
      batch_normals_[b].assign((size_t)n[b], Normal());
      pts[b] = reinterpret_cast<const float*>(input_clouds[b].data());
      feat[b] = reinterpret_cast<float*>(out[b].data());
      nrm[b] = reinterpret_cast<float*>(batch_normals_[b].data());
    }
    const int32_t rc = teaser_hip_features_fpfh_batch(fh_, (int32_t)batch, pts.data(), n.data(), rn.data(), rf.data(),
                                                      feat.data(), nrm.data());
    if (rc != TEASER_HIP_OK)
      throw std::runtime_error(std::string("teaser_hip_features_fpfh_batch status ") + std::to_string(rc) + ": " +
                               teaser_hip_features_last_error(fh_));
    return out;
  }
  // the normals used by the last computeFPFHFeaturesBatch, per cloud
  const std::vector<NormalCloud>& getNormalsBatch() const { return batch_normals_; }

 private:
  detail::LazyFeatures fh_;  // (declared first: destroyed after the solver)
  detail::LazySolver h_;
  NormalCloud normals_;
  std::vector<NormalCloud> batch_normals_;
};

}  // namespace teaser
