// teaser/voxel.h -- voxel down-sampling (Open3D's PointCloud::VoxelDownSample, the first step of the 3DMatch
// tutorial) over the MI355X C ABI (include/teaser_hip.h, "Voxel down-sampling", where the contract is written out).
// Header-only.
//
// Types follow teaser/registration.h: with Eigen a cloud is Eigen::Matrix<double, 3, Dynamic>, without it the
// header's teaser::Matrix3X (same column-major layout).  Output voxels come in ascending (i_x, i_y, i_z) order.  The
// VoxelGrid object holds one device handle and is reusable but not re-entrant (one call at a time per object); its
// constructor throws teaser::VoxelError with TEASER_HIP_ERR_NO_DEVICE when no MI355X is visible (there is no CPU
// path), the calls throw teaser::VoxelError on a failed call (TEASER_HIP_ERR_BAD_ARG: the message names the
// argument).
#pragma once

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "teaser/registration.h"
#include "teaser_hip.h"

namespace teaser {

struct VoxelDownSampleResult {
  Matrix3X points;                      // 3 x n_out voxel means
  std::vector<int32_t> counts;          // points per output voxel
  std::vector<int32_t> voxel_of_point;  // output voxel of every input point (empty unless asked for)
};

// What teaser::VoxelGrid throws when a library call fails; status() is the teaser_hip_status.
class VoxelError : public std::runtime_error {
 public:
  VoxelError(int32_t status, const std::string& what) : std::runtime_error(what), status_(status) {}
  int32_t status() const { return status_; }

 private:
  int32_t status_;
};

class VoxelGrid {
 public:
  explicit VoxelGrid(int device = -1) {
    const int32_t rc = teaser_hip_voxel_create(device, &h_);
    if (rc != TEASER_HIP_OK)
      throw VoxelError(rc, "teaser::VoxelGrid: teaser_hip_voxel_create failed (status " + std::to_string(rc) +
                               (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)" : ")"));
  }
  ~VoxelGrid() { teaser_hip_voxel_destroy(h_); }
  VoxelGrid(const VoxelGrid&) = delete;
  VoxelGrid& operator=(const VoxelGrid&) = delete;

  // Many clouds in one launch sequence; result b is identical to cloud b down-sampled alone.
  std::vector<VoxelDownSampleResult> voxelDownSampleBatch(const std::vector<Matrix3X>& clouds,
                                                          const std::vector<double>& voxel_size,
                                                          bool with_voxel_of_point = false) {
    const size_t b = clouds.size();
    if (voxel_size.size() != b) throw std::invalid_argument("teaser::VoxelGrid: one voxel size per cloud");
    std::vector<const double*> pts(b);
    std::vector<int32_t> n(b);
    std::vector<std::vector<double>> out(b);
    std::vector<double*> po(b);
    std::vector<int64_t> n_out(b, 0);
    std::vector<VoxelDownSampleResult> res(b);
    std::vector<int32_t*> pc(b), pv(b);
    for (size_t k = 0; k < b; ++k) {
      pts[k] = clouds[k].data();
      n[k] = (int32_t)clouds[k].cols();
      out[k].resize(3 * (size_t)(n[k] > 0 ? n[k] : 1));
      po[k] = out[k].data();
      res[k].counts.resize((size_t)(n[k] > 0 ? n[k] : 1));
      pc[k] = res[k].counts.data();
      if (with_voxel_of_point) {
        res[k].voxel_of_point.resize((size_t)(n[k] > 0 ? n[k] : 1));
        pv[k] = res[k].voxel_of_point.data();
      }
    }
    const int32_t rc = teaser_hip_voxel_down_sample_batch(h_, (int32_t)b, pts.data(), n.data(), voxel_size.data(),
                                                          po.data(), n_out.data(), pc.data(),
                                                          with_voxel_of_point ? pv.data() : nullptr);
    if (rc != TEASER_HIP_OK)
      throw VoxelError(rc, "teaser::VoxelGrid: status " + std::to_string(rc) + ": " + teaser_hip_voxel_last_error(h_));
    for (size_t k = 0; k < b; ++k) {
      res[k].points = Matrix3X(3, n_out[k]);
      if (n_out[k] > 0) std::memcpy(res[k].points.data(), out[k].data(), 24 * (size_t)n_out[k]);
      res[k].counts.resize((size_t)n_out[k]);
      if (with_voxel_of_point) res[k].voxel_of_point.resize((size_t)n[k]);
    }
    return res;
  }

  VoxelDownSampleResult voxelDownSample(const Matrix3X& cloud, double voxel_size, bool with_voxel_of_point = false) {
    return voxelDownSampleBatch({cloud}, {voxel_size}, with_voxel_of_point)[0];
  }

 private:
  teaser_hip_voxel* h_ = nullptr;
};

// Open3D's pcd.voxel_down_sample(voxel_size), one cloud; creates a handle per call -- keep a teaser::VoxelGrid
// object for repeated calls.
inline Matrix3X voxelDownSample(const Matrix3X& cloud, double voxel_size) {
  VoxelGrid grid;
  return grid.voxelDownSample(cloud, voxel_size).points;
}

}  // namespace teaser
