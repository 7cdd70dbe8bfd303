// teaser/icp.h -- ICP refinement (Open3D's RegistrationICP with TransformationEstimationPointToPoint(with_scaling =
// false), or with TransformationEstimationPointToPlane and an optional robust kernel on caller-given target
// normals, or with TransformationEstimationForGeneralizedICP on per-point covariances of both clouds, which
// ICP::estimateCovariances computes on the GPU) over the MI355X C ABI (include/teaser_hip.h, "ICP refinement", where
// the contracts are written out).
// Header-only.
//
// Types follow teaser/registration.h: with Eigen the clouds are Matrix<double,3,Dynamic> and the transform is
// Eigen::Matrix4d; without Eigen the same members are the header's small value types and teaser::Matrix4 below
// (column-major, operator()(r, c)).  The ICP object holds one device handle and is reusable but not re-entrant (one
// call at a time per object); its constructor throws teaser::ICPError with TEASER_HIP_ERR_NO_DEVICE when no MI355X is
// visible (there is no CPU path), registrationICP throws teaser::ICPError on a failed call.
#pragma once

#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "teaser/registration.h"
#include "teaser_hip.h"

namespace teaser {

#if TEASER_HIP_HAVE_EIGEN
using Matrix4 = Eigen::Matrix4d;
#else
struct Matrix4 {  // column-major 4 x 4, like Eigen::Matrix4d
  std::array<double, 16> v{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
  static Matrix4 Identity() { return Matrix4(); }
  double& operator()(int r, int c) { return v[(size_t)(4 * c + r)]; }
  double operator()(int r, int c) const { return v[(size_t)(4 * c + r)]; }
};
#endif

// The 6 x 6 information matrix of a registered pair (rotation block first, like Open3D's 6-vectors).
#if TEASER_HIP_HAVE_EIGEN
using Matrix6 = Eigen::Matrix<double, 6, 6>;
#else
struct Matrix6 {  // column-major 6 x 6, like Eigen::Matrix<double, 6, 6>; zero-initialised
  std::array<double, 36> v{};
  static Matrix6 Zero() { return Matrix6(); }
  double& operator()(int r, int c) { return v[(size_t)(6 * c + r)]; }
  double operator()(int r, int c) const { return v[(size_t)(6 * c + r)]; }
};
#endif

// Open3D's ICPConvergenceCriteria (the stop rule compares ABSOLUTE changes of fitness and inlier RMSE).
struct ICPConvergenceCriteria {
  double relative_fitness = 1e-6;
  double relative_rmse = 1e-6;
  int max_iteration = 30;
};

// Open3D's RobustKernel: the weight of a point-to-plane residual (table in include/teaser_hip.h).  L1Loss is not
// offered.
struct RobustKernel {
  int32_t kernel = 0;  // teaser_icp_estimation_c::kernel
  double k = 1.0;
};
inline RobustKernel L2Loss() { return RobustKernel{0, 1.0}; }
inline RobustKernel HuberLoss(double k = 1.0) { return RobustKernel{1, k}; }
inline RobustKernel CauchyLoss(double k = 1.0) { return RobustKernel{2, k}; }
inline RobustKernel GMLoss(double k = 1.0) { return RobustKernel{3, k}; }
inline RobustKernel TukeyLoss(double k = 1.0) { return RobustKernel{4, k}; }

// The neighbourhood of normal estimation (include/teaser_hip.h, "Normal estimation"): Open3D's
// KDTreeSearchParamHybrid(radius, max_nn) or KDTreeSearchParamKNN(knn), optionally with an orientation --
// .towards(point) (orient_normals_towards_camera_location) or .along(direction)
// (orient_normals_to_align_with_direction).  A default-constructed NormalSearch means "none" (max_nn = 0).
struct NormalSearch {
  teaser_icp_normal_search_c rec{};  // max_nn = 0: none
  static NormalSearch Hybrid(double radius, int max_nn = 30) {
    NormalSearch s;
    s.rec.search = 0, s.rec.max_nn = max_nn, s.rec.radius = radius;
    return s;
  }
  static NormalSearch KNN(int k = 30) {
    NormalSearch s;
    s.rec.search = 1, s.rec.max_nn = k;
    return s;
  }
  NormalSearch towards(double x, double y, double z) const { return oriented(1, x, y, z); }
  NormalSearch along(double x, double y, double z) const { return oriented(2, x, y, z); }
  bool given() const { return rec.max_nn != 0; }

 private:
  NormalSearch oriented(int32_t orient, double x, double y, double z) const {
    NormalSearch s = *this;
    s.rec.orient = orient, s.rec.ref[0] = x, s.rec.ref[1] = y, s.rec.ref[2] = z;
    return s;
  }
};

// What estimateNormals returns: one unit normal per point (column), and what was asked for of the raw sample
// covariances (9 doubles per point, row-major) and the ascending eigenvalues (3 per point).
struct Normals {
  Matrix3X normals;
  std::vector<double> covariances;
  std::vector<double> eigenvalues;
};

// Open3D's TransformationEstimationPointToPlane(kernel).  The target normals are an argument of registrationICP, or,
// with a normal_search, estimated from the target on the device (the registrationICP overloads without dst_normals).
struct TransformationEstimationPointToPlane {
  RobustKernel kernel;
  NormalSearch normal_search;
  TransformationEstimationPointToPlane() = default;
  explicit TransformationEstimationPointToPlane(const RobustKernel& k) : kernel(k) {}
  explicit TransformationEstimationPointToPlane(const NormalSearch& s) : normal_search(s) {}
  TransformationEstimationPointToPlane(const RobustKernel& k, const NormalSearch& s) : kernel(k), normal_search(s) {}
};

// Open3D's TransformationEstimationForGeneralizedICP, L2 only (include/teaser_hip.h says why).  The covariances of both
// clouds are arguments of registrationICP; epsilon is what estimateCovariances / covariancesFromNormals take.
struct TransformationEstimationForGeneralizedICP {
  double epsilon = 1e-3;
  TransformationEstimationForGeneralizedICP() = default;
  explicit TransformationEstimationForGeneralizedICP(double eps) : epsilon(eps) {}
};

// Open3D's TransformationEstimationForColoredICP(lambda_geometric, kernel) (include/teaser_hip.h, "ICP refinement:
// Colored ICP"): the kernel weights both residuals.  The colours of both clouds and the target normals are arguments
// of registrationColoredICP; gradient_radius (<= 0: twice max_correspondence_distance, Open3D's choice) and
// gradient_max_nn choose the neighbourhood the target's colour gradients are estimated from on the device.
struct TransformationEstimationForColoredICP {
  double lambda_geometric = 0.968;
  RobustKernel kernel;
  double gradient_radius = 0.0;
  int gradient_max_nn = 30;
  TransformationEstimationForColoredICP() = default;
  explicit TransformationEstimationForColoredICP(double lambda, const RobustKernel& k = L2Loss())
      : lambda_geometric(lambda), kernel(k) {}
};

// One 3 x 3 covariance per point: 9 doubles each, row-major (only the upper triangle is read).
using Covariances = std::vector<double>;

// C = I - (1 - epsilon) n n^T / (n^T n) per normal; the identity for a zero or non-finite normal.  Host arithmetic.
inline Covariances covariancesFromNormals(const Matrix3X& normals, double epsilon = 1e-3) {
  const size_t n = (size_t)normals.cols();
  Covariances out(9 * n, 0.0);
  for (size_t i = 0; i < n; ++i) {
    const double v[3] = {normals(0, (int64_t)i), normals(1, (int64_t)i), normals(2, (int64_t)i)};
    const double nn = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const bool ok = std::isfinite(nn) && nn > 0;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b)
        out[9 * i + (size_t)(3 * a + b)] = (a == b ? 1.0 : 0.0) - (ok ? ((1.0 - epsilon) * v[a]) * v[b] / nn : 0.0);
  }
  return out;
}

// Open3D's RegistrationResult + the number of iterations run.
struct ICPResult {
  Matrix4 transformation;
  double fitness = 0;
  double inlier_rmse = 0;
  std::vector<std::pair<int, int>> correspondence_set;  // (source, target), ascending source index
  int iterations = 0;
};

// What teaser::ICP throws when a library call fails; status() is the teaser_hip_status
// (TEASER_HIP_ERR_NO_DEVICE from the constructor: no MI355X visible).
class ICPError : public std::runtime_error {
 public:
  ICPError(int32_t status, const std::string& what) : std::runtime_error(what), status_(status) {}
  int32_t status() const { return status_; }

 private:
  int32_t status_;
};

class ICP {
 public:
  explicit ICP(int device = -1) {
    const int32_t rc = teaser_hip_icp_create(device, &h_);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::ICP: teaser_hip_icp_create failed (status " + std::to_string(rc) +
                             (rc == TEASER_HIP_ERR_NO_DEVICE ? ": no MI355X visible, there is no CPU path)" : ")"));
  }
  ~ICP() { teaser_hip_icp_destroy(h_); }
  ICP(const ICP&) = delete;
  ICP& operator=(const ICP&) = delete;

  // Many independent problems in one launch sequence; result b is identical to problem b run alone.
  std::vector<ICPResult> registrationICPBatch(const std::vector<Matrix3X>& src, const std::vector<Matrix3X>& dst,
                                              const std::vector<double>& max_correspondence_distance,
                                              const std::vector<Matrix4>& init,
                                              const std::vector<ICPConvergenceCriteria>& criteria) {
    return run(src, dst, max_correspondence_distance, init, criteria, nullptr, nullptr);
  }

  // The same with Generalized ICP: src_cov[b] / dst_cov[b] hold one covariance per point of src[b] / dst[b].
  std::vector<ICPResult> registrationICPBatch(const std::vector<Matrix3X>& src, const std::vector<Matrix3X>& dst,
                                              const std::vector<Covariances>& src_cov,
                                              const std::vector<Covariances>& dst_cov,
                                              const std::vector<double>& max_correspondence_distance,
                                              const std::vector<Matrix4>& init,
                                              const std::vector<TransformationEstimationForGeneralizedICP>& estimation,
                                              const std::vector<ICPConvergenceCriteria>& criteria) {
    const size_t b = src.size();
    if (dst.size() != b || src_cov.size() != b || dst_cov.size() != b || estimation.size() != b)
      throw std::invalid_argument("teaser::ICP: one entry per problem in every argument");
    std::vector<const double*> ps(b), pd(b);
    std::vector<teaser_icp_estimation_c> est(b);
    for (size_t k = 0; k < b; ++k) {
      if (src_cov[k].size() != 9 * (size_t)src[k].cols() || dst_cov[k].size() != 9 * (size_t)dst[k].cols())
        throw std::invalid_argument("teaser::ICP: one 3 x 3 covariance (9 doubles) per point");
      ps[k] = src_cov[k].data();
      pd[k] = dst_cov[k].data();
      est[k].method = 2;
      est[k].kernel = 0;
      est[k].kernel_k = 1.0;
    }
    return run(src, dst, max_correspondence_distance, init, criteria, nullptr, est.data(), ps.data(), pd.data());
  }

  // Covariances for Generalized ICP, estimated on the GPU (include/teaser_hip.h, "Covariance estimation"): per point
  // the max_nn nearest neighbours inside radius, C = I - (1 - epsilon) n n^T; the identity below 3 neighbours.
  std::vector<Covariances> estimateCovariancesBatch(const std::vector<Matrix3X>& clouds,
                                                    const std::vector<double>& radius,
                                                    const std::vector<int>& max_nn,
                                                    const std::vector<double>& epsilon) {
    const size_t b = clouds.size();
    if (radius.size() != b || max_nn.size() != b || epsilon.size() != b)
      throw std::invalid_argument("teaser::ICP: one entry per cloud in every argument");
    std::vector<const double*> pp(b);
    std::vector<int32_t> n(b), k(b);
    std::vector<Covariances> out(b);
    std::vector<double*> po(b);
    for (size_t c = 0; c < b; ++c) {
      pp[c] = clouds[c].data();
      n[c] = (int32_t)clouds[c].cols();
      k[c] = max_nn[c];
      out[c].resize(9 * (size_t)n[c]);
      po[c] = out[c].data();
    }
    const int32_t rc = teaser_hip_icp_covariances_batch(h_, (int32_t)b, pp.data(), n.data(), radius.data(), k.data(),
                                                        epsilon.data(), po.data());
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::ICP: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
    return out;
  }

  Covariances estimateCovariances(const Matrix3X& cloud, double radius, int max_nn = 20, double epsilon = 1e-3) {
    return estimateCovariancesBatch({cloud}, {radius}, {max_nn}, {epsilon})[0];
  }

  // Colored ICP: src_colors[b] / dst_colors[b] hold one colour (r, g, b) per point, dst_normals[b] one normal per
  // target point; dst_gradients: empty (every problem's colour gradients are estimated on the device), or per problem
  // an empty matrix or one gradient per target point.
  std::vector<ICPResult> registrationColoredICPBatch(
      const std::vector<Matrix3X>& src, const std::vector<Matrix3X>& dst, const std::vector<Matrix3X>& src_colors,
      const std::vector<Matrix3X>& dst_colors, const std::vector<Matrix3X>& dst_normals,
      const std::vector<double>& max_correspondence_distance, const std::vector<Matrix4>& init,
      const std::vector<TransformationEstimationForColoredICP>& estimation,
      const std::vector<ICPConvergenceCriteria>& criteria, const std::vector<Matrix3X>& dst_gradients = {}) {
    const size_t b = src.size();
    if (dst.size() != b || src_colors.size() != b || dst_colors.size() != b || dst_normals.size() != b ||
        estimation.size() != b || (!dst_gradients.empty() && dst_gradients.size() != b))
      throw std::invalid_argument("teaser::ICP: one entry per problem in every argument");
    ColorArgs col;
    col.src_colors.resize(b), col.dst_colors.resize(b), col.dst_gradients.assign(b, nullptr), col.rec.resize(b);
    std::vector<const double*> pn(b);
    std::vector<teaser_icp_estimation_c> est(b);
    for (size_t k = 0; k < b; ++k) {
      const bool given = !dst_gradients.empty() && dst_gradients[k].cols() > 0;
      if (src_colors[k].cols() != src[k].cols() || dst_colors[k].cols() != dst[k].cols() ||
          dst_normals[k].cols() != dst[k].cols() || (given && dst_gradients[k].cols() != dst[k].cols()))
        throw std::invalid_argument("teaser::ICP: one colour per point, one normal and one gradient per target point");
      pn[k] = dst_normals[k].data();
      col.src_colors[k] = src_colors[k].data();
      col.dst_colors[k] = dst_colors[k].data();
      if (given) col.dst_gradients[k] = dst_gradients[k].data();
      est[k].method = 3;
      est[k].kernel = estimation[k].kernel.kernel;
      est[k].kernel_k = estimation[k].kernel.k;
      col.rec[k].lambda_geometric = estimation[k].lambda_geometric;
      col.rec[k].gradient_radius = estimation[k].gradient_radius;
      col.rec[k].gradient_max_nn = estimation[k].gradient_max_nn;
      col.rec[k].reserved = 0;
    }
    return run(src, dst, max_correspondence_distance, init, criteria, pn.data(), est.data(), nullptr, nullptr, nullptr,
               &col);
  }

  ICPResult registrationColoredICP(const Matrix3X& src, const Matrix3X& dst, const Matrix3X& src_colors,
                                   const Matrix3X& dst_colors, const Matrix3X& dst_normals,
                                   double max_correspondence_distance, const Matrix4& init = Matrix4::Identity(),
                                   const TransformationEstimationForColoredICP& estimation =
                                       TransformationEstimationForColoredICP(),
                                   const ICPConvergenceCriteria& criteria = ICPConvergenceCriteria()) {
    return registrationColoredICPBatch({src}, {dst}, {src_colors}, {dst_colors}, {dst_normals},
                                       {max_correspondence_distance}, {init}, {estimation}, {criteria})[0];
  }

  // The colour gradients Colored ICP uses, for many clouds in one launch sequence; result c is identical to cloud c
  // estimated alone.
  std::vector<Matrix3X> estimateColorGradientsBatch(const std::vector<Matrix3X>& clouds,
                                                    const std::vector<Matrix3X>& normals,
                                                    const std::vector<Matrix3X>& colors,
                                                    const std::vector<double>& radius, const std::vector<int>& max_nn) {
    const size_t b = clouds.size();
    if (normals.size() != b || colors.size() != b || radius.size() != b || max_nn.size() != b)
      throw std::invalid_argument("teaser::ICP: one entry per cloud in every argument");
    std::vector<const double*> pp(b), pn(b), pc(b);
    std::vector<int32_t> n(b), k(b);
    std::vector<Matrix3X> out(b);
    std::vector<double*> po(b);
    for (size_t c = 0; c < b; ++c) {
      if (normals[c].cols() != clouds[c].cols() || colors[c].cols() != clouds[c].cols())
        throw std::invalid_argument("teaser::ICP: one normal and one colour per point");
      pp[c] = clouds[c].data(), pn[c] = normals[c].data(), pc[c] = colors[c].data();
      n[c] = (int32_t)clouds[c].cols();
      k[c] = max_nn[c];
      out[c] = Matrix3X(3, clouds[c].cols());
      po[c] = out[c].data();
    }
    const int32_t rc = teaser_hip_icp_color_gradients_batch(h_, (int32_t)b, pp.data(), n.data(), pn.data(), pc.data(),
                                                            radius.data(), k.data(), po.data());
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::ICP: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
    return out;
  }

  Matrix3X estimateColorGradients(const Matrix3X& cloud, const Matrix3X& normals, const Matrix3X& colors, double radius,
                                  int max_nn = 30) {
    return std::move(estimateColorGradientsBatch({cloud}, {normals}, {colors}, {radius}, {max_nn})[0]);
  }

  // The same with point-to-plane estimation: dst_normals[b] holds one normal per point of dst[b], used as given.
  std::vector<ICPResult> registrationICPBatch(const std::vector<Matrix3X>& src, const std::vector<Matrix3X>& dst,
                                              const std::vector<Matrix3X>& dst_normals,
                                              const std::vector<double>& max_correspondence_distance,
                                              const std::vector<Matrix4>& init,
                                              const std::vector<TransformationEstimationPointToPlane>& estimation,
                                              const std::vector<ICPConvergenceCriteria>& criteria) {
    const size_t b = src.size();
    if (dst.size() != b || dst_normals.size() != b || estimation.size() != b)
      throw std::invalid_argument("teaser::ICP: one entry per problem in every argument");
    std::vector<const double*> pn(b);
    std::vector<teaser_icp_estimation_c> est(b);
    for (size_t k = 0; k < b; ++k) {
      if (dst_normals[k].cols() != dst[k].cols())
        throw std::invalid_argument("teaser::ICP: one normal per target point");
      pn[k] = dst_normals[k].data();
      est[k].method = 1;
      est[k].kernel = estimation[k].kernel.kernel;
      est[k].kernel_k = estimation[k].kernel.k;
    }
    return run(src, dst, max_correspondence_distance, init, criteria, pn.data(), est.data());
  }

  // Point-to-plane with target normals the library estimates itself: every estimation[b] carries a normal_search
  // (teaser_hip_icp_batch_auto: the normals go from the normals kernel to the correspondence pass on the device).
  std::vector<ICPResult> registrationICPBatch(const std::vector<Matrix3X>& src, const std::vector<Matrix3X>& dst,
                                              const std::vector<double>& max_correspondence_distance,
                                              const std::vector<Matrix4>& init,
                                              const std::vector<TransformationEstimationPointToPlane>& estimation,
                                              const std::vector<ICPConvergenceCriteria>& criteria) {
    const size_t b = src.size();
    if (dst.size() != b || estimation.size() != b)
      throw std::invalid_argument("teaser::ICP: one entry per problem in every argument");
    std::vector<teaser_icp_estimation_c> est(b);
    std::vector<teaser_icp_normal_search_c> rec(b);
    for (size_t k = 0; k < b; ++k) {
      est[k].method = 1;
      est[k].kernel = estimation[k].kernel.kernel;
      est[k].kernel_k = estimation[k].kernel.k;
      rec[k] = estimation[k].normal_search.rec;
    }
    return run(src, dst, max_correspondence_distance, init, criteria, nullptr, est.data(), nullptr, nullptr, rec.data());
  }

  // Normals of many clouds in one launch sequence (include/teaser_hip.h, "Normal estimation"); result c is identical
  // to cloud c estimated alone.
  std::vector<Normals> estimateNormalsBatch(const std::vector<Matrix3X>& clouds, const std::vector<NormalSearch>& search,
                                            bool covariances = false, bool eigenvalues = false) {
    const size_t b = clouds.size();
    if (search.size() != b) throw std::invalid_argument("teaser::ICP: one entry per cloud in every argument");
    std::vector<const double*> pp(b);
    std::vector<int32_t> n(b);
    std::vector<teaser_icp_normal_search_c> rec(b);
    std::vector<Normals> out(b);
    std::vector<double*> pn(b), pc(b), pe(b);
    for (size_t c = 0; c < b; ++c) {
      pp[c] = clouds[c].data();
      n[c] = (int32_t)clouds[c].cols();
      rec[c] = search[c].rec;
      out[c].normals = Matrix3X(3, clouds[c].cols());
      if (covariances) out[c].covariances.resize(9 * (size_t)n[c]);
      if (eigenvalues) out[c].eigenvalues.resize(3 * (size_t)n[c]);
      pn[c] = out[c].normals.data();
      pc[c] = out[c].covariances.data();
      pe[c] = out[c].eigenvalues.data();
    }
    const int32_t rc = teaser_hip_icp_normals_batch(h_, (int32_t)b, pp.data(), n.data(), rec.data(), pn.data(),
                                                    covariances ? pc.data() : nullptr, eigenvalues ? pe.data() : nullptr);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::ICP: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
    return out;
  }

  Normals estimateNormals(const Matrix3X& cloud, const NormalSearch& search, bool covariances = false,
                          bool eigenvalues = false) {
    return std::move(estimateNormalsBatch({cloud}, {search}, covariances, eigenvalues)[0]);
  }

  // Open3D's evaluate_registration for many pairs in one launch sequence: the correspondences, fitness and inlier RMSE
  // of the given poses (registrationICPBatch with max_iteration = 0).
  std::vector<ICPResult> evaluateRegistrationBatch(const std::vector<Matrix3X>& src, const std::vector<Matrix3X>& dst,
                                                   const std::vector<double>& max_correspondence_distance,
                                                   const std::vector<Matrix4>& transformation) {
    ICPConvergenceCriteria none;
    none.max_iteration = 0;
    return run(src, dst, max_correspondence_distance, transformation,
               std::vector<ICPConvergenceCriteria>(src.size(), none), nullptr, nullptr);
  }

  ICPResult evaluateRegistration(const Matrix3X& src, const Matrix3X& dst, double max_correspondence_distance,
                                 const Matrix4& transformation = Matrix4::Identity()) {
    return evaluateRegistrationBatch({src}, {dst}, {max_correspondence_distance}, {transformation})[0];
  }

  // The information matrices of many registered pairs in one launch sequence (include/teaser_hip.h, "Information
  // matrices"; Open3D's GetInformationMatrixFromPointClouds); matrix b is identical to pair b evaluated alone.
  // evaluation: NULL, or receives what evaluateRegistrationBatch returns for the same arguments.
  std::vector<Matrix6> getInformationMatrixFromPointCloudsBatch(const std::vector<Matrix3X>& src,
                                                                const std::vector<Matrix3X>& dst,
                                                                const std::vector<double>& max_correspondence_distance,
                                                                const std::vector<Matrix4>& transformation,
                                                                std::vector<ICPResult>* evaluation = nullptr) {
    const size_t b = src.size();
    if (dst.size() != b || max_correspondence_distance.size() != b || transformation.size() != b)
      throw std::invalid_argument("teaser::ICP: one entry per problem in every argument");
    std::vector<const double*> ps(b), pd(b);
    std::vector<int32_t> ns(b), nd(b);
    std::vector<double> T(16 * b), info(36 * b);
    std::vector<std::vector<int32_t>> corr(b);
    std::vector<int32_t*> pc(b);
    for (size_t k = 0; k < b; ++k) {
      ps[k] = src[k].data();
      pd[k] = dst[k].data();
      ns[k] = (int32_t)src[k].cols();
      nd[k] = (int32_t)dst[k].cols();
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) T[16 * k + (size_t)(4 * r + c)] = transformation[k](r, c);
      if (evaluation) corr[k].resize(2 * (size_t)(ns[k] > 0 ? ns[k] : 1));
      pc[k] = evaluation ? corr[k].data() : nullptr;
    }
    std::vector<teaser_icp_result_c> out(b);
    const int32_t rc = teaser_hip_icp_information_batch(h_, (int32_t)b, ps.data(), ns.data(), pd.data(), nd.data(),
                                                        T.data(), max_correspondence_distance.data(), info.data(),
                                                        evaluation ? out.data() : nullptr, evaluation ? pc.data() : nullptr);
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::ICP: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
    std::vector<Matrix6> res(b);
    for (size_t k = 0; k < b; ++k)
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) res[k](r, c) = info[36 * k + (size_t)(6 * r + c)];
    if (evaluation) *evaluation = unpack(out, corr);
    return res;
  }

  Matrix6 getInformationMatrixFromPointClouds(const Matrix3X& src, const Matrix3X& dst,
                                              double max_correspondence_distance, const Matrix4& transformation) {
    return getInformationMatrixFromPointCloudsBatch({src}, {dst}, {max_correspondence_distance}, {transformation})[0];
  }

  ICPResult registrationICP(const Matrix3X& src, const Matrix3X& dst, double max_correspondence_distance,
                            const Matrix4& init, const TransformationEstimationPointToPlane& estimation,
                            const ICPConvergenceCriteria& criteria = ICPConvergenceCriteria()) {
    return registrationICPBatch({src}, {dst}, {max_correspondence_distance}, {init}, {estimation}, {criteria})[0];
  }

  ICPResult registrationICP(const Matrix3X& src, const Matrix3X& dst, double max_correspondence_distance,
                            const Matrix4& init = Matrix4::Identity(),
                            const ICPConvergenceCriteria& criteria = ICPConvergenceCriteria()) {
    return registrationICPBatch({src}, {dst}, {max_correspondence_distance}, {init}, {criteria})[0];
  }

  ICPResult registrationICP(const Matrix3X& src, const Matrix3X& dst, const Matrix3X& dst_normals,
                            double max_correspondence_distance, const Matrix4& init,
                            const TransformationEstimationPointToPlane& estimation,
                            const ICPConvergenceCriteria& criteria = ICPConvergenceCriteria()) {
    return registrationICPBatch({src}, {dst}, {dst_normals}, {max_correspondence_distance}, {init}, {estimation},
                                {criteria})[0];
  }

  ICPResult registrationICP(const Matrix3X& src, const Matrix3X& dst, const Covariances& src_cov,
                            const Covariances& dst_cov, double max_correspondence_distance, const Matrix4& init,
                            const TransformationEstimationForGeneralizedICP& estimation,
                            const ICPConvergenceCriteria& criteria = ICPConvergenceCriteria()) {
    return registrationICPBatch({src}, {dst}, {src_cov}, {dst_cov}, {max_correspondence_distance}, {init},
                                {estimation}, {criteria})[0];
  }

 private:
  // What a coloured call hands to teaser_hip_icp_batch_color besides run's own arguments.
  struct ColorArgs {
    std::vector<const double*> src_colors, dst_colors, dst_gradients;
    std::vector<teaser_icp_color_c> rec;
  };

  std::vector<ICPResult> run(const std::vector<Matrix3X>& src, const std::vector<Matrix3X>& dst,
                             const std::vector<double>& max_correspondence_distance,
                             const std::vector<Matrix4>& init, const std::vector<ICPConvergenceCriteria>& criteria,
                             const double* const* normals, const teaser_icp_estimation_c* est,
                             const double* const* src_cov = nullptr, const double* const* dst_cov = nullptr,
                             const teaser_icp_normal_search_c* normal_search = nullptr,
                             const ColorArgs* color = nullptr) {
    const size_t b = src.size();
    if (dst.size() != b || max_correspondence_distance.size() != b || init.size() != b || criteria.size() != b)
      throw std::invalid_argument("teaser::ICP: one entry per problem in every argument");
    std::vector<const double*> ps(b), pd(b);
    std::vector<int32_t> ns(b), nd(b);
    std::vector<double> T(16 * b);
    std::vector<teaser_icp_params_c> params(b);
    std::vector<std::vector<int32_t>> corr(b);
    std::vector<int32_t*> pc(b);
    for (size_t k = 0; k < b; ++k) {
      ps[k] = src[k].data();
      pd[k] = dst[k].data();
      ns[k] = (int32_t)src[k].cols();
      nd[k] = (int32_t)dst[k].cols();
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) T[16 * k + (size_t)(4 * r + c)] = init[k](r, c);
      params[k].max_correspondence_distance = max_correspondence_distance[k];
      params[k].max_iteration = criteria[k].max_iteration;
      params[k].relative_fitness = criteria[k].relative_fitness;
      params[k].relative_rmse = criteria[k].relative_rmse;
      corr[k].resize(2 * (size_t)(ns[k] > 0 ? ns[k] : 1));
      pc[k] = corr[k].data();
    }
    std::vector<teaser_icp_result_c> out(b);
    const int32_t rc =
        color ? teaser_hip_icp_batch_color(h_, (int32_t)b, ps.data(), ns.data(), pd.data(), nd.data(), T.data(),
                                           params.data(), out.data(), pc.data(), normals, est, src_cov, dst_cov,
                                           color->src_colors.data(), color->dst_colors.data(),
                                           color->dst_gradients.data(), color->rec.data())
        : normal_search
            ? teaser_hip_icp_batch_auto(h_, (int32_t)b, ps.data(), ns.data(), pd.data(), nd.data(), T.data(),
                                        params.data(), out.data(), pc.data(), normals, est, src_cov, dst_cov,
                                        normal_search)
        : src_cov ? teaser_hip_icp_batch_cov(h_, (int32_t)b, ps.data(), ns.data(), pd.data(), nd.data(), T.data(),
                                           params.data(), out.data(), pc.data(), normals, est, src_cov, dst_cov)
        : est ? teaser_hip_icp_batch_ex(h_, (int32_t)b, ps.data(), ns.data(), pd.data(), nd.data(), T.data(),
                                      params.data(), out.data(), pc.data(), normals, est)
            : teaser_hip_icp_batch(h_, (int32_t)b, ps.data(), ns.data(), pd.data(), nd.data(), T.data(),
                                   params.data(), out.data(), pc.data());
    if (rc != TEASER_HIP_OK)
      throw ICPError(rc, "teaser::ICP: status " + std::to_string(rc) + ": " + teaser_hip_icp_last_error(h_));
    return unpack(out, corr);
  }

  // The records and correspondence buffers of a call as results.
  static std::vector<ICPResult> unpack(const std::vector<teaser_icp_result_c>& out,
                                       const std::vector<std::vector<int32_t>>& corr) {
    const size_t b = out.size();
    std::vector<ICPResult> res(b);
    for (size_t k = 0; k < b; ++k) {
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) res[k].transformation(r, c) = out[k].transformation[4 * r + c];
      res[k].fitness = out[k].fitness;
      res[k].inlier_rmse = out[k].inlier_rmse;
      res[k].iterations = out[k].iterations;
      for (int32_t i = 0; i < out[k].n_correspondences; ++i)
        res[k].correspondence_set.emplace_back(corr[k][(size_t)(2 * i)], corr[k][(size_t)(2 * i + 1)]);
    }
    return res;
  }

  teaser_hip_icp* h_ = nullptr;
};

// Open3D's free function (registration_icp), one problem; creates a handle per call -- keep a teaser::ICP object
// for repeated calls.
inline ICPResult registrationICP(const Matrix3X& src, const Matrix3X& dst, double max_correspondence_distance,
                                 const Matrix4& init = Matrix4::Identity(),
                                 const ICPConvergenceCriteria& criteria = ICPConvergenceCriteria()) {
  ICP icp;
  return icp.registrationICP(src, dst, max_correspondence_distance, init, criteria);
}

// Open3D's registration_icp with TransformationEstimationPointToPlane: dst_normals holds one normal per target point.
inline ICPResult registrationICP(const Matrix3X& src, const Matrix3X& dst, const Matrix3X& dst_normals,
                                 double max_correspondence_distance, const Matrix4& init,
                                 const TransformationEstimationPointToPlane& estimation,
                                 const ICPConvergenceCriteria& criteria = ICPConvergenceCriteria()) {
  ICP icp;
  return icp.registrationICP(src, dst, dst_normals, max_correspondence_distance, init, estimation, criteria);
}

}  // namespace teaser

namespace teaser {

// Open3D's registration_generalized_icp with given covariances, one problem; creates a handle per call.
inline ICPResult registrationICP(const Matrix3X& src, const Matrix3X& dst, const Covariances& src_cov,
                                 const Covariances& dst_cov, double max_correspondence_distance, const Matrix4& init,
                                 const TransformationEstimationForGeneralizedICP& estimation,
                                 const ICPConvergenceCriteria& criteria = ICPConvergenceCriteria()) {
  ICP icp;
  return icp.registrationICP(src, dst, src_cov, dst_cov, max_correspondence_distance, init, estimation, criteria);
}

// Open3D's estimate_normals (+ orient_normals_*), one cloud; creates a handle per call.
inline Normals estimateNormals(const Matrix3X& cloud, const NormalSearch& search, bool covariances = false,
                               bool eigenvalues = false) {
  ICP icp;
  return icp.estimateNormals(cloud, search, covariances, eigenvalues);
}

// Point-to-plane ICP that estimates the target normals itself (estimation.normal_search); creates a handle per call.
inline ICPResult registrationICP(const Matrix3X& src, const Matrix3X& dst, double max_correspondence_distance,
                                 const Matrix4& init, const TransformationEstimationPointToPlane& estimation,
                                 const ICPConvergenceCriteria& criteria = ICPConvergenceCriteria()) {
  ICP icp;
  return icp.registrationICP(src, dst, max_correspondence_distance, init, estimation, criteria);
}

// Open3D's evaluate_registration, one pair; creates a handle per call.
inline ICPResult evaluateRegistration(const Matrix3X& src, const Matrix3X& dst, double max_correspondence_distance,
                                      const Matrix4& transformation = Matrix4::Identity()) {
  ICP icp;
  return icp.evaluateRegistration(src, dst, max_correspondence_distance, transformation);
}

// Open3D's GetInformationMatrixFromPointClouds, one pair; creates a handle per call.
inline Matrix6 getInformationMatrixFromPointClouds(const Matrix3X& src, const Matrix3X& dst,
                                                   double max_correspondence_distance, const Matrix4& transformation) {
  ICP icp;
  return icp.getInformationMatrixFromPointClouds(src, dst, max_correspondence_distance, transformation);
}

// Covariances of one cloud for Generalized ICP, estimated on the GPU; creates a handle per call.
inline Covariances estimateCovariances(const Matrix3X& cloud, double radius, int max_nn = 20, double epsilon = 1e-3) {
  ICP icp;
  return icp.estimateCovariances(cloud, radius, max_nn, epsilon);
}

// Open3D's registration_colored_icp, one problem; creates a handle per call.
inline ICPResult registrationColoredICP(const Matrix3X& src, const Matrix3X& dst, const Matrix3X& src_colors,
                                        const Matrix3X& dst_colors, const Matrix3X& dst_normals,
                                        double max_correspondence_distance, const Matrix4& init = Matrix4::Identity(),
                                        const TransformationEstimationForColoredICP& estimation =
                                            TransformationEstimationForColoredICP(),
                                        const ICPConvergenceCriteria& criteria = ICPConvergenceCriteria()) {
  ICP icp;
  return icp.registrationColoredICP(src, dst, src_colors, dst_colors, dst_normals, max_correspondence_distance, init,
                                    estimation, criteria);
}

}  // namespace teaser
