// teaser::registrationICP with TransformationEstimationForGeneralizedICP (include/teaser/icp.h) used like Open3D's
// registration_generalized_icp.
//   icp_gicp_example                                 synthetic curved surface, covariances from its analytic normals
//                                                    (teaser::covariancesFromNormals) and a known pose; then the same
//                                                    with covariances estimated on the GPU; 0 ok, 1 wrong result
//   icp_gicp_example DIR r max_iteration radius nn   reads DIR/src.bin, DIR/dst.bin (n x 3 doubles) and DIR/init.bin
//                                                    (16 doubles, row-major), estimates both clouds' covariances with
//                                                    (radius, nn, 1e-3), refines, prints T / fitness / rmse /
//                                                    iterations / correspondences
// Exit code 77: no MI355X visible (loud failure, no CPU path); 1: any other failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "teaser/icp.h"

static std::vector<double> read_doubles(const std::string& path) {
  std::vector<double> v;
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return v;
  double x;
  while (std::fread(&x, sizeof(double), 1, f) == 1) v.push_back(x);
  std::fclose(f);
  return v;
}

static teaser::Matrix3X cloud(const std::vector<double>& xyz) {
  teaser::Matrix3X m(3, (int64_t)(xyz.size() / 3));
  for (int64_t i = 0; i < m.cols(); ++i)
    for (int r = 0; r < 3; ++r) m(r, i) = xyz[(size_t)(3 * i + r)];
  return m;
}

int main(int argc, char** argv) {
  try {
    teaser::ICP icp;
    const teaser::TransformationEstimationForGeneralizedICP gicp;
    if (argc == 6) {
      const std::string dir = argv[1];
      const std::vector<double> s = read_doubles(dir + "/src.bin"), d = read_doubles(dir + "/dst.bin"),
                                t = read_doubles(dir + "/init.bin");
      if (t.size() != 16) return 2;
      teaser::Matrix4 init;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) init(r, c) = t[(size_t)(4 * r + c)];
      teaser::ICPConvergenceCriteria crit;
      crit.max_iteration = std::atoi(argv[3]);
      const double radius = std::atof(argv[4]);
      const int nn = std::atoi(argv[5]);
      const std::vector<teaser::Covariances> cov =
          icp.estimateCovariancesBatch({cloud(s), cloud(d)}, {radius, radius}, {nn, nn}, {gicp.epsilon, gicp.epsilon});
      const teaser::ICPResult res =
          icp.registrationICP(cloud(s), cloud(d), cov[0], cov[1], std::atof(argv[2]), init, gicp, crit);
      std::printf("T");
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) std::printf(" %.17g", res.transformation(r, c));
      std::printf("\nfitness %.17g\nrmse %.17g\niterations %d\ncorrespondences %zu\n", res.fitness, res.inlier_rmse,
                  res.iterations, res.correspondence_set.size());
      return 0;
    }
    // the surface z = 0.2 sin(2 x) cos(1.5 y) on a grid with its analytic normals, and the same points moved back by
    // a small known pose (a rotation about z, so the source normals are the target's rotated back) as the source
    std::vector<double> s, d, n, ns;
    const double c = std::cos(0.01), sn = std::sin(0.01);
    for (int i = 0; i < 40; ++i)
      for (int j = 0; j < 40; ++j) {
        const double x = 0.05 * i - 1.0, y = 0.05 * j - 1.0, z = 0.2 * std::sin(2 * x) * std::cos(1.5 * y);
        const double zx = 0.4 * std::cos(2 * x) * std::cos(1.5 * y), zy = -0.3 * std::sin(2 * x) * std::sin(1.5 * y);
        const double len = std::sqrt(zx * zx + zy * zy + 1.0);
        const double n0 = -zx / len, n1 = -zy / len, n2 = 1.0 / len;
        d.insert(d.end(), {x, y, z});
        n.insert(n.end(), {n0, n1, n2});
        const double u = x - 0.004, v = y + 0.003, w = z - 0.002;  // source = R^T (q - t)
        s.insert(s.end(), {c * u + sn * v, -sn * u + c * v, w});
        ns.insert(ns.end(), {c * n0 + sn * n1, -sn * n0 + c * n1, n2});
      }
    teaser::ICPConvergenceCriteria crit;
    crit.max_iteration = 50;
    const teaser::ICPResult res = teaser::registrationICP(
        cloud(s), cloud(d), teaser::covariancesFromNormals(cloud(ns)), teaser::covariancesFromNormals(cloud(n)), 0.04,
        teaser::Matrix4::Identity(), gicp, crit);
    bool ok = res.fitness == 1.0 && res.inlier_rmse < 1e-5 && std::fabs(res.transformation(0, 3) - 0.004) < 1e-5 &&
              std::fabs(res.transformation(1, 0) - sn) < 1e-5;
    std::printf("fitness %.6f rmse %.3g iterations %d\n", res.fitness, res.inlier_rmse, res.iterations);
    const teaser::ICPResult est =
        icp.registrationICP(cloud(s), cloud(d), icp.estimateCovariances(cloud(s), 0.12),
                            teaser::estimateCovariances(cloud(d), 0.12), 0.04, teaser::Matrix4::Identity(), gicp, crit);
    ok = ok && est.fitness == 1.0 && est.inlier_rmse < 1e-3 && std::fabs(est.transformation(0, 3) - 0.004) < 1e-3;
    std::printf("estimated covariances: fitness %.6f rmse %.3g iterations %d\n", est.fitness, est.inlier_rmse,
                est.iterations);
    return ok ? 0 : 1;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
