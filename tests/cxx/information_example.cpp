// teaser::getInformationMatrixFromPointClouds and teaser::evaluateRegistration (include/teaser/icp.h) used like
// Open3D's get_information_matrix_from_point_clouds and evaluate_registration.
//   information_example          a lattice and a shifted copy: every entry of the matrix is known in closed form;
//                                0 ok, 1 wrong result
//   information_example DIR r    reads DIR/src.bin, DIR/dst.bin (n x 3 doubles) and DIR/T.bin (16 doubles, row-major),
//                                prints the 36 entries (row-major) / fitness / rmse / correspondences
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
    if (argc == 3) {
      const std::string dir = argv[1];
      const std::vector<double> s = read_doubles(dir + "/src.bin"), d = read_doubles(dir + "/dst.bin"),
                                t = read_doubles(dir + "/T.bin");
      if (t.size() != 16) return 2;
      teaser::Matrix4 T;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) T(r, c) = t[(size_t)(4 * r + c)];
      std::vector<teaser::ICPResult> ev;
      const teaser::Matrix6 info =
          icp.getInformationMatrixFromPointCloudsBatch({cloud(s)}, {cloud(d)}, {std::atof(argv[2])}, {T}, &ev)[0];
      const teaser::ICPResult res = icp.evaluateRegistration(cloud(s), cloud(d), std::atof(argv[2]), T);
      if (res.fitness != ev[0].fitness || res.inlier_rmse != ev[0].inlier_rmse ||
          res.correspondence_set != ev[0].correspondence_set || res.iterations != 0)
        return 1;
      std::printf("information");
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) std::printf(" %.17g", info(r, c));
      std::printf("\nfitness %.17g\nrmse %.17g\ncorrespondences %zu\n", res.fitness, res.inlier_rmse,
                  res.correspondence_set.size());
      return 0;
    }
    // the lattice {-2 .. 2}^3 as the target, the same points shifted by (-0.5, 0, 0) as the source, T the shift back:
    // SUM q = 0, SUM q_a q_b = 250 (a == b) or 0, |C| = 125
    std::vector<double> s, d;
    for (int i = -2; i <= 2; ++i)
      for (int j = -2; j <= 2; ++j)
        for (int k = -2; k <= 2; ++k) {
          d.insert(d.end(), {(double)i, (double)j, (double)k});
          s.insert(s.end(), {(double)i - 0.5, (double)j, (double)k});
        }
    teaser::Matrix4 T = teaser::Matrix4::Identity();
    T(0, 3) = 0.5;
    const teaser::Matrix6 info = teaser::getInformationMatrixFromPointClouds(cloud(s), cloud(d), 0.5, T);
    const teaser::ICPResult res = teaser::evaluateRegistration(cloud(s), cloud(d), 0.5, T);
    bool ok = res.fitness == 1.0 && res.inlier_rmse == 0.0 && res.correspondence_set.size() == 125;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) ok = ok && info(r, c) == (r != c ? 0.0 : r < 3 ? 500.0 : 125.0);
    // under the identity the nearest targets are exactly r away, and a point at r is no match
    const teaser::ICPResult off = teaser::evaluateRegistration(cloud(s), cloud(d), 0.5);
    ok = ok && off.fitness == 0.0 && off.correspondence_set.empty();
    std::printf("information(0,0) %.1f information(5,5) %.1f fitness %.3f\n", info(0, 0), info(5, 5), res.fitness);
    return ok ? 0 : 1;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
