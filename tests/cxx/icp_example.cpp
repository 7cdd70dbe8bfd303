// teaser::registrationICP (include/teaser/icp.h) used like Open3D's registration_icp.
//   icp_example                      synthetic pair with a known pose; 0 ok, 1 wrong result
//   icp_example DIR r max_iteration  reads DIR/src.bin, DIR/dst.bin (n x 3 doubles) and DIR/init.bin (16 doubles,
//                                    row-major), refines, prints T / fitness / rmse / iterations / correspondences
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
    if (argc == 4) {
      const std::string dir = argv[1];
      const std::vector<double> s = read_doubles(dir + "/src.bin"), d = read_doubles(dir + "/dst.bin"),
                                t = read_doubles(dir + "/init.bin");
      if (t.size() != 16) return 2;
      teaser::Matrix4 init;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) init(r, c) = t[(size_t)(4 * r + c)];
      teaser::ICPConvergenceCriteria crit;
      crit.max_iteration = std::atoi(argv[3]);
      const teaser::ICPResult res = icp.registrationICP(cloud(s), cloud(d), std::atof(argv[2]), init, crit);
      std::printf("T");
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) std::printf(" %.17g", res.transformation(r, c));
      std::printf("\nfitness %.17g\nrmse %.17g\niterations %d\ncorrespondences %zu\n", res.fitness, res.inlier_rmse,
                  res.iterations, res.correspondence_set.size());
      return 0;
    }
    // a grid of points, moved by a small known pose
    std::vector<double> s, d;
    const double c = std::cos(0.03), sn = std::sin(0.03);
    for (int i = 0; i < 10; ++i)
      for (int j = 0; j < 10; ++j)
        for (int k = 0; k < 10; ++k) {
          const double x = 0.1 * i, y = 0.1 * j + 0.01 * i * i, z = 0.1 * k + 0.02 * j * k;
          s.insert(s.end(), {x, y, z});
          d.insert(d.end(), {c * x - sn * y + 0.01, sn * x + c * y - 0.005, z + 0.002});
        }
    const teaser::ICPResult res = teaser::registrationICP(cloud(s), cloud(d), 0.05);
    const bool ok = res.fitness == 1.0 && res.inlier_rmse < 1e-9 && std::fabs(res.transformation(0, 3) - 0.01) < 1e-9;
    std::printf("fitness %.6f rmse %.3g iterations %d\n", res.fitness, res.inlier_rmse, res.iterations);
    return ok ? 0 : 1;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
