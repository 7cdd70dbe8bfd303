// teaser::registrationColoredICP (include/teaser/icp.h) used like Open3D's registration_colored_icp.
//   colored_icp_example                      a synthetic textured, gently curved surface and a known pose that slides
//                                            along it: Colored ICP recovers the pose (point-to-plane is printed
//                                            beside it); 0 ok, 1 wrong result
//   colored_icp_example DIR r max_iteration  reads DIR/src.bin, DIR/dst.bin, DIR/src_colors.bin, DIR/dst_colors.bin,
//                                            DIR/dst_normals.bin (n x 3 doubles each), refines from the identity with
//                                            the default estimation, prints T / fitness / rmse / iterations /
//                                            correspondences, then the gradients of the target's first three points
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

static double pose_error(const teaser::Matrix4& T, double c, double sn, double tx, double ty, double tz) {
  const double want[16] = {c, -sn, 0, tx, sn, c, 0, ty, 0, 0, 1, tz, 0, 0, 0, 1};
  double e = 0;
  for (int r = 0; r < 4; ++r)
    for (int k = 0; k < 4; ++k) e += (T(r, k) - want[4 * r + k]) * (T(r, k) - want[4 * r + k]);
  return std::sqrt(e);
}

int main(int argc, char** argv) {
  try {
    teaser::ICP icp;
    if (argc == 4) {
      const std::string dir = argv[1];
      const teaser::Matrix3X s = cloud(read_doubles(dir + "/src.bin")), d = cloud(read_doubles(dir + "/dst.bin")),
                             sc = cloud(read_doubles(dir + "/src_colors.bin")),
                             dc = cloud(read_doubles(dir + "/dst_colors.bin")),
                             dn = cloud(read_doubles(dir + "/dst_normals.bin"));
      teaser::ICPConvergenceCriteria crit;
      crit.max_iteration = std::atoi(argv[3]);
      const double r = std::atof(argv[2]);
      const teaser::ICPResult res = icp.registrationColoredICP(s, d, sc, dc, dn, r, teaser::Matrix4::Identity(),
                                                               teaser::TransformationEstimationForColoredICP(), crit);
      std::printf("T");
      for (int a = 0; a < 4; ++a)
        for (int c = 0; c < 4; ++c) std::printf(" %.17g", res.transformation(a, c));
      std::printf("\nfitness %.17g\nrmse %.17g\niterations %d\ncorrespondences %zu\n", res.fitness, res.inlier_rmse,
                  res.iterations, res.correspondence_set.size());
      const teaser::Matrix3X g = icp.estimateColorGradients(d, dn, dc, 2 * r);
      std::printf("gradients");
      for (int64_t i = 0; i < 3 && i < g.cols(); ++i)
        for (int c = 0; c < 3; ++c) std::printf(" %.17g", g(c, i));
      std::printf("\n");
      return 0;
    }
    // z = 0.05 sin(1.5 x) cos(1.2 y) on a lattice with its analytic normals and the intensity
    // 0.5 + 0.2 sin 4x + 0.2 cos 3y; the source: the same surface at other points, moved back by a known pose
    const double c = std::cos(0.0174), sn = std::sin(0.0174), tx = 0.03, ty = -0.02, tz = 0.002;
    std::vector<double> s, d, n, sc, dc;
    auto surface = [](double x, double y) { return 0.05 * std::sin(1.5 * x) * std::cos(1.2 * y); };
    auto texture = [](double x, double y) { return 0.5 + 0.2 * std::sin(4 * x) + 0.2 * std::cos(3 * y); };
    for (int i = 0; i < 48; ++i)
      for (int j = 0; j < 48; ++j) {
        const double x = -1.0 + 2.0 * i / 47, y = -1.0 + 2.0 * j / 47;
        const double zx = 0.075 * std::cos(1.5 * x) * std::cos(1.2 * y), zy = -0.06 * std::sin(1.5 * x) * std::sin(1.2 * y);
        const double len = std::sqrt(zx * zx + zy * zy + 1.0);
        d.insert(d.end(), {x, y, surface(x, y)});
        n.insert(n.end(), {-zx / len, -zy / len, 1.0 / len});
        dc.insert(dc.end(), 3, texture(x, y));
      }
    for (int i = 0; i < 38; ++i)
      for (int j = 0; j < 38; ++j) {
        const double x = -0.9 + 0.0473 * i + 0.011, y = -0.9 + 0.0473 * j + 0.017;
        const double u = x - tx, v = y - ty, w = surface(x, y) - tz;  // source = R^T (q - t)
        s.insert(s.end(), {c * u + sn * v, -sn * u + c * v, w});
        sc.insert(sc.end(), 3, texture(x, y));
      }
    teaser::ICPConvergenceCriteria crit;
    crit.max_iteration = 50;
    const teaser::ICPResult col = teaser::registrationColoredICP(cloud(s), cloud(d), cloud(sc), cloud(dc), cloud(n), 0.08,
                                                                 teaser::Matrix4::Identity(),
                                                                 teaser::TransformationEstimationForColoredICP(), crit);
    const teaser::ICPResult pl =
        icp.registrationICP(cloud(s), cloud(d), cloud(n), 0.08, teaser::Matrix4::Identity(),
                            teaser::TransformationEstimationPointToPlane(), crit);
    const double ec = pose_error(col.transformation, c, sn, tx, ty, tz), ep = pose_error(pl.transformation, c, sn, tx, ty, tz);
    std::printf("coloured: fitness %.6f error %.3g iterations %d; point-to-plane: error %.3g iterations %d\n",
                col.fitness, ec, col.iterations, ep, pl.iterations);
    return col.fitness == 1.0 && ec < 1e-3 ? 0 : 1;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
