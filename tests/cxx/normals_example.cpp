// teaser::estimateNormals (include/teaser/icp.h) used like Open3D's pcd.estimate_normals, and point-to-plane ICP that
// estimates its own target normals.  Without arguments: a jittered plane z = 0, whose normals must be +-(0, 0, 1) and,
// oriented along +z, (0, 0, 1).  With a directory (src.bin, dst.bin, init.bin: float64) plus the ICP radius and the
// normal-search radius: prints the normals of dst (hybrid and k-NN search) and the ICP result as hexadecimal floats,
// which tests/test_gpu_normals_cxx.py compares with the restatement and with the Python interface.
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "teaser/icp.h"

static std::vector<double> read(const std::string& path) {
  std::vector<double> v;
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return v;
  double x;
  while (std::fread(&x, sizeof(x), 1, f) == 1) v.push_back(x);
  std::fclose(f);
  return v;
}

static teaser::Matrix3X cloud(const std::vector<double>& xyz) {
  teaser::Matrix3X m(3, (int64_t)(xyz.size() / 3));
  for (int64_t i = 0; i < m.cols(); ++i)
    for (int r = 0; r < 3; ++r) m(r, i) = xyz[(size_t)(3 * i + r)];
  return m;
}

static void print(const char* name, const double* v, size_t n) {
  std::printf("%s", name);
  for (size_t k = 0; k < n; ++k) std::printf(" %a", v[k]);
  std::printf("\n");
}

static int fail(const char* what) {
  std::fprintf(stderr, "normals_example: %s\n", what);
  return 1;
}

int main(int argc, char** argv) {
  try {
    if (argc == 1) {
      std::vector<double> xyz;
      for (int a = 0; a < 12; ++a)
        for (int b = 0; b < 12; ++b) {
          const double p[3] = {0.1 * a + 0.003 * ((7 * a + 3 * b) % 5), 0.1 * b + 0.002 * ((5 * a + b) % 7), 0.0};
          xyz.insert(xyz.end(), p, p + 3);
        }
      const teaser::Matrix3X P = cloud(xyz);
      teaser::ICP icp;
      const auto both = icp.estimateNormalsBatch(
          {P, cloud({}), P}, {teaser::NormalSearch::Hybrid(0.25, 30), teaser::NormalSearch::KNN(5),
                              teaser::NormalSearch::KNN(10).along(0, 0, 1)}, true, true);
      if (both[1].normals.cols() != 0) return fail("an empty cloud has no normals");
      for (int64_t i = 0; i < P.cols(); ++i) {
        if (both[0].normals(0, i) != 0 || both[0].normals(1, i) != 0 || std::fabs(both[0].normals(2, i)) != 1)
          return fail("the plane's normals are +-(0, 0, 1)");
        if (both[2].normals(2, i) != 1) return fail("along +z the plane's normals are (0, 0, 1)");
        if (both[0].eigenvalues[(size_t)(3 * i)] != 0 || !(both[0].eigenvalues[(size_t)(3 * i + 1)] > 0))
          return fail("the plane's smallest eigenvalue is 0");
        if (both[0].covariances[(size_t)(9 * i + 8)] != 0) return fail("the plane's covariance has no z part");
      }
      const teaser::Normals alone = teaser::estimateNormals(P, teaser::NormalSearch::Hybrid(0.25, 30));
      for (int64_t i = 0; i < P.cols(); ++i)
        if (alone.normals(2, i) != both[0].normals(2, i)) return fail("the single call equals the batched one");
      bool threw = false;
      try {
        icp.estimateNormals(P, teaser::NormalSearch::KNN(2));
      } catch (const teaser::ICPError& e) {
        threw = e.status() == TEASER_HIP_ERR_BAD_ARG;
      }
      if (!threw) return fail("max_nn = 2 throws BAD_ARG");
      std::printf("checks 1\n");
      return 0;
    }
    if (argc != 4) return fail("usage: normals_example [DIR ICP_RADIUS NORMAL_RADIUS]");
    const std::string dir = argv[1];
    const double r = std::strtod(argv[2], nullptr), nr = std::strtod(argv[3], nullptr);
    const teaser::Matrix3X P = cloud(read(dir + "/src.bin")), Q = cloud(read(dir + "/dst.bin"));
    const std::vector<double> t = read(dir + "/init.bin");
    if (t.size() != 16) return fail("init.bin holds 16 doubles");
    teaser::Matrix4 init = teaser::Matrix4::Identity();
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b) init(a, b) = t[(size_t)(4 * a + b)];
    teaser::ICP icp;
    const teaser::NormalSearch hyb = teaser::NormalSearch::Hybrid(nr, 30).along(0, 0, 1);
    const teaser::Normals h = icp.estimateNormals(Q, hyb, true, true);
    const teaser::Normals k = icp.estimateNormals(Q, teaser::NormalSearch::KNN(30).towards(0, 0, 0));
    print("hybrid_normals", h.normals.data(), 3 * (size_t)Q.cols());
    print("hybrid_covariances", h.covariances.data(), h.covariances.size());
    print("hybrid_eigenvalues", h.eigenvalues.data(), h.eigenvalues.size());
    print("knn_normals", k.normals.data(), 3 * (size_t)Q.cols());
    const teaser::ICPResult res =
        icp.registrationICP(P, Q, r, init, teaser::TransformationEstimationPointToPlane(teaser::TukeyLoss(0.1), hyb));
    double T[16];
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b) T[4 * a + b] = res.transformation(a, b);
    print("T", T, 16);
    print("fitness", &res.fitness, 1);
    print("rmse", &res.inlier_rmse, 1);
    std::printf("iterations %d\ncorrespondences %zu\n", res.iterations, res.correspondence_set.size());
    // the given-normals form on the estimated normals: the same bits
    const teaser::ICPResult two = icp.registrationICP(
        P, Q, h.normals, r, init, teaser::TransformationEstimationPointToPlane(teaser::TukeyLoss(0.1)));
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b)
        if (two.transformation(a, b) != res.transformation(a, b)) return fail("the two-call form gives other bits");
    if (two.iterations != res.iterations || two.correspondence_set != res.correspondence_set)
      return fail("the two-call form gives another result");
    return 0;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
