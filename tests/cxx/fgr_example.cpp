// teaser::registrationFGRBasedOnCorrespondence (include/teaser/fgr.h) used like Open3D's
// FastGlobalRegistrationBasedOnCorrespondence.
//   fgr_example                    an exact quarter turn planted in 30 of 40 pairs: recovered; an empty cloud is refused
//                                  by name; 0 ok, 1 wrong result
//   fgr_example PROBLEM RESULT     reads a problem file (sizes, the options, the points, the pairs) and writes the result:
//                                  iterations n_corr failed_solves flags fitness rmse final_mu, T, the correspondence set
//                                  of the evaluation (%.17g)
// Exit code 77: no MI355X visible (loud failure, no CPU path); 1: any other failure.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "teaser/fgr.h"

int main(int argc, char** argv) {
  try {
    if (argc == 3) {
      FILE* in = std::fopen(argv[1], "r");
      if (!in) return 2;
      int ns = 0, nt = 0, nc = 0, abs_scale = 0, dec = 0, tuple = 0;
      teaser::FastGlobalRegistrationOption o;
      bool ok = std::fscanf(in, "%d %d %d %lf %d %d %lf %d %lf %d %" SCNu64, &ns, &nt, &nc, &o.division_factor, &abs_scale,
                            &dec, &o.maximum_correspondence_distance, &o.iteration_number, &o.tuple_scale, &tuple,
                            &o.seed) == 11;
      if (!ok || ns < 0 || nt < 0 || nc < 0 || ns > (1 << 20) || nt > (1 << 20) || nc > (1 << 20)) return 2;
      o.use_absolute_scale = abs_scale != 0;
      o.decrease_mu = dec != 0;
      o.tuple_test = tuple != 0;
      teaser::Matrix3X P(3, ns), Q(3, nt);
      for (int i = 0; i < ns; ++i)
        for (int r = 0; r < 3; ++r) ok = ok && std::fscanf(in, "%lf", &P(r, i)) == 1;
      for (int i = 0; i < nt; ++i)
        for (int r = 0; r < 3; ++r) ok = ok && std::fscanf(in, "%lf", &Q(r, i)) == 1;
      std::vector<std::pair<int, int>> corres((size_t)nc);
      for (auto& c : corres) ok = ok && std::fscanf(in, "%d %d", &c.first, &c.second) == 2;
      std::fclose(in);
      if (!ok) return 2;
      teaser::FGR fgr;
      const teaser::FGRResult res = fgr.registrationFGRBasedOnCorrespondence(P, Q, corres, o);
      FILE* out = std::fopen(argv[2], "w");
      if (!out) return 2;
      std::fprintf(out, "%d %d %d %d %zu %.17g %.17g %.17g\n", res.record.iterations, res.record.n_corr,
                   res.record.failed_solves, res.record.flags, res.correspondence_set.size(), res.fitness,
                   res.inlier_rmse, res.record.final_mu);
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) std::fprintf(out, "%.17g ", res.transformation(r, c));
      std::fprintf(out, "\n");
      for (const auto& c : res.correspondence_set) std::fprintf(out, "%d %d\n", c.first, c.second);
      std::fclose(out);
      return 0;
    }
    // 40 pairs, 30 of them moved by a quarter turn about z and a shift, every fourth one anywhere
    const int n = 40;
    teaser::Matrix3X P(3, n), Q(3, n);
    std::vector<std::pair<int, int>> corres;
    uint64_t state = 7;
    auto uni = [&]() {
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      return (double)(state >> 40) / 16777216.0 * 2.0 - 1.0;
    };
    for (int i = 0; i < n; ++i) {
      for (int r = 0; r < 3; ++r) P(r, i) = uni(), Q(r, i) = uni();
      if (i % 4 != 0) Q(0, i) = -P(1, i) + 0.25, Q(1, i) = P(0, i) - 0.5, Q(2, i) = P(2, i) + 0.125;
      corres.emplace_back(i, i);
    }
    teaser::FastGlobalRegistrationOption o;
    o.tuple_test = false;
    const teaser::FGRResult res = teaser::registrationFGRBasedOnCorrespondence(P, Q, corres, o);
    bool ok = res.record.iterations == 64 && res.record.failed_solves == 0 && res.record.flags == 0 &&
              res.record.n_corr == n && res.correspondence_set.size() >= 30 && res.fitness >= 0.75;
    const double want[3][4] = {{0, -1, 0, 0.25}, {1, 0, 0, -0.5}, {0, 0, 1, 0.125}};
    double worst = 0;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) worst = std::fmax(worst, std::fabs(res.transformation(r, c) - want[r][c]));
    ok = ok && worst < 1e-2;  // the outliers keep a weight of (mu / (e e + mu))^2: the bound of the restatement's test
    bool refused = false;
    try {
      teaser::FGR f;
      f.registrationFGRBasedOnCorrespondence(teaser::Matrix3X(3, 0), Q, {}, o);
    } catch (const teaser::FGRError& e) {
      refused = e.status() == TEASER_HIP_ERR_BAD_ARG && std::string(e.what()).find("source is empty") != std::string::npos;
    }
    std::printf("%d iterations, final mu %.6g, %zu inliers, fitness %.3g, rmse %.3g, |dT| %.3g\n", res.record.iterations,
                res.record.final_mu, res.correspondence_set.size(), res.fitness, res.inlier_rmse, worst);
    return ok && refused ? 0 : 1;
  } catch (const teaser::FGRError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return std::string(e.what()).find("status 3") != std::string::npos ? 77 : 1;
  }
}
