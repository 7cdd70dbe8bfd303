// teaser::registrationRANSACBasedOnCorrespondence (include/teaser/ransac.h) used like Open3D's
// RegistrationRANSACBasedOnCorrespondence.
//   ransac_example                    an exact quarter turn planted in half of 40 pairs: recovered; the requests that
//                                     are not offered are refused by name; 0 ok, 1 wrong result
//   ransac_example PROBLEM RESULT     reads a problem file (sizes, r, ransac_n, max_iteration, confidence, seed, the two
//                                     checker thresholds (0: off), the points, the pairs) and writes the result record:
//                                     best_trial trials valid_trials n fitness rmse, T, the inlier pairs (%.17g)
// Exit code 77: no MI355X visible (loud failure, no CPU path); 1: any other failure.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "teaser/ransac.h"

int main(int argc, char** argv) {
  try {
    if (argc == 3) {
      FILE* in = std::fopen(argv[1], "r");
      if (!in) return 2;
      int ns = 0, nt = 0, nc = 0;
      double s = 0, d = 0;
      teaser::RANSACOption o;
      bool ok = std::fscanf(in, "%d %d %d %lf %d %d %lf %" SCNu64 " %lf %lf", &ns, &nt, &nc, &o.max_correspondence_distance,
                            &o.ransac_n, &o.criteria.max_iteration, &o.criteria.confidence, &o.seed, &s, &d) == 10;
      if (!ok || ns < 0 || nt < 0 || nc < 0 || ns > (1 << 20) || nt > (1 << 20) || nc > (1 << 20)) return 2;
      teaser::Matrix3X P(3, ns), Q(3, nt);
      for (int i = 0; i < ns; ++i)
        for (int r = 0; r < 3; ++r) ok = ok && std::fscanf(in, "%lf", &P(r, i)) == 1;
      for (int i = 0; i < nt; ++i)
        for (int r = 0; r < 3; ++r) ok = ok && std::fscanf(in, "%lf", &Q(r, i)) == 1;
      teaser::CorrespondenceSet corres((size_t)nc);
      for (auto& c : corres) ok = ok && std::fscanf(in, "%d %d", &c.first, &c.second) == 2;
      std::fclose(in);
      if (!ok) return 2;
      const teaser::CorrespondenceCheckerBasedOnEdgeLength edge(s);
      const teaser::CorrespondenceCheckerBasedOnDistance dist(d);
      o.edge_length = s > 0 ? &edge : nullptr;
      o.distance = d > 0 ? &dist : nullptr;
      teaser::RANSAC ransac;
      const teaser::RANSACResult res = ransac.registrationRANSACBasedOnCorrespondence(P, Q, corres, o);
      FILE* out = std::fopen(argv[2], "w");
      if (!out) return 2;
      std::fprintf(out, "%lld %lld %lld %zu %.17g %.17g\n", (long long)res.best_trial, (long long)res.trials,
                   (long long)res.valid_trials, res.correspondence_set.size(), res.fitness, res.inlier_rmse);
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) std::fprintf(out, "%.17g ", res.transformation(r, c));
      std::fprintf(out, "\n");
      for (const auto& c : res.correspondence_set) std::fprintf(out, "%d %d\n", c.first, c.second);
      std::fclose(out);
      return 0;
    }
    // 40 pairs, the even ones moved by a quarter turn about z and a shift, the odd ones anywhere
    const int n = 40;
    teaser::Matrix3X P(3, n), Q(3, n);
    teaser::CorrespondenceSet corres;
    uint64_t state = 7;
    auto uni = [&]() {
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      return (double)(state >> 40) / 16777216.0 * 2.0 - 1.0;
    };
    for (int i = 0; i < n; ++i) {
      for (int r = 0; r < 3; ++r) P(r, i) = uni(), Q(r, i) = uni();
      if (i % 2 == 0) Q(0, i) = -P(1, i) + 0.25, Q(1, i) = P(0, i) - 0.5, Q(2, i) = P(2, i) + 0.125;
      corres.emplace_back(i, i);
    }
    const teaser::CorrespondenceCheckerBasedOnEdgeLength edge(0.9);
    const teaser::CorrespondenceCheckerBasedOnDistance dist(0.05);
    const teaser::RANSACResult res = teaser::registrationRANSACBasedOnCorrespondence(
        P, Q, corres, 0.01, 3, &edge, &dist, teaser::RANSACConvergenceCriteria(5000, 0.999), /*seed=*/11);
    bool ok = res.correspondence_set.size() >= 20 && res.best_trial >= 0 && res.trials < 5000 &&
              res.valid_trials <= res.trials && res.fitness >= 0.5 && res.inlier_rmse < 1e-9;
    const double want[3][4] = {{0, -1, 0, 0.25}, {1, 0, 0, -0.5}, {0, 0, 1, 0.125}};
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) ok = ok && std::fabs(res.transformation(r, c) - want[r][c]) < 1e-9;
    bool refused = false;
    try {
      teaser::RANSACOption o;
      o.max_correspondence_distance = 0.01;
      o.with_scaling = true;
      teaser::RANSAC r;
      r.registrationRANSACBasedOnCorrespondence(P, Q, corres, o);
    } catch (const teaser::RANSACError& e) {
      refused = e.status() == TEASER_HIP_ERR_BAD_ARG && std::string(e.what()).find("with_scaling") != std::string::npos;
    }
    std::printf("best trial %lld of %lld (%lld valid), %zu inliers, rmse %.3g\n", (long long)res.best_trial,
                (long long)res.trials, (long long)res.valid_trials, res.correspondence_set.size(), res.inlier_rmse);
    return ok && refused ? 0 : 1;
  } catch (const teaser::RANSACError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return std::string(e.what()).find("status 3") != std::string::npos ? 77 : 1;
  }
}
