// teaser::segmentPlane (include/teaser/plane.h) used like Open3D's PointCloud::SegmentPlane.
//   plane_example                  a floor z = 0.25 under clutter: found; a request out of range is refused by name;
//                                  0 ok, 1 wrong result
//   plane_example PROBLEM RESULT   reads a problem file (n, d, ransac_n, num_iterations, probability, seed, the points)
//                                  and writes the result record: best_trial trials valid_trials n_inliers fitness rmse,
//                                  the plane, the inlier indices (%.17g)
// Exit code 77: no MI355X visible (loud failure, no CPU path); 1: any other failure.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "teaser/plane.h"

int main(int argc, char** argv) {
  try {
    if (argc == 3) {
      FILE* in = std::fopen(argv[1], "r");
      if (!in) return 2;
      int n = 0;
      teaser::PlaneOption o;
      bool ok = std::fscanf(in, "%d %lf %d %d %lf %" SCNu64, &n, &o.distance_threshold, &o.ransac_n, &o.num_iterations,
                            &o.probability, &o.seed) == 6;
      if (!ok || n < 0 || n > (1 << 22)) return 2;
      teaser::Matrix3X P(3, n);
      for (int i = 0; i < n; ++i)
        for (int r = 0; r < 3; ++r) ok = ok && std::fscanf(in, "%lf", &P(r, i)) == 1;
      std::fclose(in);
      if (!ok) return 2;
      teaser::PlaneSegmenter seg;
      const teaser::PlaneResult res = seg.segmentPlane(P, o);
      FILE* out = std::fopen(argv[2], "w");
      if (!out) return 2;
      std::fprintf(out, "%lld %lld %lld %zu %.17g %.17g\n", (long long)res.best_trial, (long long)res.trials,
                   (long long)res.valid_trials, res.inliers.size(), res.fitness, res.inlier_rmse);
      for (int k = 0; k < 4; ++k) std::fprintf(out, "%.17g ", res.plane_model[k]);
      std::fprintf(out, "\n");
      for (int i : res.inliers) std::fprintf(out, "%d\n", i);
      std::fclose(out);
      return 0;
    }
    // 400 points, the even ones on the floor z = 0.25, the odd ones anywhere
    const int n = 400;
    teaser::Matrix3X P(3, n);
    uint64_t state = 7;
    auto uni = [&]() {
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      return (double)(state >> 40) / 16777216.0 * 2.0 - 1.0;
    };
    for (int i = 0; i < n; ++i) {
      for (int r = 0; r < 3; ++r) P(r, i) = uni();
      if (i % 2 == 0) P(2, i) = 0.25;
    }
    const teaser::PlaneResult res = teaser::segmentPlane(P, 1e-6, 3, 1000, 0.99999999, /*seed=*/11);
    bool ok = res.inliers.size() >= 200 && res.best_trial >= 0 && res.trials < 1000 && res.valid_trials <= res.trials &&
              res.fitness >= 0.5 && res.mask.size() == (size_t)n;
    const double sign = res.plane_model[2] < 0 ? -1.0 : 1.0;
    const double want[4] = {0, 0, 1, -0.25};
    for (int k = 0; k < 4; ++k) ok = ok && std::fabs(sign * res.plane_model[k] - want[k]) < 1e-9;
    for (int i : res.inliers) ok = ok && res.mask[(size_t)i] == 1;
    bool refused = false;
    try {
      teaser::segmentPlane(P, 1e-6, 2);
    } catch (const teaser::PlaneError& e) {
      refused = e.status() == TEASER_HIP_ERR_BAD_ARG && std::string(e.what()).find("ransac_n") != std::string::npos;
    }
    std::printf("best trial %lld of %lld (%lld valid), %zu inliers, plane %.6g %.6g %.6g %.6g\n", (long long)res.best_trial,
                (long long)res.trials, (long long)res.valid_trials, res.inliers.size(), res.plane_model[0],
                res.plane_model[1], res.plane_model[2], res.plane_model[3]);
    return ok && refused ? 0 : 1;
  } catch (const teaser::PlaneError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return std::string(e.what()).find("status 3") != std::string::npos ? 77 : 1;
  }
}
