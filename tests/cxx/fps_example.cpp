// teaser::farthestPointDownSample / teaser::FarthestPointSampler (include/teaser/fps.h) used like Open3D's
// farthest_point_down_sample, on a 5 x 5 x 1 integer grid (point i at (i % 5, i / 5, 0)) whose selection is worked out
// by hand: from start 12 (the centre) the four corners tie at d2 = 8 and the smallest index, 0, wins; the other three
// corners keep d = min(8, .) = 8 and follow in ascending index: 4, 20, 24.  The results are compared with literal
// expectations, the batched form with the single-cloud one, both routes with each other.
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "teaser/fps.h"

static int fail(const char* what) {
  std::fprintf(stderr, "fps_example: %s\n", what);
  return 1;
}

static teaser::Matrix3X grid() {
  teaser::Matrix3X P(3, 25);
  for (int i = 0; i < 25; ++i) P(0, i) = i % 5, P(1, i) = i / 5, P(2, i) = 0.0;
  return P;
}

int main() {
  try {
    const teaser::Matrix3X P = grid();
    const std::vector<int> want = {12, 0, 4, 20, 24};
    const std::vector<double> want_sel = {INFINITY, 8.0, 8.0, 8.0, 8.0};
    const teaser::Matrix3X S = teaser::farthestPointDownSample(P, 5, 12);
    if (S.cols() != 5) return fail("farthestPointDownSample returns num_samples points");
    for (int k = 0; k < 5; ++k)
      if (S(0, k) != want[k] % 5 || S(1, k) != want[k] / 5 || S(2, k) != 0.0) return fail("the points in order of selection");
    teaser::FarthestPointSampler fps;
    const teaser::FarthestPointResult one = fps.sample(P, 5, 12);
    if (one.indices != want || one.sel_dist != want_sel) return fail("indices and sel_dist");
    // after the centre and the four corners the farthest points are the edge mid-points at d2 = 4
    double worst = 0;
    for (double d : one.final_dist) worst = d > worst ? d : worst;
    if (one.final_dist.size() != 25 || worst != 4.0 || one.final_dist[12] != 0.0 || one.final_dist[2] != 4.0)
      return fail("final_dist");
    // K = n runs the loop: every point once, starting at start_index
    const teaser::FarthestPointResult all = fps.sample(P, 25, 3);
    std::vector<int> seen(25, 0);
    for (int i : all.indices) ++seen[(size_t)i];
    if (all.indices[0] != 3 || seen != std::vector<int>(25, 1)) return fail("K = n selects every point once");
    // the batched form: one handle, mixed records, an empty cloud and K = 0
    const teaser::Matrix3X empty(3, 0);
    std::vector<teaser::FarthestPointParams> rec(4);
    rec[0].num_samples = 5, rec[0].start_index = 12;
    rec[2].num_samples = 0, rec[2].start_index = 99;
    rec[3].num_samples = 25, rec[3].start_index = 3;
    const auto batch = fps.sampleBatch({P, empty, P, P}, rec);
    if (batch[0].indices != want || batch[0].sel_dist != want_sel || batch[0].final_dist != one.final_dist ||
        !batch[1].indices.empty() || !batch[2].indices.empty() || !batch[2].final_dist.empty() ||
        batch[3].indices != all.indices || batch[3].sel_dist != all.sel_dist)
      return fail("the batched form equals the single calls");
    // the other route gives the same bits
    const int64_t cap = fps.getOption("fps_resident_max");
    fps.setOption("fps_resident_max", 0);
    const teaser::FarthestPointResult streamed = fps.sample(P, 5, 12);
    fps.setOption("fps_resident_max", cap);
    if (cap < 25 || streamed.indices != one.indices || streamed.sel_dist != one.sel_dist ||
        streamed.final_dist != one.final_dist)
      return fail("both routes give the same result");
    bool threw = false;
    try {
      fps.sample(P, 26, 0);
    } catch (const teaser::ICPError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG && std::string(e.what()).find("num_samples") != std::string::npos;
    }
    if (!threw || fps.sample(P, 5, 12).indices != want) return fail("num_samples > n throws BAD_ARG, the handle lives");
    std::printf("samples %d of %d points\nchecks 1\n", (int)one.indices.size(), (int)P.cols());
    return 0;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
