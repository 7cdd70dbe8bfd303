// teaser::NearestNeighborSearch (include/teaser/search.h) used like Open3D's KDTreeFlann / NearestNeighborSearch, and
// teaser::computePointCloudDistance / computeNearestNeighborDistance.  No input file: the data cloud is a 5 x 5 x 5
// lattice (spacing 0.25, point (a, b, c) at index 25 a + 5 b + c); the queries are lattice points, cell centres and a
// far point, so every squared distance is exact and the results are compared with literal lists.
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cmath>
#include <cstdio>
#include <vector>

#include "teaser/search.h"

static teaser::Matrix3X cloud(const std::vector<double>& xyz) {
  teaser::Matrix3X m(3, (int64_t)(xyz.size() / 3));
  for (int64_t i = 0; i < m.cols(); ++i)
    for (int r = 0; r < 3; ++r) m(r, i) = xyz[(size_t)(3 * i + r)];
  return m;
}

static int fail(const char* what) {
  std::fprintf(stderr, "search_example: %s\n", what);
  return 1;
}

int main() {
  try {
    std::vector<double> xyz;
    for (int a = 0; a < 5; ++a)
      for (int b = 0; b < 5; ++b)
        for (int c = 0; c < 5; ++c) {
          const double p[3] = {0.25 * a, 0.25 * b, 0.25 * c};
          xyz.insert(xyz.end(), p, p + 3);
        }
    const teaser::Matrix3X P = cloud(xyz);
    // queries: the lattice point 31 = (1, 1, 1), the centre of the first cell, and a point far outside the box
    const teaser::Matrix3X Q = cloud({0.25, 0.25, 0.25, 0.125, 0.125, 0.125, 100.0, 0.0, 0.0});
    teaser::NearestNeighborSearch nns(P);

    const teaser::KnnSearchResult k = nns.knnSearch(Q, 8);
    const int32_t at_point[8] = {31, 6, 26, 30, 32, 36, 56, 1}, at_centre[8] = {0, 1, 5, 6, 25, 26, 30, 31};
    for (int t = 0; t < 8; ++t)
      if (k.indices[(size_t)t] != at_point[t] || k.indices[8 + (size_t)t] != at_centre[t])
        return fail("k-NN: ascending (d2, index), ties to the smaller index");
    if (k.distances2[0] != 0.0 || k.distances2[1] != 0.0625 || k.distances2[7] != 0.125 || k.distances2[8] != 0.046875)
      return fail("k-NN: squared distances");
    if (k.indices[16] != 100 || k.distances2[16] != 99.0 * 99.0) return fail("k-NN of the far query");
    if (nns.getOption("knn_fallbacks") < 1) return fail("the far query is served by the scan of the whole cloud");

    const teaser::RadiusSearchResult r = nns.radiusSearch(Q, 0.25 * 1.0001);
    const std::vector<int64_t> splits = {0, 7, 15, 15};
    const std::vector<int32_t> rows = {31, 6, 26, 30, 32, 36, 56, 0, 1, 5, 6, 25, 26, 30, 31};
    if (r.row_splits != splits || r.indices != rows) return fail("radius search: rows and row splits");
    if (r.distances2.size() != 15 || r.distances2[6] != 0.0625 || r.distances2[14] != 0.046875)
      return fail("radius search: squared distances");
    // at exactly the lattice spacing only the point itself is closer than the radius
    if (nns.radiusSearch(Q, 0.25).row_splits != std::vector<int64_t>{0, 1, 9, 9}) return fail("d2 < r r is strict");

    const teaser::KnnSearchResult h = nns.hybridSearch(Q, 0.25 * 1.0001, 4);
    const std::vector<int32_t> counts = {4, 4, 0}, hrows = {31, 6, 26, 30, 0, 1, 5, 6, -1, -1, -1, -1};
    if (h.counts != counts || h.indices != hrows || !std::isinf(h.distances2[8]))
      return fail("hybrid search: the first max_nn of the radius row");

    // the batch forms: two data clouds, mixed parameters, an empty query set
    const teaser::Matrix3X none = cloud({});
    teaser::NearestNeighborSearch two(std::vector<teaser::Matrix3X>{P, P});
    const auto kb = two.knnSearchBatch({none, Q}, {3, 8});
    if (!kb[0].indices.empty() || kb[1].indices != k.indices || kb[1].distances2 != k.distances2)
      return fail("batched k-NN equals the single call");
    const auto rb = two.radiusSearchBatch({Q, none}, {0.25 * 1.0001, 1.0});
    if (rb[0].indices != r.indices || rb[0].row_splits != r.row_splits || rb[1].row_splits != std::vector<int64_t>{0})
      return fail("batched radius search equals the single call");
    const auto hb = two.hybridSearchBatch({Q, Q}, {0.25 * 1.0001, 0.25}, {4, 100});
    if (hb[0].indices != h.indices || hb[1].counts != std::vector<int32_t>{1, 8, 0})
      return fail("batched hybrid search equals the single call");
    two.setOption("knn_ring_cap", 0);
    if (two.knnSearchBatch({Q, Q}, {8, 8})[1].indices != k.indices || two.getOption("knn_fallbacks") != 6)
      return fail("the whole-cloud route gives the same neighbours");

    const std::vector<double> d = teaser::computePointCloudDistance(Q, P);
    if (d.size() != 3 || d[0] != 0.0 || d[1] != std::sqrt(0.046875) || d[2] != 99.0)
      return fail("computePointCloudDistance");
    const std::vector<double> nn = teaser::computeNearestNeighborDistance(P);
    for (double v : nn)
      if (v != 0.25) return fail("computeNearestNeighborDistance on the lattice");
    if (nn.size() != 125 || teaser::computeNearestNeighborDistance(cloud({1.0, 2.0, 3.0})) != std::vector<double>{0.0})
      return fail("computeNearestNeighborDistance: zeros below two points");
    bool threw = false;
    try {
      nns.knnSearch(Q, 101);
    } catch (const teaser::ICPError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG;
    }
    if (!threw) return fail("k = 101 throws BAD_ARG");
    std::printf("queries %d  radius entries %zu  far distance %.6g\nchecks 1\n", (int)Q.cols(), r.indices.size(), d[2]);
    return 0;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
