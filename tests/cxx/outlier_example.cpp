// teaser::removeStatisticalOutliers / removeRadiusOutliers / selfKnn (include/teaser/outlier.h) used like Open3D's
// pcd.remove_statistical_outlier / pcd.remove_radius_outlier.  No input file: a 5 x 5 x 5 lattice (spacing 0.25) with
// three far points planted at indices 10, 60 and 127; the kept index sets are compared with literal lists, the batched
// forms with the single-cloud ones.
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cstdio>
#include <vector>

#include "teaser/outlier.h"

static teaser::Matrix3X cloud(const std::vector<double>& xyz) {
  teaser::Matrix3X m(3, (int64_t)(xyz.size() / 3));
  for (int64_t i = 0; i < m.cols(); ++i)
    for (int r = 0; r < 3; ++r) m(r, i) = xyz[(size_t)(3 * i + r)];
  return m;
}

static int fail(const char* what) {
  std::fprintf(stderr, "outlier_example: %s\n", what);
  return 1;
}

int main() {
  try {
    std::vector<double> xyz;
    const double planted[3][3] = {{5.0, 5.0, 5.0}, {-4.0, 6.0, 0.0}, {9.0, -3.0, 2.0}};
    int next = 0;
    for (int a = 0; a < 5; ++a)
      for (int b = 0; b < 5; ++b)
        for (int c = 0; c < 5; ++c) {
          if (xyz.size() / 3 == 10 || xyz.size() / 3 == 60) {
            xyz.insert(xyz.end(), planted[next], planted[next] + 3);
            ++next;
          }
          const double p[3] = {0.25 * a, 0.25 * b, 0.25 * c};
          xyz.insert(xyz.end(), p, p + 3);
        }
    xyz.insert(xyz.end(), planted[2], planted[2] + 3);  // index 127
    const teaser::Matrix3X P = cloud(xyz);
    if (P.cols() != 128) return fail("the scene has 128 points");
    std::vector<int> lattice;  // the literal list: everything but 10, 60, 127
    for (int i = 0; i < 128; ++i)
      if (i != 10 && i != 60 && i != 127) lattice.push_back(i);

    const teaser::StatisticalOutlierResult s = teaser::removeStatisticalOutliers(P, 8, 1.0);
    if (s.indices != lattice) return fail("statistical removal keeps exactly the lattice");
    if (s.avg.size() != 128 || !(s.avg[10] > s.threshold) || !(s.avg[0] < s.threshold) || !(s.std_dev > 0))
      return fail("statistical removal's per-point values");
    const teaser::RadiusOutlierResult r = teaser::removeRadiusOutliers(P, 3, 0.3);
    if (r.indices != lattice) return fail("radius removal keeps exactly the lattice");
    if (r.counts[0] != 4 || r.counts[10] != 1) return fail("radius removal's counts");
    // at exactly the lattice spacing nothing but the point itself is closer than the radius
    if (!teaser::removeRadiusOutliers(P, 1, 0.25).indices.empty()) return fail("d2 < r r is strict");
    const teaser::SelfKnnResult k = teaser::selfKnn(P, 5);
    const int32_t first[5] = {0, 1, 5, 26, 6};
    for (int t = 0; t < 5; ++t)
      if (k.indices[(size_t)t] != first[t]) return fail("self k-NN: ties go to the smaller index");
    if (k.distances2[0] != 0.0 || k.distances2[1] != 0.0625 || k.distances2[4] != 0.125) return fail("self k-NN: d2");
    if (k.indices[5 * 10] != 10 || k.indices[5 * 10 + 1] != 126) return fail("self k-NN of a far point");

    // the batched forms: one handle, mixed parameters, an empty cloud in the middle
    teaser::OutlierRemoval o;
    const teaser::Matrix3X empty = cloud({});
    const auto sb = o.removeStatisticalOutliersBatch({P, empty, P}, {8, 5, 20}, {1.0, 2.0, 1.0});
    if (sb[0].indices != lattice || !sb[1].indices.empty() || sb[0].avg != s.avg || sb[0].threshold != s.threshold)
      return fail("batched statistical removal equals the single call");
    const auto rb = o.removeRadiusOutliersBatch({P, empty, P}, {3, 1, 1}, {0.3, 0.1, 0.25});
    if (rb[0].indices != lattice || rb[0].counts != r.counts || !rb[2].indices.empty())
      return fail("batched radius removal equals the single call");
    const auto kb = o.selfKnnBatch({empty, P}, {3, 5});
    if (!kb[0].indices.empty() || kb[1].indices != k.indices || kb[1].distances2 != k.distances2)
      return fail("batched self k-NN equals the single call");
    o.setOption("knn_ring_cap", 0);
    if (o.selfKnn(P, 5).indices != k.indices || o.getOption("knn_fallbacks") != 128)
      return fail("the whole-cloud route gives the same neighbours");
    bool threw = false;
    try {
      o.removeStatisticalOutliers(P, 0, 1.0);
    } catch (const teaser::ICPError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG;
    }
    if (!threw) return fail("nb_neighbors = 0 throws BAD_ARG");
    std::printf("kept %zu of %d  mean %.6g  std %.6g  threshold %.6g\nchecks 1\n", s.indices.size(), (int)P.cols(),
                s.mean, s.std_dev, s.threshold);
    return 0;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
