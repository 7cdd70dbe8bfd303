// teaser::clusterDBSCAN / teaser::DBSCAN (include/teaser/cluster.h) used like Open3D's cluster_dbscan, on the
// contested-border scene of tests/dbscan_reference.py: two rows of 10 points (spacing 0.5) whose ends lie 3 apart, and
// one point half-way between the ends.  With eps = 1.75 and min_points = 4 every row point is core, the point between
// them sees itself and the two ends (3 neighbours: not core) and borders BOTH clusters; it takes the smaller label.
// The results are compared with literal expectations, the batched form with the single-cloud one.
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cstdio>
#include <string>
#include <vector>

#include "teaser/cluster.h"

static int fail(const char* what) {
  std::fprintf(stderr, "dbscan_example: %s\n", what);
  return 1;
}

// b_first: indices [B0..B9, A0..A9, c], else [c, A0..A9, B0..B9]
static teaser::Matrix3X scene(bool b_first) {
  teaser::Matrix3X P(3, 21);
  for (int i = 0; i < 21; ++i) P(0, i) = P(1, i) = P(2, i) = 0.0;
  const int a0 = b_first ? 10 : 1, b0 = b_first ? 0 : 11, c = b_first ? 20 : 0;
  for (int k = 0; k < 10; ++k) {
    P(0, a0 + k) = -0.5 * k;
    P(0, b0 + k) = 3.0 + 0.5 * k;
  }
  P(0, c) = 1.5;
  return P;
}

int main() {
  try {
    const std::vector<int32_t> row = {5, 5, 6, 7, 7, 7, 7, 6, 5, 4};
    std::vector<int> want_c(21, 0), want_b(21, 0);
    std::vector<int32_t> roots_c(21, 1), roots_b(21, 0), counts_c(21, 3), counts_b(21, 3);
    for (int k = 0; k < 10; ++k) {
      want_c[11 + k] = 1, want_b[10 + k] = 1;
      roots_c[11 + k] = 11, roots_b[10 + k] = 10;
      counts_c[1 + k] = counts_c[11 + k] = counts_b[k] = counts_b[10 + k] = row[k];
    }
    roots_c[0] = -1, roots_b[20] = -1;
    const teaser::Matrix3X Pc = scene(false), Pb = scene(true);
    if (teaser::clusterDBSCAN(Pc, 1.75, 4) != want_c) return fail("the contested point takes the smaller label (c first)");
    if (teaser::clusterDBSCAN(Pb, 1.75, 4) != want_b) return fail("the contested point takes the smaller label (B first)");
    teaser::DBSCAN db;
    teaser::DBSCANParams prm;
    prm.eps = 1.75, prm.min_points = 4;
    const teaser::DBSCANResult one = db.cluster(Pc, prm);
    if (one.labels != want_c || one.n_clusters != 2 || one.counts != counts_c || one.roots != roots_c)
      return fail("labels, cluster count, neighbour counts and roots (c first)");
    const teaser::DBSCANResult two = db.cluster(Pb, prm);
    if (two.labels != want_b || two.n_clusters != 2 || two.counts != counts_b || two.roots != roots_b)
      return fail("labels, cluster count, neighbour counts and roots (B first)");
    // min_points 3 makes the contested point core: it joins both rows into one cluster
    teaser::DBSCANParams join = prm;
    join.min_points = 3;
    const teaser::DBSCANResult joined = db.cluster(Pc, join);
    if (joined.n_clusters != 1 || joined.labels != std::vector<int>(21, 0) || joined.roots != std::vector<int32_t>(21, 0))
      return fail("a core point between the rows joins them");
    // the batched form: one handle, mixed parameters, an empty cloud in the middle, a cloud without radius
    const teaser::Matrix3X empty(3, 0);
    teaser::DBSCANParams zero = prm;
    zero.eps = 0.0;
    const auto batch = db.clusterBatch({Pc, empty, Pb, Pc, Pb}, {prm, prm, prm, join, zero});
    if (batch[0].labels != want_c || batch[0].roots != roots_c || !batch[1].labels.empty() || batch[1].n_clusters != 0 ||
        batch[2].labels != want_b || batch[2].counts != counts_b || batch[3].labels != joined.labels ||
        batch[3].n_clusters != 1 || batch[4].n_clusters != 0 || batch[4].labels != std::vector<int>(21, -1) ||
        batch[4].counts != std::vector<int32_t>(21, 0))
      return fail("the batched form equals the single calls");
    if (teaser::clusterDBSCANBatch({Pb, empty}, {prm, prm})[0] != want_b) return fail("clusterDBSCANBatch");
    bool threw = false;
    try {
      teaser::DBSCANParams bad = prm;
      bad.min_points = 0;
      db.cluster(Pc, bad);
    } catch (const teaser::ICPError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG && std::string(e.what()).find("min_points") != std::string::npos;
    }
    if (!threw || db.cluster(Pc, prm).labels != want_c) return fail("min_points 0 throws BAD_ARG, the handle lives");
    std::printf("clusters %d of %d points\nchecks 1\n", one.n_clusters, (int)Pc.cols());
    return 0;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
