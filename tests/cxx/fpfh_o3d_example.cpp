// teaser::computeFPFHFeature / teaser::FPFHOpen3D (include/teaser/fpfh_open3d.h) used like Open3D's compute_fpfh_feature.
// No input file: two points with perpendicular normals, a cloud of coincident points and a 4 x 4 x 4 lattice (spacing
// 0.25) with normals along the axes, whose rows are known in closed form or by the sums of their groups.
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cmath>
#include <cstdio>
#include <vector>

#include "teaser/fpfh_open3d.h"

static teaser::Matrix3X cloud(const std::vector<double>& xyz) {
  teaser::Matrix3X m(3, (int64_t)(xyz.size() / 3));
  for (int64_t i = 0; i < m.cols(); ++i)
    for (int r = 0; r < 3; ++r) m(r, i) = xyz[(size_t)(3 * i + r)];
  return m;
}

static int fail(const char* what) {
  std::fprintf(stderr, "fpfh_o3d_example: %s\n", what);
  return 1;
}

int main() {
  try {
    using teaser::NormalSearch;
    // two points, normals z and x: both pairs are degenerate (dp parallel to the first normal after the swap rule), so
    // every feature is 0: bins 5, 16 and 27 hold c = 100; FPFH = 100 SPFH[other] / 100 + SPFH[own]
    const teaser::FPFHOpen3DFeature two =
        teaser::computeFPFHFeature(cloud({0, 0, 0, 1, 0, 0}), cloud({0, 0, 1, 1, 0, 0}), NormalSearch::KNN(2));
    if (two.n != 2 || two.data.size() != 66) return fail("two points: n x 33 rows");
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 33; ++j)
        if (two.row(i)[j] != ((j == 5 || j == 16 || j == 27) ? 200.0 : 0.0)) return fail("two points: bins 5, 16, 27");

    // coincident points: every d2 == 0 is skipped, FPFH equals SPFH = 100 in bins 5, 16, 27
    teaser::FPFHOpen3D f;
    std::vector<double> same;
    for (int i = 0; i < 9; ++i) same.insert(same.end(), {0.3, -1.25, 7.0});
    std::vector<double> up;
    for (int i = 0; i < 9; ++i) up.insert(up.end(), {0.0, 0.0, 1.0});
    const auto co = f.computeBatch({cloud(same)}, {cloud(up)}, {NormalSearch::Hybrid(0.5, 5)}, {}, true, true);
    for (int i = 0; i < 9; ++i)
      for (int j = 0; j < 33; ++j) {
        const double want = (j == 5 || j == 16 || j == 27) ? 100.0 : 0.0;
        if (co[0].row(i)[j] != want || co[0].spfh[(size_t)(33 * i + j)] != want) return fail("coincident points");
      }
    if (co[0].normals.cols() != 9 || co[0].normals(2, 4) != 1.0) return fail("normals_out returns the given normals");

    // the lattice: every group of an SPFH row sums to 100 and of an FPFH row to 200 up to rounding; an isolating radius
    // gives zero rows; the batch equals the single calls; a small list bound changes no bit
    std::vector<double> xyz, nrm;
    const double axes[6][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {-1, 0, 0}, {0, -1, 0}, {0, 0, -1}};
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b)
        for (int c = 0; c < 4; ++c) {
          const double p[3] = {0.25 * a, 0.25 * b, 0.25 * c};
          xyz.insert(xyz.end(), p, p + 3);
          const double* ax = axes[(16 * a + 4 * b + c) % 6];
          nrm.insert(nrm.end(), ax, ax + 3);
        }
    const teaser::Matrix3X P = cloud(xyz), N = cloud(nrm);
    const teaser::FPFHOpen3DFeature lat = f.compute(P, N, NormalSearch::Hybrid(0.3, 20));
    for (int64_t i = 0; i < lat.n; ++i)
      for (int g = 0; g < 3; ++g) {
        double s = 0;
        for (int j = 0; j < 11; ++j) s += lat.row(i)[11 * g + j];
        if (std::fabs(s - 200.0) > 1e-9) return fail("lattice: a group of an FPFH row sums to 200");
      }
    const teaser::FPFHOpen3DFeature alone = f.compute(P, N, NormalSearch::Hybrid(0.2, 20));
    for (double v : alone.data)
      if (v != 0.0) return fail("a radius that isolates every point gives zero rows");
    const auto batch = f.computeBatch({P, cloud({}), P}, {N, cloud({}), N},
                                      {NormalSearch::KNN(27), NormalSearch::KNN(5), NormalSearch::Hybrid(0.3, 20)});
    if (batch[2].data != lat.data || batch[1].n != 0 || !batch[1].data.empty()) return fail("the batch equals the single call");
    const int64_t bound = f.getOption("fpfh_list_bytes");
    f.setOption("fpfh_list_bytes", 1);
    const auto pieces = f.computeBatch({P, P}, {N, N}, {NormalSearch::KNN(27), NormalSearch::Hybrid(0.3, 20)});
    f.setOption("fpfh_list_bytes", bound);
    if (pieces[0].data != batch[0].data || pieces[1].data != lat.data) return fail("fpfh_list_bytes changes no bit");

    // normals inside the call: extractFPFH equals estimateNormals followed by compute
    const teaser::FPFHOpen3DFeature ex = f.extractFPFH(P, 0.125, true);
    const teaser::Normals nr = teaser::estimateNormals(P, NormalSearch::Hybrid(0.25, 30));
    const teaser::FPFHOpen3DFeature ex2 = f.compute(P, nr.normals, NormalSearch::Hybrid(0.625, 100));
    if (ex.data != ex2.data) return fail("extractFPFH equals estimateNormals + compute");
    for (int64_t i = 0; i < P.cols(); ++i)
      for (int r = 0; r < 3; ++r)
        if (ex.normals(r, i) != nr.normals(r, i)) return fail("extractFPFH returns the estimated normals");

    bool threw = false;
    try {
      NormalSearch radius_only = NormalSearch::Hybrid(0.3, 20);
      radius_only.rec.search = 2;
      f.compute(P, N, radius_only);
    } catch (const teaser::ICPError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG;
    }
    if (!threw) return fail("radius-only search throws BAD_ARG");
    threw = false;
    try {
      f.compute(P, N, NormalSearch::KNN(5).along(0, 0, 1));
    } catch (const teaser::ICPError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG;
    }
    if (!threw) return fail("an oriented search throws BAD_ARG");
    std::printf("lattice points %d  row 0 bin 5 %.6g\nchecks 1\n", (int)lat.n, lat.row(0)[5]);
    return 0;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
