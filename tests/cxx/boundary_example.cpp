// teaser::computeBoundaryPoints / teaser::BoundaryDetector (include/teaser/boundary.h) used like Open3D's
// ComputeBoundaryPoints.  No input file: a 9 x 9 planar lattice (spacing 0.125, normals +z, radius 1.5 spacings,
// threshold 90 degrees), whose boundary points are exactly its 32 perimeter points: interior gaps are 45 degrees, edge
// gaps 180, corner gaps 270.
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cmath>
#include <cstdio>
#include <vector>

#include "teaser/boundary.h"

static int fail(const char* what) {
  std::fprintf(stderr, "boundary_example: %s\n", what);
  return 1;
}

int main() {
  try {
    const int side = 9;
    teaser::Matrix3X P(3, side * side), N(3, side * side);
    for (int a = 0; a < side; ++a)
      for (int b = 0; b < side; ++b) {
        const int i = side * a + b;
        P(0, i) = 0.125 * a, P(1, i) = 0.125 * b, P(2, i) = 0.0;
        N(0, i) = 0.0, N(1, i) = 0.0, N(2, i) = 1.0;
      }
    const teaser::BoundaryParams params(1.5 * 0.125, 30, 90.0);
    const teaser::BoundaryResult one = teaser::computeBoundaryPoints(P, N, params);
    if (one.mask.size() != (size_t)(side * side) || one.n_boundary != 32) return fail("the lattice has 32 boundary points");
    for (int a = 0; a < side; ++a)
      for (int b = 0; b < side; ++b) {
        const bool rim = a == 0 || b == 0 || a == side - 1 || b == side - 1;
        if ((one.mask[(size_t)(side * a + b)] != 0) != rim) return fail("the mask is the perimeter");
      }
    if (one.indices().size() != 32 || one.indices().front() != 0) return fail("indices() lists the ones");

    // the batch: the same cloud twice around an empty one, k-NN beside hybrid, the gaps and the counts asked for; a
    // small list bound changes nothing
    teaser::BoundaryDetector d;
    const double pi = 3.14159265358979323846;
    const auto batch = d.computeBatch({P, teaser::Matrix3X(3, 0), P}, {N, teaser::Matrix3X(3, 0), N},
                                      {params, params, teaser::BoundaryParams(teaser::NormalSearch::KNN(9), 90.0)}, {},
                                      true, true);
    if (batch[0].mask != one.mask || batch[0].n_boundary != 32 || !batch[1].mask.empty() || batch[1].n_boundary != 0)
      return fail("the batch equals the single call");
    for (size_t i = 0; i < batch[0].mask.size(); ++i) {
      const int m = batch[0].counts[i];
      const double want = m == 9 ? pi / 4 : (m == 6 ? pi : 3 * pi / 2);
      if ((m != 9 && m != 6 && m != 4) || std::fabs(batch[0].max_gap[i] - want) > 1e-12) return fail("gaps of 45, 180, 270");
    }
    const int64_t bound = d.getOption("fpfh_list_bytes");
    d.setOption("fpfh_list_bytes", 1);
    const auto pieces = d.computeBatch({P, P}, {N, N}, {params, teaser::BoundaryParams(teaser::NormalSearch::KNN(9), 90.0)},
                                       {}, true, true);
    d.setOption("fpfh_list_bytes", bound);
    if (pieces[0].mask != one.mask || pieces[0].max_gap != batch[0].max_gap || pieces[1].mask != batch[2].mask ||
        pieces[1].max_gap != batch[2].max_gap)
      return fail("fpfh_list_bytes changes no bit");

    // normals inside the call equal estimateNormals followed by the call
    const teaser::NormalSearch ns = teaser::NormalSearch::Hybrid(0.3, 30);
    const auto est = d.computeBatch({P}, {teaser::Matrix3X(3, 0)}, {params}, {ns}, true, false, true);
    const teaser::Normals nr = teaser::estimateNormals(P, ns);
    const teaser::BoundaryResult two = d.compute(P, nr.normals, params, true);
    if (est[0].mask != two.mask || est[0].max_gap != two.max_gap) return fail("normals inside the call");
    if (est[0].mask != one.mask) return fail("estimated normals of a plane give the perimeter");

    bool threw = false;
    try {
      d.compute(P, N, teaser::BoundaryParams(0.2, 30, 361.0));
    } catch (const teaser::ICPError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG;
    }
    if (!threw) return fail("a threshold above 360 throws BAD_ARG");
    threw = false;
    try {
      teaser::NormalSearch radius_only = teaser::NormalSearch::Hybrid(0.3, 20);
      radius_only.rec.search = 2;
      d.compute(P, N, teaser::BoundaryParams(radius_only, 90.0));
    } catch (const teaser::ICPError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG;
    }
    if (!threw) return fail("radius-only search throws BAD_ARG");
    if (d.compute(P, N, params).mask != one.mask) return fail("the detector works after a refusal");
    std::printf("lattice points %d  boundary points %d\nchecks 1\n", side * side, (int)one.n_boundary);
    return 0;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
