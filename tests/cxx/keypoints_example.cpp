// teaser::computeISSKeypoints / teaser::ISSKeypoints (include/teaser/keypoints.h) used like Open3D's
// compute_iss_keypoints.  Without arguments: a 5 x 5 x 5 lattice (spacing 0.25); with salient radius 0.3, suppression
// radius 0.6 and both gammas at 2 its keypoints are the 27 inner points, which tie exactly and survive together; the
// result is compared with that literal list, the batched form with the single-cloud one.
//   keypoints_example DIR    reads DIR/cloud.bin (n x 3 doubles) and prints the keypoints, saliencies, counts and radii
//                            of the default parameters in hex, for tests/test_gpu_keypoints_cxx.py
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "teaser/keypoints.h"

static int fail(const char* what) {
  std::fprintf(stderr, "keypoints_example: %s\n", what);
  return 1;
}

static int from_file(const std::string& dir) {
  FILE* f = std::fopen((dir + "/cloud.bin").c_str(), "rb");
  if (!f) return fail("cannot open cloud.bin");
  std::vector<double> xyz;
  double p[3];
  while (std::fread(p, sizeof(double), 3, f) == 3) xyz.insert(xyz.end(), p, p + 3);
  std::fclose(f);
  teaser::Matrix3X P(3, (int64_t)(xyz.size() / 3));
  for (int64_t i = 0; i < P.cols(); ++i)
    for (int r = 0; r < 3; ++r) P(r, i) = xyz[(size_t)(3 * i + r)];
  teaser::ISSKeypoints iss;
  const teaser::ISSResult res = iss.compute(P);
  std::printf("indices");
  for (int i : res.indices) std::printf(" %d", i);
  std::printf("\nsaliency");
  for (double s : res.saliency) std::printf(" %a", s);
  std::printf("\ncounts");
  for (int32_t c : res.counts) std::printf(" %d", c);
  std::printf("\nradii %a %a %a\n", res.resolution, res.salient_radius, res.non_max_radius);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc == 2) return from_file(argv[1]);
    teaser::Matrix3X P(3, 125);
    std::vector<int> inner;
    for (int a = 0; a < 5; ++a)
      for (int b = 0; b < 5; ++b)
        for (int c = 0; c < 5; ++c) {
          const int i = 25 * a + 5 * b + c;
          P(0, i) = 0.25 * a, P(1, i) = 0.25 * b, P(2, i) = 0.25 * c;
          if (a >= 1 && a <= 3 && b >= 1 && b <= 3 && c >= 1 && c <= 3) inner.push_back(i);
        }
    teaser::ISSParams prm;
    prm.salient_radius = 0.3, prm.non_max_radius = 0.6, prm.gamma_21 = prm.gamma_32 = 2.0;
    if (teaser::computeISSKeypoints(P, prm) != inner) return fail("the keypoints are the 27 inner lattice points");
    teaser::ISSKeypoints iss;
    const teaser::ISSResult one = iss.compute(P, prm);
    if (one.indices != inner || one.counts[2 * 62] != 7 || one.counts[2 * 62 + 1] != 57 || one.counts[0] != 4 ||
        one.counts[1] != 17)
      return fail("neighbour counts of the centre and of a corner");
    if (one.saliency[62] != 0.125 / 7.0 || one.saliency[0] != 0.0 || !std::isnan(one.resolution) ||
        one.salient_radius != 0.3 || one.non_max_radius != 0.6)
      return fail("saliency of the centre (2 (1/4)^2 / 7), of a corner (below min_neighbors), and the radii");
    // automatic radii: the resolution of the lattice is its spacing, and both radii are replaced
    teaser::ISSParams half = prm;
    half.non_max_radius = 0.0;
    const teaser::ISSResult aut = iss.compute(P, half);
    if (aut.resolution != 0.25 || aut.salient_radius != 1.5 || aut.non_max_radius != 1.0)
      return fail("automatic radii replace both");
    // the batched form: one handle, mixed parameters, an empty cloud in the middle
    const teaser::Matrix3X empty(3, 0);
    const auto batch = iss.computeBatch({P, empty, P}, {prm, teaser::ISSParams(), half});
    if (batch[0].indices != inner || batch[0].saliency != one.saliency || !batch[1].indices.empty() ||
        batch[2].indices != aut.indices || batch[2].saliency != aut.saliency)
      return fail("the batched form equals the single calls");
    if (teaser::computeISSKeypointsBatch({P, empty}, {prm, prm})[0] != inner) return fail("computeISSKeypointsBatch");
    bool threw = false;
    try {
      teaser::ISSParams bad = prm;
      bad.salient_radius = -1.0;
      iss.compute(P, bad);
    } catch (const teaser::ICPError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG && std::string(e.what()).find("salient_radius") != std::string::npos;
    }
    if (!threw || iss.compute(P, prm).indices != inner) return fail("a negative radius throws BAD_ARG, the handle lives");
    std::printf("keypoints %zu of %d\nchecks 1\n", one.indices.size(), (int)P.cols());
    return 0;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
