// teaser::RGBDOdometry (include/teaser/odometry.h) used like Open3D's ComputeRGBDOdometry.  No input file: three 48 x 36
// frames given by formulas (tests/test_gpu_odometry_cxx.py builds the same arrays) -- uint16 depth in padded rows and a
// float32 intensity --, the two consecutive pairs computed in one call and again one by one.  The record printed -- the
// successes, counts and FNV-1a hashes of the bytes of every matrix -- is what the test compares with the Python calls'.
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cstdio>
#include <cstring>
#include <vector>

#include "teaser/odometry.h"

static int fail(const char* what) {
  std::fprintf(stderr, "odometry_example: %s\n", what);
  return 1;
}

static unsigned long long fnv(const void* p, size_t bytes) {
  unsigned long long h = 1469598103934665603ull;
  const unsigned char* b = (const unsigned char*)p;
  for (size_t k = 0; k < bytes; ++k) h = (h ^ b[k]) * 1099511628211ull;
  return h;
}

// row-major bytes of a matrix, as the Python arrays hold them
template <class M>
static unsigned long long hash_rows(const M& m, int n) {
  std::vector<double> v;
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) v.push_back(m(r, c));
  return fnv(v.data(), sizeof(double) * v.size());
}

int main() {
  try {
    const int w = 48, h = 36, padded = 52, n = 3;  // the depth rows lie 52 samples apart
    std::vector<std::vector<uint16_t>> depth(n, std::vector<uint16_t>((size_t)(padded * h), 9));
    std::vector<std::vector<float>> gray(n, std::vector<float>((size_t)(w * h)));
    for (int k = 0; k < n; ++k)
      for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) {
          depth[k][(size_t)(padded * i + j)] = (uint16_t)(1500 + 3 * i + 2 * (j + k) + ((i * (j + k)) % 5));
          gray[k][(size_t)(w * i + j)] = (float)((i * 3 + (j + k) * 5 + (i * (j + k)) % 7) % 32) / 32.0f;
        }
    const teaser::PinholeCameraIntrinsic K(w, h, 40.0, 40.0, 23.5, 17.5);
    std::vector<teaser::DepthFrame> frames;
    for (int k = 0; k < n; ++k) {
      frames.push_back(teaser::DepthFrame::U16(depth[k].data(), w, h, 2 * padded));
      frames.back().withIntensityF32(gray[k].data());
    }
    teaser::OdometryOption option;
    option.iteration_number_per_pyramid_level = {4, 3, 2};
    teaser::RGBDOdometry odo;
    const std::vector<teaser::DepthFrame> src(frames.begin(), frames.end() - 1), tgt(frames.begin() + 1, frames.end());
    const std::vector<teaser::RGBDOdometryResult> both = odo.computeBatch(src, tgt, {K}, {}, teaser::RGBDOdometryJacobian::HybridTerm, option);
    if (both.size() != 2) return fail("one result per pair");
    for (int k = 0; k < 2; ++k) {
      const teaser::RGBDOdometryResult one = odo.compute(src[(size_t)k], tgt[(size_t)k], K, teaser::Matrix4::Identity(),
                                                         teaser::RGBDOdometryJacobian::HybridTerm, option);
      if (one.success != both[(size_t)k].success || one.count != both[(size_t)k].count ||
          hash_rows(one.transformation, 4) != hash_rows(both[(size_t)k].transformation, 4) ||
          hash_rows(one.information, 6) != hash_rows(both[(size_t)k].information, 6))
        return fail("a pair alone gives the bits it gives in the batch");
    }
    const teaser::RGBDOdometryResult color = odo.compute(src[0], tgt[0], K, teaser::Matrix4::Identity(), teaser::RGBDOdometryJacobian::ColorTerm, option);
    bool threw = false;
    try {
      teaser::PinholeCameraIntrinsic bad = K;
      bad.fx = 0.0;
      odo.compute(src[0], tgt[0], bad);
    } catch (const teaser::ICPError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG && std::string(e.what()).find("fx and fy") != std::string::npos;
    }
    if (!threw) return fail("fx = 0 throws BAD_ARG");
    threw = false;
    try {
      teaser::OdometryOption deep = option;
      deep.iteration_number_per_pyramid_level = {1, 1, 1, 1, 1, 1, 1};  // 36 >> 6 = 0: a level without a pixel
      odo.compute(src[0], tgt[0], K, teaser::Matrix4::Identity(), teaser::RGBDOdometryJacobian::HybridTerm, deep);
    } catch (const teaser::ICPError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG && std::string(e.what()).find("every level needs a pixel") != std::string::npos;
    }
    if (!threw) return fail("a level without a pixel throws BAD_ARG");
    for (int k = 0; k < 2; ++k)
      std::printf("pair %d success %d count %d iterations %d transformation %016llx information %016llx\n", k, (int)both[(size_t)k].success,
                  both[(size_t)k].count, both[(size_t)k].iterations, hash_rows(both[(size_t)k].transformation, 4),
                  hash_rows(both[(size_t)k].information, 6));
    std::printf("color success %d count %d transformation %016llx information %016llx\n", (int)color.success, color.count,
                hash_rows(color.transformation, 4), hash_rows(color.information, 6));
    std::printf("checks 1\n");
    return 0;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
