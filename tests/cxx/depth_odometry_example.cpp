// teaser::DepthOdometry (include/teaser/odometry.h).  No input file: three 48 x 36 depth frames given by formulas
// (tests/test_gpu_depth_odometry_cxx.py builds the same arrays) -- uint16 depth in padded rows --, the two consecutive
// pairs computed in one call and again one by one, then the first pair as float32 metres through computeDepthOdometry.
// The record printed -- the successes, counts, measures and FNV-1a hashes of the bytes of every matrix -- is what the test
// compares with the Python calls'.  trackFrameToModel is instantiated for both volume classes (compiled, not run: the
// Python test of track_frame_to_model runs the loop).
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cstdio>
#include <cstring>
#include <vector>

#include "teaser/odometry.h"

static int fail(const char* what) {
  std::fprintf(stderr, "depth_odometry_example: %s\n", what);
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

static void print(const char* name, int k, const teaser::DepthOdometryResult& r) {
  std::printf("%s %d success %d count %d iterations %d converged %d fitness %a rmse %a transformation %016llx information %016llx\n", name, k,
              (int)r.success, r.count, r.iterations, r.converged_levels, r.fitness, r.inlier_rmse, hash_rows(r.transformation, 4),
              hash_rows(r.information, 6));
}

// both instantiations must compile
template teaser::TrackingResult teaser::trackFrameToModel<teaser::UniformTSDFVolume>(teaser::UniformTSDFVolume&, teaser::DepthOdometry&,
                                                                                      const teaser::DepthFrame&, const teaser::PinholeCameraIntrinsic&,
                                                                                      const teaser::Matrix4&, const teaser::DepthOdometryOption&, double);
template teaser::TrackingResult teaser::trackFrameToModel<teaser::ScalableTSDFVolume>(teaser::ScalableTSDFVolume&, teaser::DepthOdometry&,
                                                                                       const teaser::DepthFrame&, const teaser::PinholeCameraIntrinsic&,
                                                                                       const teaser::Matrix4&, const teaser::DepthOdometryOption&, double);

int main() {
  try {
    const int w = 48, h = 36, padded = 52, n = 3;  // the depth rows lie 52 samples apart
    std::vector<std::vector<uint16_t>> depth(n, std::vector<uint16_t>((size_t)(padded * h), 9));
    for (int k = 0; k < n; ++k)
      for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j)
          depth[k][(size_t)(padded * i + j)] = (uint16_t)(1500 + 3 * i + 2 * (j + k) + ((i * i + (j + k) * (j + k)) % 97));
    const teaser::PinholeCameraIntrinsic K(w, h, 40.0, 40.0, 23.5, 17.5);
    std::vector<teaser::DepthFrame> frames;
    for (int k = 0; k < n; ++k) frames.push_back(teaser::DepthFrame::U16(depth[k].data(), w, h, 2 * padded));
    teaser::DepthOdometryOption option;
    option.iterations = {4, 3, 2};
    teaser::DepthOdometry odo;
    const std::vector<teaser::DepthFrame> src(frames.begin(), frames.end() - 1), tgt(frames.begin() + 1, frames.end());
    const std::vector<teaser::DepthOdometryResult> both = odo.computeBatch(src, tgt, {K}, {}, option);
    if (both.size() != 2) return fail("one result per pair");
    for (int k = 0; k < 2; ++k) {
      const teaser::DepthOdometryResult one = odo.compute(src[(size_t)k], tgt[(size_t)k], K, teaser::Matrix4::Identity(), option);
      if (one.success != both[(size_t)k].success || one.count != both[(size_t)k].count ||
          hash_rows(one.transformation, 4) != hash_rows(both[(size_t)k].transformation, 4) ||
          hash_rows(one.information, 6) != hash_rows(both[(size_t)k].information, 6))
        return fail("a pair alone differs from the pair in a batch");
      print("pair", k, both[(size_t)k]);
    }
    std::vector<float> m0((size_t)(w * h)), m1((size_t)(w * h));
    for (int i = 0; i < h; ++i)
      for (int j = 0; j < w; ++j) {
        m0[(size_t)(w * i + j)] = (float)depth[0][(size_t)(padded * i + j)] / 1000.0f;
        m1[(size_t)(w * i + j)] = (float)depth[1][(size_t)(padded * i + j)] / 1000.0f;
      }
    print("metres", 0, teaser::computeDepthOdometry(teaser::DepthFrame::F32(m0.data(), w, h), teaser::DepthFrame::F32(m1.data(), w, h), K,
                                                    teaser::Matrix4::Identity(), option));
    std::printf("checks 1\n");
    return 0;
  } catch (const teaser::ICPError& e) {
    std::fprintf(stderr, "depth_odometry_example: %s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  }
}
