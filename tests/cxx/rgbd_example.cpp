// teaser::createPointCloudFromRGBDImage / teaser::projectToRGBDImage / teaser::FrameConverter (include/teaser/rgbd.h) used
// like Open3D's calls.  No input file: a 40 x 30 uint16 depth frame and an RGB image given by formulas
// (tests/test_gpu_rgbd_cxx.py builds the same arrays), seen by a camera turned a quarter about its axis and shifted by
// dyadic amounts, so that the inverse of the extrinsic is exact whoever computes it.  The frame is unprojected, the cloud
// projected back into the same camera, and the record printed: counts and FNV-1a hashes of the bytes of every output,
// which the test compares with the Python calls'.
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cstdio>
#include <cstring>
#include <vector>

#include "teaser/rgbd.h"

static int fail(const char* what) {
  std::fprintf(stderr, "rgbd_example: %s\n", what);
  return 1;
}

static unsigned long long fnv(const void* p, size_t bytes) {
  unsigned long long h = 1469598103934665603ull;
  const unsigned char* b = (const unsigned char*)p;
  for (size_t k = 0; k < bytes; ++k) h = (h ^ b[k]) * 1099511628211ull;
  return h;
}

int main() {
  try {
    const int w = 40, h = 30, padded = 44;  // the depth rows lie 44 samples apart
    std::vector<uint16_t> depth((size_t)(padded * h), 9);
    std::vector<uint8_t> rgb((size_t)(3 * w * h));
    for (int i = 0; i < h; ++i)
      for (int j = 0; j < w; ++j) {
        depth[(size_t)(padded * i + j)] = (uint16_t)((i * 7 + j * 13) % 50 == 0 ? 0 : 500 + (i * 131 + j * 77) % 3000);
        uint8_t* px = &rgb[(size_t)(3 * (w * i + j))];
        px[0] = (uint8_t)((i * 3 + j) % 256), px[1] = (uint8_t)((i + j * 5) % 256), px[2] = (uint8_t)((i * j) % 256);
      }
    const teaser::PinholeCameraIntrinsic K(w, h, 32.0, 32.0, 19.5, 14.5);
    teaser::Matrix4 E = teaser::Matrix4::Identity();  // world to camera: a quarter turn about z and a shift
    E(0, 0) = 0.0, E(0, 1) = -1.0, E(1, 0) = 1.0, E(1, 1) = 0.0;
    E(0, 3) = 0.5, E(1, 3) = -0.25, E(2, 3) = 0.125;
    teaser::DepthFrame frame = teaser::DepthFrame::U16(depth.data(), w, h, 2 * padded);
    frame.withRGB8(rgb.data());

    const teaser::DepthCloud cloud = teaser::createPointCloudFromRGBDImage(frame, K, E, 1000.0, 3.0, true);
    const int64_t count = cloud.points.cols();
    if (count <= 0 || count >= w * h || cloud.colors.cols() != count) return fail("some pixels are valid, some are not");
    for (int64_t k = 0; k < count; ++k)
      if (cloud.colors(0, k) != cloud.colors(1, k) || cloud.colors(1, k) != cloud.colors(2, k)) return fail("intensity colours");
    const teaser::DepthImage image = teaser::projectToRGBDImage(cloud.points, cloud.colors, K, E, 1000.0, 3.0);
    if (image.depth.size() != (size_t)(w * h) || image.color.size() != (size_t)(3 * w * h)) return fail("image sizes");
    if (image.n_hit <= 0 || image.n_hit > count) return fail("n_hit");

    // the converter: the same frame twice around an empty one gives the same bits as the single call, with the pixels
    teaser::FrameConverter conv;
    teaser::UnprojectOptions o;
    o.extrinsic = E, o.depth_trunc = 3.0, o.convert_rgb_to_intensity = true, o.with_colors = true, o.with_pixels = true;
    teaser::UnprojectOptions plain = o;
    plain.with_colors = false;
    teaser::DepthFrame none = teaser::DepthFrame::U16(nullptr, 0, 5);
    const auto batch = conv.unprojectBatch({frame, none, frame}, {K, K, K}, {o, plain, o});
    if (batch[1].points.cols() != 0 || batch[0].points.cols() != count || batch[2].points.cols() != count)
      return fail("the batch's counts");
    const size_t bytes = sizeof(double) * 3 * (size_t)count;
    if (std::memcmp(batch[0].points.data(), cloud.points.data(), bytes) != 0 ||
        std::memcmp(batch[2].points.data(), cloud.points.data(), bytes) != 0 ||
        std::memcmp(batch[2].colors.data(), cloud.colors.data(), bytes) != 0)
      return fail("the batch equals the single call");
    for (int64_t k = 0; k < count; ++k) {
      const int32_t px = batch[0].pixels[(size_t)k];
      if (px < 0 || px >= w * h || depth[(size_t)(padded * (px / w) + px % w)] == 0) return fail("pixels of valid samples");
    }
    // depth alone: Open3D's default truncation lets every non-zero sample through
    const teaser::Matrix3X all = teaser::createPointCloudFromDepthImage(frame, K, E);
    int nonzero = 0;
    for (int i = 0; i < h; ++i)
      for (int j = 0; j < w; ++j) nonzero += depth[(size_t)(padded * i + j)] != 0;
    if (all.cols() != nonzero || nonzero <= count) return fail("createPointCloudFromDepthImage");
    // the round trip: with the identity pose, a depth scale of 1024 and this camera (fx and fy powers of two, cx and cy
    // with one binary place) nothing is rounded, and every valid pixel comes back to itself
    teaser::ProjectOptions po;
    po.with_index = true, po.depth_scale = 1024.0;
    teaser::UnprojectOptions id = o;
    id.extrinsic = teaser::Matrix4::Identity(), id.depth_scale = 1024.0;
    const teaser::DepthCloud at_origin = conv.unproject(frame, K, id);
    const int64_t kept = at_origin.points.cols();
    const teaser::DepthImage back = conv.project(at_origin.points, K, po);
    if (kept <= 0 || back.n_hit != kept) return fail("the round trip keeps every valid pixel");
    for (int64_t k = 0; k < kept; ++k) {
      const int32_t px = at_origin.pixels[(size_t)k];
      if (back.index[(size_t)px] != k || back.depth[(size_t)px] != (float)depth[(size_t)(padded * (px / w) + px % w)])
        return fail("the round trip is exact");
    }

    bool threw = false;
    try {
      teaser::UnprojectOptions bad = o;
      bad.depth_scale = 0.0;
      conv.unproject(frame, K, bad);
    } catch (const teaser::ICPError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG;
    }
    if (!threw) return fail("a depth_scale of 0 throws BAD_ARG");
    threw = false;
    try {
      conv.unproject(teaser::DepthFrame::U16(depth.data(), w, h, 2 * padded), K, o);  // colours of a frame without a colour image
    } catch (const teaser::ICPError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG;
    }
    if (!threw) return fail("colours of a frame without colour throw BAD_ARG");
    if (conv.unproject(frame, K, o).points.cols() != count) return fail("the converter works after a refusal");

    std::printf("count %lld\n", (long long)count);
    std::printf("points %016llx\ncolors %016llx\n", fnv(cloud.points.data(), bytes), fnv(cloud.colors.data(), bytes));
    std::printf("pixels %016llx\n", fnv(batch[0].pixels.data(), sizeof(int32_t) * (size_t)count));
    std::printf("n_hit %d\n", (int)image.n_hit);
    std::printf("depth %016llx\ncolor %016llx\n", fnv(image.depth.data(), sizeof(float) * image.depth.size()),
                fnv(image.color.data(), sizeof(float) * image.color.size()));
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
