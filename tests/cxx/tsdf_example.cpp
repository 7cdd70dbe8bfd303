// teaser::UniformTSDFVolume (include/teaser/tsdf.h) used like Open3D's class.  No input file: two 40 x 30 uint16 depth
// frames and RGB images given by formulas (tests/test_gpu_tsdf_cxx.py builds the same arrays), seen by cameras shifted by
// dyadic amounts, integrated in one call into a 16^3 RGB8 volume of side 1 in front of the camera.  The record printed --
// counts and FNV-1a hashes of the bytes of every output -- is what the test compares with the Python calls'.
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cstdio>
#include <cstring>
#include <vector>

#include "teaser/tsdf.h"

static int fail(const char* what) {
  std::fprintf(stderr, "tsdf_example: %s\n", what);
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
    std::vector<std::vector<uint16_t>> depth(2, std::vector<uint16_t>((size_t)(padded * h), 9));
    std::vector<std::vector<uint8_t>> rgb(2, std::vector<uint8_t>((size_t)(3 * w * h)));
    for (int k = 0; k < 2; ++k)
      for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) {
          depth[k][(size_t)(padded * i + j)] = (uint16_t)((i * 7 + j * 13) % 50 == 0 ? 0 : 900 + 4 * i + 3 * j + 20 * k + (i * j) % 7);
          uint8_t* px = &rgb[k][(size_t)(3 * (w * i + j))];
          px[0] = (uint8_t)((i * 3 + j + 40 * k) % 256), px[1] = (uint8_t)((i + j * 5) % 256), px[2] = (uint8_t)((i * j + k) % 256);
        }
    const teaser::PinholeCameraIntrinsic K(w, h, 32.0, 32.0, 19.5, 14.5);
    std::vector<teaser::Matrix4> E(2, teaser::Matrix4::Identity());  // world to camera
    E[1](0, 3) = 0.0625, E[1](1, 3) = -0.03125, E[1](2, 3) = 0.015625;
    std::vector<teaser::DepthFrame> frames;
    for (int k = 0; k < 2; ++k) {
      frames.push_back(teaser::DepthFrame::U16(depth[k].data(), w, h, 2 * padded));
      frames.back().withRGB8(rgb[k].data());
    }

    teaser::UniformTSDFVolume vol(1.0, 16, 0.15, teaser::TSDFVolumeColorType::RGB8, -0.5, -0.5, 0.5);
    if (vol.resolution() != 16 || vol.voxelLength() != 0.0625) return fail("the volume's shape");
    if (vol.extractPointCloud().points.cols() != 0) return fail("a fresh volume is empty");
    vol.integrateBatch(frames, {K}, E);
    const teaser::TSDFPointCloud cloud = vol.extractPointCloud();
    const int64_t count = cloud.points.cols();
    if (count <= 0 || cloud.normals.cols() != count || cloud.colors.cols() != count) return fail("the surface has rows");
    const teaser::TSDFPointCloud voxels = vol.extractVoxelPointCloud();
    if (voxels.points.cols() <= count / 3 || voxels.normals.cols() != 0) return fail("the voxel cloud");
    const std::vector<float> tw = vol.extractVolumeTSDF();
    const std::vector<double> col = vol.extractVolumeColor();
    if (tw.size() != 2 * 4096 || col.size() != 3 * 4096) return fail("the volume's arrays");

    // a second volume, alive beside the first, fed one frame per call: the same bits
    teaser::UniformTSDFVolume one(1.0, 16, 0.15, teaser::TSDFVolumeColorType::RGB8, -0.5, -0.5, 0.5);
    for (int k = 0; k < 2; ++k) one.integrate(frames[(size_t)k], K, E[(size_t)k]);
    if (one.extractVolumeTSDF() != tw || one.extractVolumeColor() != col) return fail("one call per frame gives the same volume");
    one.reset();
    if (one.extractVoxelPointCloud().points.cols() != 0) return fail("reset empties the volume");
    one.injectVolumeTSDF(tw);
    one.injectVolumeColor(col);
    const teaser::TSDFPointCloud again = one.extractPointCloud(false);
    const size_t bytes = sizeof(double) * 3 * (size_t)count;
    if (again.points.cols() != count || again.normals.cols() != 0 || std::memcmp(again.points.data(), cloud.points.data(), bytes) != 0 ||
        std::memcmp(again.colors.data(), cloud.colors.data(), bytes) != 0)
      return fail("the injected volume gives the same surface");

    bool threw = false;
    try {
      vol.integrate(frames[0], K, E[0], /*depth_scale=*/0.0);
    } catch (const teaser::TSDFError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG;
    }
    if (!threw) return fail("a depth_scale of 0 throws BAD_ARG");
    threw = false;
    try {
      vol.integrate(teaser::DepthFrame::U16(depth[0].data(), w, h, 2 * padded), K, E[0]);  // no colour image for an RGB8 volume
    } catch (const teaser::TSDFError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG;
    }
    if (!threw) return fail("a frame without colour throws BAD_ARG for an RGB8 volume");
    threw = false;
    try {
      teaser::UniformTSDFVolume bad(1.0, 0, 0.15, teaser::TSDFVolumeColorType::NoColor);
    } catch (const teaser::TSDFError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG && std::string(e.what()).find("resolution") != std::string::npos;
    }
    if (!threw) return fail("a resolution of 0 throws BAD_ARG");
    if (vol.extractVolumeTSDF() != tw) return fail("the refusals left the volume alone");

    std::printf("count %lld\n", (long long)count);
    std::printf("points %016llx\nnormals %016llx\ncolors %016llx\n", fnv(cloud.points.data(), bytes), fnv(cloud.normals.data(), bytes),
                fnv(cloud.colors.data(), bytes));
    std::printf("vcount %lld\n", (long long)voxels.points.cols());
    std::printf("vpoints %016llx\nvcolors %016llx\n", fnv(voxels.points.data(), sizeof(double) * 3 * (size_t)voxels.points.cols()),
                fnv(voxels.colors.data(), sizeof(double) * 3 * (size_t)voxels.points.cols()));
    std::printf("tsdf %016llx\ncolor %016llx\n", fnv(tw.data(), sizeof(float) * tw.size()), fnv(col.data(), sizeof(double) * col.size()));
    std::printf("checks 1\n");
    return 0;
  } catch (const teaser::TSDFError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
