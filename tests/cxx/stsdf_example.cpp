// teaser::ScalableTSDFVolume (include/teaser/tsdf.h) used like Open3D's class.  No input file: the two 40 x 30 uint16
// depth frames and RGB images of tests/cxx/tsdf_example.cpp, given by formulas (tests/test_gpu_stsdf_cxx.py builds the same
// arrays), integrated in one call into a scalable RGB8 volume with voxels of 1/16.  The record printed -- counts and
// FNV-1a hashes of the bytes of every output -- is what the test compares with the numpy restatement's.
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cstdio>
#include <cstring>
#include <vector>

#include "teaser/tsdf.h"

static int fail(const char* what) {
  std::fprintf(stderr, "stsdf_example: %s\n", what);
  return 1;
}

static unsigned long long fnv(const void* p, size_t bytes) {
  unsigned long long h = 1469598103934665603ull;
  const unsigned char* b = (const unsigned char*)p;
  for (size_t k = 0; k < bytes; ++k) h = (h ^ b[k]) * 1099511628211ull;
  return h;
}

static bool same(const teaser::Matrix3X& a, const teaser::Matrix3X& b) {
  return a.cols() == b.cols() && (a.cols() == 0 || std::memcmp(a.data(), b.data(), sizeof(double) * 3 * (size_t)a.cols()) == 0);
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

    teaser::ScalableTSDFVolume vol(0.0625, 0.15, teaser::TSDFVolumeColorType::RGB8);
    if (vol.voxelLength() != 0.0625 || vol.blockCount() != 0) return fail("a fresh volume has no blocks");
    if (vol.extractPointCloud().points.cols() != 0) return fail("a fresh volume is empty");
    vol.integrateBatch(frames, {K}, E);
    const teaser::ScalableTSDFVolume::Counts counts = vol.lastCounts();
    const std::vector<int32_t> keys = vol.blockKeys();
    if (vol.blockCount() <= 1 || keys.size() != 3 * (size_t)vol.blockCount() || counts.opened != vol.blockCount() ||
        counts.touched < counts.opened || counts.out_of_range != 0)
      return fail("the blocks and the counts");
    const teaser::TSDFPointCloud cloud = vol.extractPointCloud();
    const int64_t count = cloud.points.cols();
    if (count <= 0 || cloud.normals.cols() != count || cloud.colors.cols() != count) return fail("the surface has rows");
    const teaser::TSDFPointCloud voxels = vol.extractVoxelPointCloud();
    if (voxels.points.cols() <= count / 3 || voxels.normals.cols() != 0) return fail("the voxel cloud");

    // a second volume, alive beside the first, fed one frame per call: the same bits
    teaser::ScalableTSDFVolume one(0.0625, 0.15, teaser::TSDFVolumeColorType::RGB8, 16, 4);
    int64_t opened = 0;
    for (int k = 0; k < 2; ++k) {
      one.integrate(frames[(size_t)k], K, E[(size_t)k]);
      opened += one.lastCounts().opened;
    }
    const teaser::TSDFPointCloud again = one.extractPointCloud();
    if (opened != counts.opened || one.blockKeys() != keys || !same(again.points, cloud.points) || !same(again.normals, cloud.normals) ||
        !same(again.colors, cloud.colors) || !same(one.extractVoxelPointCloud().points, voxels.points))
      return fail("one call per frame gives the same volume");
    if (one.extractPointCloud(false).normals.cols() != 0) return fail("no normals when none are asked for");
    one.reset();
    if (one.blockCount() != 0 || one.extractVoxelPointCloud().points.cols() != 0) return fail("reset closes every block");

    bool threw = false;
    try {
      vol.integrate(frames[0], K, E[0], /*depth_scale=*/0.0);
    } catch (const teaser::TSDFError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG;
    }
    if (!threw) return fail("a depth_scale of 0 throws BAD_ARG");
    threw = false;
    try {
      teaser::Matrix4 flat = teaser::Matrix4::Identity();
      flat(2, 2) = 0.0;  // no inverse
      vol.integrate(frames[0], K, flat);
    } catch (const teaser::TSDFError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG && std::string(e.what()).find("singular") != std::string::npos;
    }
    if (!threw) return fail("a singular extrinsic throws BAD_ARG");
    threw = false;
    try {
      teaser::ScalableTSDFVolume bad(0.0625, 0.15, teaser::TSDFVolumeColorType::NoColor, 8);
    } catch (const teaser::TSDFError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG && std::string(e.what()).find("only 16") != std::string::npos;
    }
    if (!threw) return fail("a volume_unit_resolution of 8 throws BAD_ARG");
    threw = false;
    try {
      teaser::ScalableTSDFVolume bad(0.0625, 1.5, teaser::TSDFVolumeColorType::NoColor);
    } catch (const teaser::TSDFError& e) {
      threw = e.status() == TEASER_HIP_ERR_BAD_ARG && std::string(e.what()).find("sdf_trunc") != std::string::npos;
    }
    if (!threw) return fail("an sdf_trunc above a block's side throws BAD_ARG");
    if (vol.blockKeys() != keys || !same(vol.extractPointCloud().points, cloud.points)) return fail("the refusals left the volume alone");

    const size_t bytes = sizeof(double) * 3 * (size_t)count, vbytes = sizeof(double) * 3 * (size_t)voxels.points.cols();
    std::printf("blocks %lld\ntouched %lld\nopened %lld\n", (long long)vol.blockCount(), (long long)counts.touched, (long long)counts.opened);
    std::printf("keys %016llx\n", fnv(keys.data(), sizeof(int32_t) * keys.size()));
    std::printf("count %lld\n", (long long)count);
    std::printf("points %016llx\nnormals %016llx\ncolors %016llx\n", fnv(cloud.points.data(), bytes), fnv(cloud.normals.data(), bytes),
                fnv(cloud.colors.data(), bytes));
    std::printf("vcount %lld\n", (long long)voxels.points.cols());
    std::printf("vpoints %016llx\nvcolors %016llx\n", fnv(voxels.points.data(), vbytes), fnv(voxels.colors.data(), vbytes));
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
