// teaser::ScalableTSDFVolume::rayCast and rayCastBatch (include/teaser/tsdf.h) used like Open3D's ray_cast.  The frames
// are those of tests/cxx/tsdf_example.cpp (tests/test_gpu_tsdf_cxx.py builds the same arrays), the volume that of
// tests/cxx/stsdf_example.cpp.  The record printed -- hit counts and FNV-1a hashes of the bytes of every map -- is what
// tests/test_gpu_stsdf_raycast_cxx.py compares with the Python calls'.
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cstdio>
#include <cstring>
#include <vector>

#include "teaser/tsdf.h"

static int fail(const char* what) {
  std::fprintf(stderr, "stsdf_raycast_example: %s\n", what);
  return 1;
}

static unsigned long long fnv(const void* p, size_t bytes) {
  unsigned long long h = 1469598103934665603ull;
  const unsigned char* b = (const unsigned char*)p;
  for (size_t k = 0; k < bytes; ++k) h = (h ^ b[k]) * 1099511628211ull;
  return h;
}

static unsigned long long fnv(const std::vector<float>& v) { return fnv(v.data(), sizeof(float) * v.size()); }

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
    teaser::TSDFRayCastOptions opt;
    opt.weight_threshold = 2.0;  // two frames were integrated
    const teaser::TSDFRayCastResult none = vol.rayCast(K, E[0], w, h, opt);
    if (none.hits != 0 || none.depth.size() != (size_t)(w * h) || none.color.size() != (size_t)(3 * w * h)) return fail("a fresh volume shows nothing");
    for (float z : none.depth)
      if (z != 0.0f) return fail("a fresh volume shows nothing");
    vol.integrateBatch(frames, {K}, E);
    const teaser::TSDFRayCastResult one = vol.rayCast(K, E[1], w, h, opt);
    if (one.hits <= 0 || one.hits >= (int64_t)(w * h)) return fail("the model frame has hits and misses");
    if (one.width != w || one.height != h || one.vertex_map.size() != (size_t)(3 * w * h) || one.normal_map.size() != one.vertex_map.size() ||
        one.color.size() != one.vertex_map.size())
      return fail("the sizes of the maps");
    int64_t seen = 0;
    for (float z : one.depth) seen += z != 0.0f;
    if (seen != one.hits) return fail("the depth of a hit is not 0 here, that of a miss is");
    // two views of different sizes in one call: the first equals the call above
    const std::vector<teaser::TSDFRayCastResult> two = vol.rayCastBatch({K}, {E[1], E[0]}, {w, 17}, {h, 9}, opt);
    if (two.size() != 2 || two[0].hits != one.hits || two[0].depth != one.depth || two[0].vertex_map != one.vertex_map ||
        std::memcmp(two[0].color.data(), one.color.data(), sizeof(float) * one.color.size()) != 0)
      return fail("a view in a batch equals the view alone");
    if (two[1].width != 17 || two[1].depth.size() != 17u * 9u) return fail("the second view's size");
    teaser::TSDFRayCastOptions depth_only = opt;
    depth_only.vertex_map = depth_only.normal_map = depth_only.color = false;
    const teaser::TSDFRayCastResult d = vol.rayCast(K, E[1], w, h, depth_only);
    if (!d.vertex_map.empty() || !d.normal_map.empty() || !d.color.empty() || d.depth != one.depth || d.hits != one.hits)
      return fail("the depth alone");
    teaser::ScalableTSDFVolume bare(0.0625, 0.15, teaser::TSDFVolumeColorType::NoColor);
    bare.integrateBatch(frames, {K}, E);
    const teaser::TSDFRayCastResult grey = bare.rayCast(K, E[1], w, h, opt);
    if (!grey.color.empty() || grey.depth != one.depth) return fail("a volume without colour gives the same depth");
    bool refused = false;
    try {
      teaser::TSDFRayCastOptions bad = opt;
      bad.depth_max = 0.01;
      vol.rayCast(K, E[1], w, h, bad);
    } catch (const teaser::TSDFError& e) {
      refused = e.status() == TEASER_HIP_ERR_BAD_ARG && std::strstr(e.what(), "depth_max must not be below depth_min (view 0)");
    }
    if (!refused) return fail("depth_max below depth_min is refused with its text");

    std::printf("hits %lld\nhits_small %lld\n", (long long)one.hits, (long long)two[1].hits);
    std::printf("depth_bits %016llx\nvertex_bits %016llx\nnormal_bits %016llx\ncolor_bits %016llx\nsmall_depth_bits %016llx\n", fnv(one.depth),
                fnv(one.vertex_map), fnv(one.normal_map), fnv(one.color), fnv(two[1].depth));
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
