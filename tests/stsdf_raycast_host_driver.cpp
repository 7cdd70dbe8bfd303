// Host-only check of the ray cast of the scalable TSDF volume (tests/test_stsdf_raycast_host.py): csrc/stsdf.hip and
// csrc/stsdf_raycast.hip compiled by g++ against the HIP stand-in header (tests/hip_stub), built with -ffp-contract=off
// -fsanitize=address,undefined as a stand-alone program.  The volume's launchers, the reader of the case file and the
// helpers are those of tests/stsdf_host_driver.cpp, which is included with its main renamed (its cases are not run
// here); the ray cast's launcher is a serial loop over the blocks and their threads that calls stsdf_ray_thread of
// csrc/stsdf_raycast_device.h -- the text the kernel compiles, the pixel mapping and the block cache included.  "Device"
// buffers are host allocations of the size the host code asked for, so a view record, block map, directory or output
// layout that is sized or addressed wrongly is an AddressSanitizer report.  Depth, vertex, normal and colour maps are
// compared bit for bit, and the hit counts for equality, with those of tests/stsdf_raycast_reference.py, read from a
// text file.
//   stsdf_raycast_host_driver CASES.txt    exit code 0: every case equal and every refusal refused
// TEST INFRASTRUCTURE ONLY.
#define main stsdf_host_driver_main
#include "stsdf_host_driver.cpp"
#undef main
#include "../teaser-plusplus_amd/csrc/stsdf_raycast.hip"

static int g_ray_launches = 0;

namespace thip {

void launch_stsdf_raycast(hipStream_t, const TsdfGrid& g, const StsdfDir& dir, const StsdfRayArgs& a, int32_t n_blocks) {
  ++g_ray_launches;
  for (int32_t b = 0; b < n_blocks; ++b) {
    int32_t hits = 0;
    for (int t = 0; t < kTsdfRayBlock; ++t) hits += stsdf_ray_thread(g, dir, a, b, t) ? 1 : 0;
    a.blk_hits[b] = hits;
  }
}

}  // namespace thip

struct View {
  teaser_tsdf_view_c w;
  int64_t hits = 0;
  std::vector<uint32_t> depth, vertex, normal, color;
};
struct RayCase {
  teaser_stsdf_volume_c vol;
  int64_t blocks = 0;
  std::vector<int32_t> keys;
  std::vector<float> tw;
  std::vector<double> color;
  std::vector<View> views;
};

static std::vector<uint32_t> bits(const std::vector<float>& v) {
  std::vector<uint32_t> b(v.size());
  if (!v.empty()) memcpy(b.data(), v.data(), 4 * v.size());
  return b;
}

static const float kFill = -7.5f;

// The views `order` of the case in one call with the maps `maps` (bit 0 depth, 1 vertex, 2 normal, 3 colour) asked of
// every view, except that view order[0] asks for the depth alone when `first_depth_only`.
static void check_views(teaser_hip_stsdf* h, const RayCase& cs, const std::vector<int>& order, int maps, bool first_depth_only,
                        bool whole_arrays_null, int c, const char* what) {
  const size_t n = order.size();
  std::vector<teaser_tsdf_view_c> rec(n);
  std::vector<std::vector<float>> buf[4];
  std::vector<float*> ptr[4];
  for (int m = 0; m < 4; ++m) buf[m].resize(n), ptr[m].assign(n, nullptr);
  for (size_t k = 0; k < n; ++k) {
    const View& v = cs.views[(size_t)order[k]];
    rec[k] = v.w;
    const size_t px = (size_t)v.w.width * (size_t)v.w.height;
    for (int m = 0; m < 4; ++m) {
      const bool want = ((maps >> m) & 1) && !(first_depth_only && k == 0 && m != 0) && !(m == 3 && cs.vol.color_type == 0);
      if (!want) continue;
      buf[m][k].assign((m == 0 ? 1 : 3) * px + 2, kFill);  // two floats behind the map: they must stay
      ptr[m][k] = buf[m][k].data();
    }
  }
  std::vector<int64_t> hits(n, -5);
  float* const* arg[4];
  for (int m = 0; m < 4; ++m) {
    bool any = false;
    for (float* p : ptr[m]) any = any || p;
    arg[m] = !any && whole_arrays_null ? nullptr : ptr[m].data();
  }
  g_ray_launches = 0;
  const int32_t rc = teaser_hip_stsdf_ray_cast_views(h, (int32_t)n, rec.data(), arg[0], arg[1], arg[2], arg[3], hits.data());
  expect(rc == TEASER_HIP_OK, (std::string(what) + ": the call / " + teaser_hip_stsdf_last_error(h)).c_str(), c);
  if (rc != TEASER_HIP_OK) return;
  bool pixels = false;
  for (size_t k = 0; k < n; ++k) pixels = pixels || (rec[k].width > 0 && rec[k].height > 0);
  expect(g_ray_launches == (pixels ? 1 : 0), (std::string(what) + ": one launch").c_str(), c);
  for (size_t k = 0; k < n; ++k) {
    const View& v = cs.views[(size_t)order[k]];
    expect(hits[k] == v.hits, (std::string(what) + ": the hit count").c_str(), c);
    const std::vector<uint32_t>* want[4] = {&v.depth, &v.vertex, &v.normal, &v.color};
    const char* name[4] = {": depth bits", ": vertex bits", ": normal bits", ": colour bits"};
    for (int m = 0; m < 4; ++m) {
      if (!ptr[m][k]) continue;
      std::vector<float>& got = buf[m][k];
      expect(got[got.size() - 1] == kFill && got[got.size() - 2] == kFill, (std::string(what) + ": a float behind a map is written").c_str(), c);
      got.resize(got.size() - 2);
      expect(same(bits(got), *want[m]), (std::string(what) + name[m]).c_str(), c);
    }
  }
}

static void refused_view(teaser_hip_stsdf* h, const teaser_tsdf_view_c& good, void (*change)(teaser_tsdf_view_c&), const char* word) {
  teaser_tsdf_view_c two[2] = {good, good};
  change(two[1]);
  std::vector<float> d((size_t)good.width * good.height, kFill);
  float* dp[2] = {d.data(), d.data()};
  int64_t hits[2] = {-5, -5};
  refused(h, teaser_hip_stsdf_ray_cast_views(h, 2, two, dp, nullptr, nullptr, nullptr, hits), TEASER_HIP_ERR_BAD_ARG, word, "(view 1)");
  expect(d[0] == kFill && hits[0] == -5, "a refused call writes nothing", -1);
}

static teaser_hip_stsdf* volume_of(const RayCase& cs, int initial, int slab) {
  teaser_stsdf_volume_c vol = cs.vol;
  vol.initial_blocks = initial, vol.slab_blocks = slab;
  teaser_hip_stsdf* h = nullptr;
  if (teaser_hip_stsdf_create(&vol, 0, &h) != TEASER_HIP_OK) std::exit(2);
  if (cs.blocks > 0 &&
      teaser_hip_stsdf_upload_blocks(h, cs.blocks, cs.keys.data(), cs.tw.data(), cs.vol.color_type ? cs.color.data() : nullptr) != TEASER_HIP_OK)
    std::exit(2);
  return h;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int nc = (int)read_number(f);
  std::vector<RayCase> cases((size_t)nc);
  for (RayCase& cs : cases) {
    if (teaser_hip_stsdf_volume_default(&cs.vol) != TEASER_HIP_OK) return 2;
    cs.vol.color_type = (int)read_number(f);
    cs.vol.voxel_length = read_number(f), cs.vol.sdf_trunc = read_number(f);
    cs.blocks = (int64_t)read_number(f);
    const size_t n = (size_t)cs.blocks * thip::kStsdfVoxels;
    read_numbers(f, cs.keys, 3 * (size_t)cs.blocks);
    read_numbers(f, cs.tw, 2 * n);
    if (cs.vol.color_type) read_numbers(f, cs.color, 3 * n);
    cs.views.resize((size_t)read_number(f));
    for (View& v : cs.views) {
      memset(&v.w, 0, sizeof(v.w));  // every field is read from the file; reserved stays 0
      v.w.width = (int)read_number(f), v.w.height = (int)read_number(f);
      v.w.fx = read_number(f), v.w.fy = read_number(f), v.w.cx = read_number(f), v.w.cy = read_number(f);
      for (double& e : v.w.extrinsic) e = read_number(f);
      v.w.depth_min = read_number(f), v.w.depth_max = read_number(f), v.w.weight_threshold = read_number(f);
      v.hits = (int64_t)read_number(f);
      const size_t px = (size_t)v.w.width * (size_t)v.w.height;
      read_numbers(f, v.depth, px);
      read_numbers(f, v.vertex, 3 * px);
      read_numbers(f, v.normal, 3 * px);
      if (cs.vol.color_type) read_numbers(f, v.color, 3 * px);
    }
  }
  std::fclose(f);

  const RayCase* plain = nullptr;
  for (int c = 0; c < nc; ++c) {
    const RayCase& cs = cases[(size_t)c];
    if (!plain && cs.vol.color_type == 0 && cs.blocks > 0 && !cs.views.empty() && cs.views[0].w.width > 0) plain = &cs;
    teaser_hip_stsdf* h = volume_of(cs, 1024, 1024);
    std::vector<int> all, reversed;
    for (size_t k = 0; k < cs.views.size(); ++k) all.push_back((int)k), reversed.insert(reversed.begin(), (int)k);
    check_views(h, cs, all, 15, false, false, c, "all views, all maps");
    expect(!h->dir_dirty, "the call leaves the directory's device copy up to date", c);
    check_views(h, cs, reversed, 15, true, false, c, "reversed, the first view's depth alone");
    check_views(h, cs, all, 1, false, true, c, "depth alone, the other arrays NULL");
    check_views(h, cs, all, 6, false, false, c, "vertex and normal, depth entries NULL");
    check_views(h, cs, all, 0, false, true, c, "the counts alone");
    for (int k : all) check_views(h, cs, {k}, 15, false, false, c, "one view alone");
    g_ray_launches = 0;
    expect(teaser_hip_stsdf_ray_cast_views(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK && g_ray_launches == 0,
           "n_views = 0", c);
    // the ray cast leaves the blocks and the directory alone
    int64_t nb = -1;
    std::vector<int32_t> keys(cs.keys.size(), -9);
    std::vector<float> tw(cs.tw.size(), kFill);
    expect(teaser_hip_stsdf_block_keys(h, cs.blocks, cs.blocks ? keys.data() : nullptr, &nb) == TEASER_HIP_OK && nb == cs.blocks, "block keys", c);
    if (cs.blocks > 0) {
      expect(teaser_hip_stsdf_download_blocks(h, cs.blocks, tw.data(), nullptr, &nb) == TEASER_HIP_OK, "download", c);
      // the case file lists the blocks in ascending key order, as the download does
      expect(same(keys, cs.keys) && same(tw, cs.tw), "the ray cast leaves the volume alone", c);
    }
    teaser_hip_stsdf_destroy(h);
    // the same volume grown a block at a time: one slab per block, and a cast between the uploads (the directory goes up
    // again after every growth)
    if (cs.blocks > 1) {
      teaser_stsdf_volume_c vol = cs.vol;
      vol.initial_blocks = 1, vol.slab_blocks = 1;
      teaser_hip_stsdf* g = nullptr;
      if (teaser_hip_stsdf_create(&vol, 0, &g) != TEASER_HIP_OK) return 2;
      const size_t V = thip::kStsdfVoxels;
      for (int64_t k = cs.blocks - 1; k >= 0; --k) {  // descending: every new block is sorted in front of the others
        expect(teaser_hip_stsdf_upload_blocks(g, 1, &cs.keys[3 * (size_t)k], &cs.tw[2 * V * (size_t)k],
                                              cs.vol.color_type ? &cs.color[3 * V * (size_t)k] : nullptr) == TEASER_HIP_OK, "upload of one block", c);
        std::vector<float> d((size_t)cs.views[0].w.width * cs.views[0].w.height + 1, kFill);
        float* dp[1] = {d.data()};
        expect(teaser_hip_stsdf_ray_cast_views(g, 1, &cs.views[0].w, dp, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK, "a cast while the volume grows", c);
      }
      check_views(g, cs, all, 15, false, false, c, "grown a block at a time");
      teaser_hip_stsdf_destroy(g);
    }
  }

  // refusals: BAD_ARG with the view and the field named; the handle stays usable
  if (!plain) return 2;
  {
    const RayCase& cs = *plain;
    teaser_hip_stsdf* h = volume_of(cs, 1024, 1024);
    const teaser_tsdf_view_c good = cs.views[0].w;
    const double inf = INFINITY, nan = NAN;
    static double bad;
    refused_view(h, good, [](teaser_tsdf_view_c& w) { w.width = -1; }, "width and height must lie in [0, 16384]");
    refused_view(h, good, [](teaser_tsdf_view_c& w) { w.height = 16385; }, "width and height must lie in [0, 16384]");
    refused_view(h, good, [](teaser_tsdf_view_c& w) { w.fx = 0.0; }, "fx and fy must be finite and not zero");
    bad = inf;
    refused_view(h, good, [](teaser_tsdf_view_c& w) { w.fy = bad; }, "fx and fy must be finite and not zero");
    bad = nan;
    refused_view(h, good, [](teaser_tsdf_view_c& w) { w.cx = bad; }, "cx and cy must be finite");
    refused_view(h, good, [](teaser_tsdf_view_c& w) { w.cy = bad; }, "cx and cy must be finite");
    refused_view(h, good, [](teaser_tsdf_view_c& w) { w.extrinsic[15] = bad; }, "extrinsic has a non-finite entry");
    refused_view(h, good, [](teaser_tsdf_view_c& w) { w.depth_min = -0.5; }, "depth_min must be >= 0");
    refused_view(h, good, [](teaser_tsdf_view_c& w) { w.depth_min = bad; }, "depth_min, depth_max and weight_threshold must be finite");
    bad = inf;
    refused_view(h, good, [](teaser_tsdf_view_c& w) { w.depth_max = bad; }, "depth_min, depth_max and weight_threshold must be finite");
    refused_view(h, good, [](teaser_tsdf_view_c& w) { w.weight_threshold = -bad; }, "depth_min, depth_max and weight_threshold must be finite");
    refused_view(h, good, [](teaser_tsdf_view_c& w) { w.depth_max = 0.5 * w.depth_min; }, "depth_max must not be below depth_min");
    refused_view(h, good, [](teaser_tsdf_view_c& w) { w.reserved = 1; }, "reserved must be 0");
    std::vector<float> room(3 * (size_t)good.width * good.height, kFill);
    float* rp[1] = {room.data()};
    const int32_t B = TEASER_HIP_ERR_BAD_ARG;
    refused(h, teaser_hip_stsdf_ray_cast_views(h, 1, &good, nullptr, nullptr, nullptr, rp, nullptr), B, "color is asked of a volume without colour", "(view 0)");
    refused(h, teaser_hip_stsdf_ray_cast_views(h, 1, nullptr, rp, nullptr, nullptr, nullptr, nullptr), B, "views must not be NULL", "");
    refused(h, teaser_hip_stsdf_ray_cast_views(h, -1, &good, rp, nullptr, nullptr, nullptr, nullptr), B, "n_views must be >= 0", "");
    expect(room[0] == kFill, "a refused call writes nothing", -1);
    {  // 2048 views of 16384 x 16384 are 2^31 blocks, one too many; refused before anything is allocated or launched
      teaser_tsdf_view_c big = good;
      big.width = big.height = 16384;
      std::vector<teaser_tsdf_view_c> many(2048, big);
      int64_t counts[1] = {-5};
      g_ray_launches = 0;
      refused(h, teaser_hip_stsdf_ray_cast_views(h, 2048, many.data(), nullptr, nullptr, nullptr, nullptr, counts), B,
              "the views of one call need more than 2147483647 blocks", "(view 2047)");
      expect(g_ray_launches == 0 && counts[0] == -5, "the refusal of too many blocks launches and writes nothing", -1);
    }
    expect(teaser_hip_stsdf_ray_cast_views(nullptr, 1, &good, rp, nullptr, nullptr, nullptr, nullptr) == B, "refusal: NULL handle", -1);
    check_views(h, cs, {0}, 15, false, false, -1, "after the refusals");  // nothing above left a trace
    // a view that asks for the largest cap: depth_max far away on a volume of small voxels still ends
    teaser_tsdf_view_c far = good;
    far.width = far.height = 2, far.depth_max = 1e30;
    std::vector<float> d(4 + 1, kFill);
    float* dp[1] = {d.data()};
    expect(teaser_hip_stsdf_ray_cast_views(h, 1, &far, dp, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK && d[4] == kFill, "a far depth_max", -1);
    // reset: every pixel misses, the maps are zeros, and the launch still writes them
    expect(teaser_hip_stsdf_reset(h) == TEASER_HIP_OK, "reset", -1);
    std::vector<float> z((size_t)good.width * good.height, kFill);
    float* zp[1] = {z.data()};
    int64_t hits = -5;
    expect(teaser_hip_stsdf_ray_cast_views(h, 1, &good, zp, nullptr, nullptr, nullptr, &hits) == TEASER_HIP_OK && hits == 0, "an empty volume", -1);
    expect(z == std::vector<float>(z.size(), 0.0f), "an empty volume gives zeros", -1);
    teaser_hip_stsdf_destroy(h);
  }
  std::printf("cases %d  mismatches %d\n", nc, g_bad);
  return g_bad ? 1 : 0;
}
