// Host-only check of the ray-casting scene (tests/test_scene_host.py): csrc/scene.hip compiled by g++ against the HIP
// stand-in header (tests/hip_stub), built with -ffp-contract=off -fsanitize=address,undefined as a stand-alone program.
// The launchers are serial loops over the functions of csrc/scene_device.h -- the text the kernels compile: the bounds,
// the Morton keys, a stable sort, the hierarchy node by node, the leaves and ropes, the refit pass by pass, and both
// traversals lane by lane.  "Device" buffers are host allocations, so a record, an offset or a layout that is sized or
// addressed wrongly is an AddressSanitizer report.  Every output is compared bit for bit with tests/scene_reference.py,
// read from a text file of unsigned 32-bit words (float32 as their bits, doubles as two words, high first).
//   scene_host_driver CASES.txt      exit code 0: every case equal and every refusal refused
// TEST INFRASTRUCTURE ONLY.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

inline hipError_t hipHostMalloc(void** p, size_t n) { return hipHostMalloc(p, n, 0u); }
thread_local stub_dim3_ blockIdx, threadIdx, gridDim, blockDim;
template <class T> T atomicAdd(T* p, T v) { T o = *p; *p += v; return o; }
#define __forceinline__ inline

#include "../teaser-plusplus_amd/csrc/scene.hip"

static int g_launches = 0;

namespace thip {

size_t scene_sort_temp_bytes(int64_t n) { return (size_t)n; }

hipError_t launch_scene_keys(hipStream_t, const SceneBuild& b, void*, size_t) {
  ++g_launches;
  float r[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0f};
  for (int32_t g = 0; g < b.n; ++g) {
    float t[6];
    scene_tri_box(b.tri, (uint32_t)g, t, t + 3);
    for (int k = 0; k < 3; ++k) r[k] = std::min(r[k], t[k]), r[3 + k] = std::max(r[3 + k], t[3 + k]);
    for (int k = 0; k < 6; ++k) r[6] = std::max(r[6], std::fabs(t[k]));
  }
  for (int k = 0; k < 8; ++k) b.bounds[k] = k < 7 ? r[k] : 0.0f;
  for (int32_t g = 0; g < b.n; ++g) b.keys[0][g] = scene_morton(b.tri, (uint32_t)g, b.bounds), b.vals[0][g] = (uint32_t)g;
  std::vector<uint32_t> order((size_t)b.n);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return b.keys[0][x] < b.keys[0][y]; });
  for (int32_t i = 0; i < b.n; ++i) b.keys[1][i] = b.keys[0][order[(size_t)i]], b.vals[1][i] = b.vals[0][order[(size_t)i]];
  return hipSuccess;
}

void launch_scene_tree(hipStream_t, const SceneBuild& b, int passes) {
  for (int32_t i = 0; i + 1 < b.n; ++i) scene_hierarchy_node(b, i);
  for (int32_t i = b.n - 1; i >= 0; --i) scene_init_node(b, i);  // any order of the threads
  for (int p = 1; p <= passes; ++p)
    for (int32_t i = b.n - 2; i >= 0; --i) scene_refit_node(b, i, p);
  g_launches += 2 + passes;
  for (int32_t i = 0; i + 1 < b.n; ++i)
    if (b.level[i] == kSceneUnset) std::abort();  // the passes did not reach every node: the height bound is wrong
}

void launch_scene_rays(hipStream_t, const SceneRayArgs& a) {
  ++g_launches;
  for (int64_t i = 0; i < (a.n + kSceneBlock - 1) / kSceneBlock * kSceneBlock; ++i) scene_ray_thread(a, i);
}
void launch_scene_occlusions(hipStream_t, const SceneRayArgs& a) {
  ++g_launches;
  for (int64_t i = 0; i < (a.n + kSceneBlock - 1) / kSceneBlock * kSceneBlock; ++i) scene_occlusion_thread(a, i);
}
void launch_scene_points(hipStream_t, const ScenePointArgs& a) {
  ++g_launches;
  for (int64_t i = 0; i < (a.n + kSceneBlock - 1) / kSceneBlock * kSceneBlock; ++i) scene_point_thread(a, i);
}
void launch_scene_views(hipStream_t, const SceneViewArgs& a, int32_t n_blocks) {
  ++g_launches;
  for (int b = 0; b < n_blocks; ++b)
    for (int t = 0; t < kSceneBlock; ++t) scene_view_thread(a, b, t);
}

}  // namespace thip

static int g_bad = 0;
static void expect(bool ok, const std::string& what, int c) {
  if (!ok) {
    std::fprintf(stderr, "case %d: %s\n", c, what.c_str());
    ++g_bad;
  }
}

static uint32_t word(FILE* f) {
  unsigned v;
  if (std::fscanf(f, "%u", &v) != 1) std::exit(2);
  return (uint32_t)v;
}
template <class T>
static std::vector<T> words(FILE* f, size_t n) {
  static_assert(sizeof(T) == 4, "a word");
  std::vector<T> v(n);
  for (T& x : v) {
    const uint32_t w = word(f);
    memcpy(&x, &w, 4);
  }
  return v;
}
static double real(FILE* f) {
  const uint64_t hi = word(f), lo = word(f), b = hi << 32 | lo;
  double d;
  memcpy(&d, &b, 8);
  return d;
}

struct Maps {
  std::vector<float> t, uv, nrm, closest;
  std::vector<uint32_t> gid, pid;
  void read(FILE* f, size_t n, bool with_closest) {
    t = words<float>(f, n), gid = words<uint32_t>(f, n), pid = words<uint32_t>(f, n);
    uv = words<float>(f, 2 * n), nrm = words<float>(f, 3 * n);
    if (with_closest) closest = words<float>(f, 3 * n);
  }
  void size(size_t n, bool with_closest) {
    t.assign(n, -7.0f), gid.assign(n, 7u), pid.assign(n, 7u), uv.assign(2 * n, -7.0f), nrm.assign(3 * n, -7.0f);
    if (with_closest) closest.assign(3 * n, -7.0f);
  }
  template <class T>
  static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), 4 * a.size()) == 0);
  }
  bool operator==(const Maps& o) const {
    return same(t, o.t) && same(gid, o.gid) && same(pid, o.pid) && same(uv, o.uv) && same(nrm, o.nrm) && same(closest, o.closest);
  }
};

static teaser_hip_scene* read_scene(FILE* f, int c) {
  teaser_hip_scene* h = nullptr;
  expect(teaser_hip_scene_create(-1, &h) == TEASER_HIP_OK && h, "create", c);
  const int ng = (int)word(f);
  for (int k = 0; k < ng; ++k) {
    const size_t nv = word(f), nt = word(f);
    const std::vector<float> vert = words<float>(f, 3 * nv);
    const std::vector<uint32_t> tri = words<uint32_t>(f, 3 * nt);
    uint32_t id = 99;
    // exactly sized copies: a read past a mesh is a report
    expect(teaser_hip_scene_add_triangles(h, nv ? vert.data() : nullptr, (int64_t)nv, nt ? tri.data() : nullptr, (int64_t)nt, &id) == 0 &&
               id == (uint32_t)k, "add_triangles", c);
  }
  return h;
}

static void refusals(int c) {
  teaser_hip_scene* h = nullptr;
  expect(teaser_hip_scene_create(-1, &h) == TEASER_HIP_OK, "create", c);
  const float vert[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
  const uint32_t tri[3] = {0, 1, 2};
  auto refused = [&](int32_t rc, const char* text) {
    expect(rc == TEASER_HIP_ERR_BAD_ARG && std::string(teaser_hip_scene_last_error(h)).find(text) != std::string::npos,
           std::string("refusal: ") + text + " / got: " + teaser_hip_scene_last_error(h), c);
  };
  float bad[9];
  memcpy(bad, vert, sizeof(bad));
  bad[4] = NAN;
  refused(teaser_hip_scene_add_triangles(h, bad, 3, tri, 1, nullptr), "vertices has a non-finite entry (vertex 1)");
  bad[4] = INFINITY;
  refused(teaser_hip_scene_add_triangles(h, bad, 3, tri, 1, nullptr), "vertices has a non-finite entry (vertex 1)");
  const uint32_t over[6] = {0, 1, 2, 0, 3, 1};
  refused(teaser_hip_scene_add_triangles(h, vert, 3, over, 2, nullptr), "triangles has an index >= n_vertices (triangle 1)");
  refused(teaser_hip_scene_add_triangles(h, vert, -1, tri, 1, nullptr), "n_vertices must be >= 0");
  refused(teaser_hip_scene_add_triangles(h, vert, 3, tri, -1, nullptr), "n_triangles must be >= 0");
  refused(teaser_hip_scene_add_triangles(h, nullptr, 3, tri, 1, nullptr), "vertices must not be NULL");
  refused(teaser_hip_scene_add_triangles(h, vert, 3, nullptr, 1, nullptr), "triangles must not be NULL");
  refused(teaser_hip_scene_add_triangles(h, vert, 3, tri, 1073741825ll, nullptr), "at most 1073741824 triangles");
  int64_t count = -1;
  expect(teaser_hip_scene_triangle_count(h, &count) == 0 && count == 0, "a refused mesh adds nothing", c);
  expect(teaser_hip_scene_add_triangles(h, vert, 3, tri, 1, nullptr) == 0, "the handle stays usable", c);
  const float ray[6] = {0.25f, 0.25f, 1.0f, 0, 0, -1.0f};
  float t = 0;
  uint8_t occ = 9;
  refused(teaser_hip_scene_cast_rays(h, ray, -1, &t, nullptr, nullptr, nullptr, nullptr), "n must be >= 0");
  refused(teaser_hip_scene_cast_rays(h, nullptr, 1, &t, nullptr, nullptr, nullptr, nullptr), "rays must not be NULL");
  refused(teaser_hip_scene_test_occlusions(h, ray, 1, NAN, 1.0, &occ), "tnear must not be NaN");
  refused(teaser_hip_scene_test_occlusions(h, ray, 1, 0.0, NAN, &occ), "tfar must not be NaN");
  refused(teaser_hip_scene_test_occlusions(h, ray, 1, 0.0, 1.0, nullptr), "occluded must not be NULL");
  refused(teaser_hip_scene_test_occlusions(h, nullptr, 1, 0.0, 1.0, &occ), "rays must not be NULL");
  refused(teaser_hip_scene_closest_points(h, nullptr, 1, nullptr, &t, nullptr, nullptr, nullptr, nullptr), "points must not be NULL");
  refused(teaser_hip_scene_closest_points(h, ray, -2, nullptr, &t, nullptr, nullptr, nullptr, nullptr), "n must be >= 0");
  teaser_scene_view_c w;
  expect(teaser_hip_scene_view_default(&w) == 0 && w.pixel_offset == 0.5 && w.extrinsic[5] == 1.0 && w.extrinsic[1] == 0.0, "view_default", c);
  w.width = 4, w.height = 3, w.fx = w.fy = 2.0, w.cx = 2.0, w.cy = 1.5;
  float* tp[1] = {&t};
  refused(teaser_hip_scene_cast_views(h, &w, -1, nullptr, nullptr, nullptr, nullptr, nullptr), "n_views must be >= 0");
  refused(teaser_hip_scene_cast_views(h, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr), "views must not be NULL");
  auto view_refused = [&](teaser_scene_view_c v, const char* text) {
    refused(teaser_hip_scene_cast_views(h, &v, 1, tp, nullptr, nullptr, nullptr, nullptr), text);
  };
  teaser_scene_view_c v = w;
  v.width = -1, view_refused(v, "width and height must lie in [0, 16384] (view 0)");
  v = w, v.height = 16385, view_refused(v, "width and height must lie in [0, 16384] (view 0)");
  v = w, v.fx = 0.0, view_refused(v, "fx and fy must be finite and not zero (view 0)");
  v = w, v.fy = NAN, view_refused(v, "fx and fy must be finite and not zero (view 0)");
  v = w, v.cx = INFINITY, view_refused(v, "cx and cy must be finite (view 0)");
  v = w, v.extrinsic[7] = NAN, view_refused(v, "extrinsic has a non-finite entry (view 0)");
  v = w, v.pixel_offset = NAN, view_refused(v, "pixel_offset must be finite (view 0)");
  v = w, v.reserved = 1, view_refused(v, "reserved must be 0 (view 0)");
  // after all that the handle answers: the ray meets the triangle at t = 1, a zero-sized query is legal
  expect(teaser_hip_scene_cast_rays(h, ray, 1, &t, nullptr, nullptr, nullptr, nullptr) == 0 && t == 1.0f, "usable after refusals", c);
  expect(teaser_hip_scene_cast_rays(h, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0, "zero rays", c);
  expect(teaser_hip_scene_closest_points(h, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0, "zero points", c);
  expect(teaser_hip_scene_cast_views(h, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0, "zero views", c);
  expect(teaser_hip_scene_test_occlusions(h, ray, 1, 0.0, INFINITY, &occ) == 0 && occ == 1, "occluded", c);
  expect(teaser_hip_scene_cast_rays(nullptr, ray, 1, &t, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG, "NULL handle", c);
  int64_t filled = -1;
  expect(teaser_hip_scene_fill_scratch(h, 256, &filled) == TEASER_HIP_ERR_BAD_ARG, "fill byte range", c);
  expect(teaser_hip_scene_destroy(h) == 0 && teaser_hip_scene_destroy(nullptr) == 0, "destroy", c);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int n_cases = (int)word(f);
  for (int c = 0; c < n_cases; ++c) {
    teaser_hip_scene* h = read_scene(f, c);
    int64_t filled = 0;
    // rays
    const size_t nr = word(f);
    const std::vector<float> rays = words<float>(f, 6 * nr);
    Maps want, got;
    want.read(f, nr, false);
    got.size(nr, false);
    expect(teaser_hip_scene_cast_rays(h, nr ? rays.data() : nullptr, (int64_t)nr, got.t.data(), got.gid.data(), got.pid.data(),
                                      got.uv.data(), got.nrm.data()) == 0, std::string("cast_rays: ") + teaser_hip_scene_last_error(h), c);
    expect(got == want, "cast_rays differs from the restatement", c);
    expect(teaser_hip_scene_fill_scratch(h, 0xA5, &filled) == 0, "fill_scratch", c);
    // only some maps, in chunks, back to front: the same bits per ray
    Maps part;
    part.size(nr, false);
    for (size_t a = 0; a < nr; a += 100) {
      const size_t m = std::min<size_t>(100, nr - a);
      std::vector<float> rev(6 * m);
      for (size_t i = 0; i < m; ++i) memcpy(&rev[6 * i], &rays[6 * (a + m - 1 - i)], 24);
      std::vector<float> t(m);
      std::vector<uint32_t> pid(m);
      expect(teaser_hip_scene_cast_rays(h, rev.data(), (int64_t)m, t.data(), nullptr, pid.data(), nullptr, nullptr) == 0, "cast_rays (chunk)", c);
      for (size_t i = 0; i < m; ++i) part.t[a + m - 1 - i] = t[i], part.pid[a + m - 1 - i] = pid[i];
    }
    expect(Maps::same(part.t, want.t) && Maps::same(part.pid, want.pid), "chunked cast_rays differs", c);
    // occlusions
    const double tnear = real(f), tfar = real(f);
    const std::vector<uint32_t> occ_want = words<uint32_t>(f, nr);
    std::vector<uint8_t> occ(nr, 7);
    expect(teaser_hip_scene_test_occlusions(h, nr ? rays.data() : nullptr, (int64_t)nr, tnear, tfar, occ.data()) == 0, "test_occlusions", c);
    for (size_t i = 0; i < nr; ++i)
      if (occ[i] != occ_want[i]) {
        expect(false, "test_occlusions differs at ray " + std::to_string(i), c);
        break;
      }
    // points
    const size_t np = word(f);
    const std::vector<float> pts = words<float>(f, 3 * np);
    Maps pwant, pgot;
    pwant.read(f, np, true);
    pgot.size(np, true);
    expect(teaser_hip_scene_closest_points(h, np ? pts.data() : nullptr, (int64_t)np, pgot.closest.data(), pgot.t.data(), pgot.gid.data(),
                                           pgot.pid.data(), pgot.uv.data(), pgot.nrm.data()) == 0,
           std::string("closest_points: ") + teaser_hip_scene_last_error(h), c);
    expect(pgot == pwant, "closest_points differs from the restatement", c);
    // views
    const int nv = (int)word(f);
    std::vector<teaser_scene_view_c> views((size_t)nv);
    std::vector<Maps> vwant((size_t)nv), vgot((size_t)nv);
    std::vector<float*> pt, puv, pn;
    std::vector<uint32_t*> pg, pp;
    for (int b = 0; b < nv; ++b) {
      teaser_scene_view_c& w = views[(size_t)b];
      teaser_hip_scene_view_default(&w);
      w.width = (int32_t)word(f), w.height = (int32_t)word(f);
      w.fx = real(f), w.fy = real(f), w.cx = real(f), w.cy = real(f);
      for (int k = 0; k < 16; ++k) w.extrinsic[k] = real(f);
      w.pixel_offset = real(f);
      const size_t px = (size_t)w.width * (size_t)w.height;
      vwant[(size_t)b].read(f, px, false);
      vgot[(size_t)b].size(px, false);
      Maps& g = vgot[(size_t)b];
      pt.push_back(g.t.data()), pg.push_back(g.gid.data()), pp.push_back(g.pid.data());
      puv.push_back(b % 2 ? nullptr : g.uv.data()), pn.push_back(g.nrm.data());  // odd views ask for no uv
    }
    expect(teaser_hip_scene_cast_views(h, views.data(), nv, pt.data(), pg.data(), pp.data(), puv.data(), pn.data()) == 0,
           std::string("cast_views: ") + teaser_hip_scene_last_error(h), c);
    for (int b = 0; b < nv; ++b) {
      if (b % 2) vgot[(size_t)b].uv = vwant[(size_t)b].uv;
      expect(vgot[(size_t)b] == vwant[(size_t)b], "cast_views differs from cast_rays on the pinhole rays, view " + std::to_string(b), c);
    }
    // a further geometry after the queries: the rebuilt scene answers the first ray as before or nearer
    if (nr > 0) {
      const float far_tri[9] = {1e6f, 1e6f, 1e6f, 1e6f + 1, 1e6f, 1e6f, 1e6f, 1e6f + 1, 1e6f};
      const uint32_t idx[3] = {0, 1, 2};
      uint32_t id = 0;
      int64_t before = 0, after = 0;
      teaser_hip_scene_triangle_count(h, &before);
      expect(teaser_hip_scene_add_triangles(h, far_tri, 3, idx, 1, &id) == 0, "add after queries", c);
      teaser_hip_scene_triangle_count(h, &after);
      expect(after == before + 1, "triangle_count", c);
      expect(teaser_hip_scene_commit(h) == 0, "commit", c);
      Maps again;
      again.size(nr, false);
      expect(teaser_hip_scene_cast_rays(h, rays.data(), (int64_t)nr, again.t.data(), again.gid.data(), again.pid.data(), nullptr, nullptr) == 0,
             "cast_rays after rebuild", c);
      size_t differ = 0;
      for (size_t i = 0; i < nr; ++i) differ += again.gid[i] != want.gid[i] && again.gid[i] != id;
      expect(differ == 0, "the rebuilt scene changed hits it should not", c);
    }
    expect(teaser_hip_scene_destroy(h) == 0, "destroy", c);
  }
  std::fclose(f);
  refusals(n_cases);
  std::printf("cases %d launches %d mismatches %d\n", n_cases, g_launches, g_bad);
  return g_bad ? 1 : 0;
}
