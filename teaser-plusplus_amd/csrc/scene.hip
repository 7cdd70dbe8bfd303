// scene.hip -- host side of the ray-casting scene (include/teaser_hip.h, "Ray casting scene"): the handle, the
// geometries, the build and the layout and one round trip of every query.  Kernels: kernels_scene.hip; device code:
// scene_device.h; design, the margins argument, bounds and the resource report: DESIGN.md section 41.
//
// The handle keeps the triangles of all geometries on the host in global order (nine floats each) and, per geometry,
// its first global index.  A query on an uncommitted scene builds first, on the same stream.
// A query: the inputs go up in one copy, the counter words are zeroed, one launch writes the requested maps into one
// buffer, one copy brings it back into the page-locked buffer, one synchronisation, and the host hands the maps out and
// splits the global triangle index into geometry and primitive.  A scene without a triangle answers on the host.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_common.h"
#include "scene_device.h"

struct teaser_hip_scene : thip::HandleBase {
  std::vector<float> tri;      // 9 per triangle, global order
  std::vector<int64_t> first;  // per geometry its first global index; one more entry: the total
  bool committed = true;       // an empty scene has nothing to build
  int64_t built = 0;           // triangles in the tree on the device
  thip::DevBuf tri_d, nodes, bounds;         // state: the tree
  thip::DevBuf work, sort_tmp, in, out;      // scratch
  thip::HostBuf stage, back;
  teaser_hip_scene() { first.push_back(0); }
};

namespace thip {

size_t scene_sort_temp_bytes(int64_t n);
hipError_t launch_scene_keys(hipStream_t s, const SceneBuild& b, void* d_temp, size_t temp_bytes);
void launch_scene_tree(hipStream_t s, const SceneBuild& b, int passes);
void launch_scene_rays(hipStream_t s, const SceneRayArgs& a);
void launch_scene_occlusions(hipStream_t s, const SceneRayArgs& a);
void launch_scene_points(hipStream_t s, const ScenePointArgs& a);
void launch_scene_views(hipStream_t s, const SceneViewArgs& a, int32_t n_blocks);

namespace {

constexpr int64_t kSceneMaxTriangles = 1073741824;  // 2^30
constexpr int32_t kSceneMaxSide = 16384;

inline size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int64_t total(const teaser_hip_scene* h) { return h->first.back(); }
inline std::string scene_view_at(int b) { return " (view " + std::to_string(b) + ")"; }

// The height of the radix tree is at most the number of distinct prefix lengths on a path: 63 code bits and the bits
// of the largest position.
inline int refit_passes(int64_t n) {
  int bits = 0;
  for (int64_t x = n - 1; x > 0; x >>= 1) ++bits;
  return 63 + bits;
}

// Builds an uncommitted scene on the stream and waits for it (the triangles are uploaded from pageable memory).
int32_t build(teaser_hip_scene* h) {
  if (h->committed) return TEASER_HIP_OK;
  const int64_t n = total(h);
  if (n == 0) {
    h->committed = true, h->built = 0;
    return TEASER_HIP_OK;
  }
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  const size_t o_k0 = 0, o_k1 = o_k0 + up(8 * (size_t)n, 256), o_v0 = o_k1 + up(8 * (size_t)n, 256);
  const size_t o_v1 = o_v0 + up(4 * (size_t)n, 256), o_last = o_v1 + up(4 * (size_t)n, 256);
  const size_t o_rope = o_last + up(4 * (size_t)n, 256), o_level = o_rope + up(4 * (size_t)n, 256);
  const size_t o_part = o_level + up(8 * (size_t)n, 256), o_end = o_part + 32 * (size_t)kSceneMaxBoundsBlocks;
  const size_t tmp = scene_sort_temp_bytes(n);
  if (!h->tri_d.ensure(36 * (size_t)n) || !h->nodes.ensure(sizeof(SceneNode) * (size_t)(2 * n - 1)) || !h->bounds.ensure(32) ||
      !h->work.ensure(o_end) || !h->sort_tmp.ensure(std::max<size_t>(tmp, 256)))
    return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (scene build buffers)");
  hipStream_t s = h->stream;
  FCHK(h, hipMemcpyAsync(h->tri_d.p, h->tri.data(), 36 * (size_t)n, hipMemcpyHostToDevice, s), "hipMemcpyAsync (triangles)");
  char* w = h->work.as<char>();
  SceneBuild b;
  memset(&b, 0, sizeof(b));
  b.tri = h->tri_d.as<float>();
  b.bounds = h->bounds.as<float>();
  b.partial = reinterpret_cast<float*>(w + o_part);
  b.keys[0] = reinterpret_cast<uint64_t*>(w + o_k0), b.keys[1] = reinterpret_cast<uint64_t*>(w + o_k1);
  b.vals[0] = reinterpret_cast<uint32_t*>(w + o_v0), b.vals[1] = reinterpret_cast<uint32_t*>(w + o_v1);
  b.nodes = h->nodes.as<SceneNode>();
  b.last = reinterpret_cast<int32_t*>(w + o_last);
  b.rope_target = reinterpret_cast<int32_t*>(w + o_rope);
  b.level = reinterpret_cast<int32_t*>(w + o_level);
  b.n = (int32_t)n;
  FCHK(h, launch_scene_keys(s, b, h->sort_tmp.p, tmp), "radix sort (scene keys)");
  launch_scene_tree(s, b, refit_passes(n));
  FCHK(h, hipGetLastError(), "kernel launch (scene build)");
  // the pageable triangle array must not change before the copy has run: add_triangles may follow at once
  FCHK(h, hipStreamSynchronize(s), "scene build");
  h->committed = true, h->built = n;
  return TEASER_HIP_OK;
}

SceneTree tree_of(const teaser_hip_scene* h) {
  SceneTree t;
  memset(&t, 0, sizeof(t));
  t.tri = h->tri_d.as<float>();
  t.nodes = h->nodes.as<SceneNode>();
  t.bounds = h->bounds.as<float>();
  t.n = (int32_t)h->built;
  t.cap = 4 * h->built + 64;
  return t;
}

// The words of a call's output buffer: the counters, then every wanted map on a 256-byte line.
struct Layout {
  size_t words = kSceneCounterWords;
  int64_t take(bool want, size_t count) {
    if (!want) return -1;
    const int64_t at = (int64_t)words;
    words += up(count, 64);
    return at;
  }
};

// What every query does around its launch.  in_bytes of h->stage go up; out_words come back into h->back.
template <class Launch>
int32_t round_trip(teaser_hip_scene* h, size_t in_bytes, size_t out_words, Launch launch) {
  hipStream_t s = h->stream;
  if (in_bytes) FCHK(h, hipMemcpyAsync(h->in.p, h->stage.p, in_bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync (scene inputs)");
  FCHK(h, hipMemsetAsync(h->out.p, 0, 4 * (size_t)kSceneCounterWords, s), "hipMemsetAsync (scene counters)");
  launch(s);
  FCHK(h, hipGetLastError(), "kernel launch (scene query)");
  FCHK(h, hipMemcpyAsync(h->back.p, h->out.p, 4 * out_words, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (scene outputs)");
  FCHK(h, hipStreamSynchronize(s), "scene query");
  const uint32_t capped = h->back.as<uint32_t>()[0];
  if (capped != 0)
    return fail(h, TEASER_HIP_ERR_HIP, "a traversal reached its visit cap (" + std::to_string(capped) + " lanes): the tree is damaged");
  return TEASER_HIP_OK;
}

bool ensure_io(teaser_hip_scene* h, size_t in_bytes, size_t out_words) {
  return h->in.ensure(std::max<size_t>(in_bytes, 256)) && h->stage.ensure(std::max<size_t>(in_bytes, 256)) &&
         h->out.ensure(4 * out_words) && h->back.ensure(4 * out_words);
}

// The maps of `count` items from the words of `back` at the offsets of `o` to the caller's arrays; the global index is
// split into the geometry and the primitive inside it.
void hand_out(const teaser_hip_scene* h, const uint32_t* back, const SceneOut& o, size_t count, float* t, uint32_t* gid,
              uint32_t* pid, float* uv, float* nrm, float* closest) {
  if (t && o.off_t >= 0) memcpy(t, back + o.off_t, 4 * count);
  if (uv && o.off_uv >= 0) memcpy(uv, back + o.off_uv, 8 * count);
  if (nrm && o.off_n >= 0) memcpy(nrm, back + o.off_n, 12 * count);
  if (closest && o.off_c >= 0) memcpy(closest, back + o.off_c, 12 * count);
  if ((gid || pid) && o.off_g >= 0) {
    const uint32_t* g = back + o.off_g;
    for (size_t i = 0; i < count; ++i) {
      uint32_t geo = kSceneNone, prim = kSceneNone;
      if (g[i] != kSceneNone) {
        const size_t k = (size_t)(std::upper_bound(h->first.begin(), h->first.end(), (int64_t)g[i]) - h->first.begin()) - 1;
        geo = (uint32_t)k, prim = (uint32_t)((int64_t)g[i] - h->first[k]);
      }
      if (gid) gid[i] = geo;
      if (pid) pid[i] = prim;
    }
  }
}

// A scene without a triangle: every item misses.
void all_miss(size_t count, float* t, uint32_t* gid, uint32_t* pid, float* uv, float* nrm, float* closest) {
  for (size_t i = 0; i < count; ++i) {
    if (t) t[i] = INFINITY;
    if (gid) gid[i] = kSceneNone;
    if (pid) pid[i] = kSceneNone;
  }
  if (uv) memset(uv, 0, 8 * count);
  if (nrm) memset(nrm, 0, 12 * count);
  if (closest) memset(closest, 0, 12 * count);
}

int32_t check_view(teaser_hip_scene* h, int b, const teaser_scene_view_c& w) {
  if (w.width < 0 || w.height < 0 || w.width > kSceneMaxSide || w.height > kSceneMaxSide)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "width and height must lie in [0, 16384]" + scene_view_at(b));
  if (!std::isfinite(w.fx) || !std::isfinite(w.fy) || w.fx == 0.0 || w.fy == 0.0)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "fx and fy must be finite and not zero" + scene_view_at(b));
  if (!std::isfinite(w.cx) || !std::isfinite(w.cy))
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "cx and cy must be finite" + scene_view_at(b));
  if (!finite_all(w.extrinsic, 16))
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "extrinsic has a non-finite entry" + scene_view_at(b));
  if (!std::isfinite(w.pixel_offset)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "pixel_offset must be finite" + scene_view_at(b));
  if (w.reserved != 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "reserved must be 0" + scene_view_at(b));
  return TEASER_HIP_OK;
}

template <class T>
inline T* entry(T* const* a, int b) { return a ? a[b] : nullptr; }

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" {

int32_t teaser_hip_scene_create(int32_t device, teaser_hip_scene** out) { return open_handle(device, out); }

int32_t teaser_hip_scene_destroy(teaser_hip_scene* h) { return close_handle(h); }

const char* teaser_hip_scene_last_error(const teaser_hip_scene* h) { return h ? h->err.c_str() : ""; }

int32_t teaser_hip_scene_fill_scratch(teaser_hip_scene* h, int32_t byte, int64_t* bytes_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  // not tri_d, nodes and bounds: the tree is the handle's state
  const ScratchSpan spans[] = {span_of(h->work), span_of(h->sort_tmp), span_of(h->in),
                               span_of(h->out),  span_of(h->stage),    span_of(h->back)};
  return fill_scratch(h, byte, spans, 6, bytes_out);
}

int32_t teaser_hip_scene_add_triangles(teaser_hip_scene* h, const float* vertices, int64_t n_vertices,
                                       const uint32_t* triangles, int64_t n_triangles, uint32_t* geometry_id_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (n_vertices < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_vertices must be >= 0");
  if (n_triangles < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_triangles must be >= 0");
  if (n_vertices > 0 && !vertices) return fail(h, TEASER_HIP_ERR_BAD_ARG, "vertices must not be NULL");
  if (n_triangles > 0 && !triangles) return fail(h, TEASER_HIP_ERR_BAD_ARG, "triangles must not be NULL");
  if (total(h) + n_triangles > kSceneMaxTriangles)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "a scene holds at most 1073741824 triangles");
  for (int64_t i = 0; i < 3 * n_vertices; ++i)
    if (!std::isfinite(vertices[i]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "vertices has a non-finite entry (vertex " + std::to_string(i / 3) + ")");
  for (int64_t i = 0; i < 3 * n_triangles; ++i)
    if ((int64_t)triangles[i] >= n_vertices)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "triangles has an index >= n_vertices (triangle " + std::to_string(i / 3) + ")");
  const size_t at = h->tri.size();
  h->tri.resize(at + 9 * (size_t)n_triangles);
  for (int64_t i = 0; i < 3 * n_triangles; ++i) memcpy(&h->tri[at + 3 * (size_t)i], vertices + 3 * (size_t)triangles[i], 12);
  if (geometry_id_out) *geometry_id_out = (uint32_t)(h->first.size() - 1);
  h->first.push_back(total(h) + n_triangles);
  h->committed = false;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_scene_commit(teaser_hip_scene* h) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  return build(h);
}

int32_t teaser_hip_scene_triangle_count(const teaser_hip_scene* h, int64_t* count_out) {
  if (!h || !count_out) return TEASER_HIP_ERR_BAD_ARG;
  *count_out = total(h);
  return TEASER_HIP_OK;
}

int32_t teaser_hip_scene_cast_rays(teaser_hip_scene* h, const float* rays, int64_t n, float* t_hit, uint32_t* geometry_ids,
                                   uint32_t* primitive_ids, float* primitive_uvs, float* primitive_normals) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (n < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must be >= 0");
  if (n == 0) return TEASER_HIP_OK;
  if (!rays) return fail(h, TEASER_HIP_ERR_BAD_ARG, "rays must not be NULL");
  if (n > 2147483647ll * 128) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n is too large for one call");
  const int32_t rc = build(h);
  if (rc != TEASER_HIP_OK) return rc;
  if (h->built == 0) {
    all_miss((size_t)n, t_hit, geometry_ids, primitive_ids, primitive_uvs, primitive_normals, nullptr);
    return TEASER_HIP_OK;
  }
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  Layout lay;
  SceneRayArgs a;
  memset(&a, 0, sizeof(a));
  a.out.off_t = lay.take(t_hit != nullptr, (size_t)n);
  a.out.off_g = lay.take(geometry_ids || primitive_ids, (size_t)n);
  a.out.off_uv = lay.take(primitive_uvs != nullptr, 2 * (size_t)n);
  a.out.off_n = lay.take(primitive_normals != nullptr, 3 * (size_t)n);
  a.out.off_c = -1;
  const size_t in_bytes = 24 * (size_t)n;
  if (!ensure_io(h, in_bytes, lay.words)) return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (scene ray buffers)");
  memcpy(h->stage.p, rays, in_bytes);
  a.tree = tree_of(h);
  a.rays = h->in.as<float>();
  a.n = n;
  a.buf = h->out.as<uint32_t>();
  const int32_t rq = round_trip(h, in_bytes, lay.words, [&](hipStream_t s) { launch_scene_rays(s, a); });
  if (rq != TEASER_HIP_OK) return rq;
  hand_out(h, h->back.as<uint32_t>(), a.out, (size_t)n, t_hit, geometry_ids, primitive_ids, primitive_uvs, primitive_normals,
           nullptr);
  return TEASER_HIP_OK;
}

int32_t teaser_hip_scene_test_occlusions(teaser_hip_scene* h, const float* rays, int64_t n, double tnear, double tfar,
                                         uint8_t* occluded) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (n < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must be >= 0");
  if (std::isnan(tnear)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "tnear must not be NaN");
  if (std::isnan(tfar)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "tfar must not be NaN");
  if (n == 0) return TEASER_HIP_OK;
  if (!rays) return fail(h, TEASER_HIP_ERR_BAD_ARG, "rays must not be NULL");
  if (!occluded) return fail(h, TEASER_HIP_ERR_BAD_ARG, "occluded must not be NULL");
  if (n > 2147483647ll * 128) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n is too large for one call");
  const int32_t rc = build(h);
  if (rc != TEASER_HIP_OK) return rc;
  if (h->built == 0) {
    memset(occluded, 0, (size_t)n);
    return TEASER_HIP_OK;
  }
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  Layout lay;
  SceneRayArgs a;
  memset(&a, 0, sizeof(a));
  a.out.off_t = lay.take(true, ((size_t)n + 3) / 4);  // bytes, not words
  a.out.off_g = a.out.off_uv = a.out.off_n = a.out.off_c = -1;
  const size_t in_bytes = 24 * (size_t)n;
  if (!ensure_io(h, in_bytes, lay.words)) return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (scene ray buffers)");
  memcpy(h->stage.p, rays, in_bytes);
  a.tree = tree_of(h);
  a.rays = h->in.as<float>();
  a.n = n;
  a.buf = h->out.as<uint32_t>();
  a.tnear = tnear, a.tfar = tfar;
  const int32_t rq = round_trip(h, in_bytes, lay.words, [&](hipStream_t s) { launch_scene_occlusions(s, a); });
  if (rq != TEASER_HIP_OK) return rq;
  memcpy(occluded, h->back.as<uint32_t>() + a.out.off_t, (size_t)n);
  return TEASER_HIP_OK;
}

int32_t teaser_hip_scene_closest_points(teaser_hip_scene* h, const float* points, int64_t n, float* closest, float* distance,
                                        uint32_t* geometry_ids, uint32_t* primitive_ids, float* primitive_uvs,
                                        float* primitive_normals) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (n < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must be >= 0");
  if (n == 0) return TEASER_HIP_OK;
  if (!points) return fail(h, TEASER_HIP_ERR_BAD_ARG, "points must not be NULL");
  if (n > 2147483647ll * 128) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n is too large for one call");
  const int32_t rc = build(h);
  if (rc != TEASER_HIP_OK) return rc;
  if (h->built == 0) {
    all_miss((size_t)n, distance, geometry_ids, primitive_ids, primitive_uvs, primitive_normals, closest);
    return TEASER_HIP_OK;
  }
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  Layout lay;
  ScenePointArgs a;
  memset(&a, 0, sizeof(a));
  a.out.off_t = lay.take(distance != nullptr, (size_t)n);
  a.out.off_g = lay.take(geometry_ids || primitive_ids, (size_t)n);
  a.out.off_uv = lay.take(primitive_uvs != nullptr, 2 * (size_t)n);
  a.out.off_n = lay.take(primitive_normals != nullptr, 3 * (size_t)n);
  a.out.off_c = lay.take(closest != nullptr, 3 * (size_t)n);
  const size_t in_bytes = 12 * (size_t)n;
  if (!ensure_io(h, in_bytes, lay.words)) return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (scene point buffers)");
  memcpy(h->stage.p, points, in_bytes);
  a.tree = tree_of(h);
  a.points = h->in.as<float>();
  a.n = n;
  a.buf = h->out.as<uint32_t>();
  const int32_t rq = round_trip(h, in_bytes, lay.words, [&](hipStream_t s) { launch_scene_points(s, a); });
  if (rq != TEASER_HIP_OK) return rq;
  hand_out(h, h->back.as<uint32_t>(), a.out, (size_t)n, distance, geometry_ids, primitive_ids, primitive_uvs,
           primitive_normals, closest);
  return TEASER_HIP_OK;
}

int32_t teaser_hip_scene_view_default(teaser_scene_view_c* w) {
  if (!w) return TEASER_HIP_ERR_BAD_ARG;
  memset(w, 0, sizeof(*w));
  for (int k = 0; k < 4; ++k) w->extrinsic[5 * k] = 1.0;
  w->pixel_offset = 0.5;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_scene_cast_views(teaser_hip_scene* h, const teaser_scene_view_c* views, int32_t n_views,
                                    float* const* t_hit, uint32_t* const* geometry_ids, uint32_t* const* primitive_ids,
                                    float* const* primitive_uvs, float* const* primitive_normals) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (n_views < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_views must be >= 0");
  if (n_views == 0) return TEASER_HIP_OK;
  if (!views) return fail(h, TEASER_HIP_ERR_BAD_ARG, "views must not be NULL");
  std::vector<SceneView> rec((size_t)n_views);
  Layout lay;
  int64_t n_blocks = 0;
  for (int b = 0; b < n_views; ++b) {
    const teaser_scene_view_c& w = views[b];
    const int32_t rc = check_view(h, b, w);
    if (rc != TEASER_HIP_OK) return rc;
    SceneView& d = rec[(size_t)b];
    memset(&d, 0, sizeof(d));
    const double* E = w.extrinsic;
    d.fx = w.fx, d.fy = w.fy, d.cx = w.cx, d.cy = w.cy, d.pixel_offset = w.pixel_offset;
    for (int k = 0; k < 3; ++k) {
      d.o[k] = (float)-((E[k] * E[3] + E[4 + k] * E[7]) + E[8 + k] * E[11]);
      for (int j = 0; j < 3; ++j) d.E[3 * j + k] = E[4 * j + k];
    }
    d.width = w.width, d.height = w.height;
    d.tiles_x = (w.width + kSceneTile - 1) / kSceneTile;
    const size_t px = (size_t)w.width * (size_t)w.height;
    const int64_t tiles = px ? (int64_t)d.tiles_x * ((w.height + kSceneTile - 1) / kSceneTile) : 0;
    if (n_blocks + tiles > 2147483647)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "the views of one call need more than 2147483647 blocks" + scene_view_at(b));
    d.blk0 = (int32_t)n_blocks;
    n_blocks += tiles;
    d.out.off_t = lay.take(px && entry(t_hit, b), px);
    d.out.off_g = lay.take(px && (entry(geometry_ids, b) || entry(primitive_ids, b)), px);
    d.out.off_uv = lay.take(px && entry(primitive_uvs, b), 2 * px);
    d.out.off_n = lay.take(px && entry(primitive_normals, b), 3 * px);
    d.out.off_c = -1;
  }
  if (n_blocks == 0) return TEASER_HIP_OK;  // no pixel
  const int32_t rc = build(h);
  if (rc != TEASER_HIP_OK) return rc;
  if (h->built == 0) {
    for (int b = 0; b < n_views; ++b)
      all_miss((size_t)views[b].width * (size_t)views[b].height, entry(t_hit, b), entry(geometry_ids, b), entry(primitive_ids, b),
               entry(primitive_uvs, b), entry(primitive_normals, b), nullptr);
    return TEASER_HIP_OK;
  }
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  const size_t o_map = up(sizeof(SceneView) * (size_t)n_views, 256), in_bytes = o_map + 4 * (size_t)n_blocks;
  if (!ensure_io(h, in_bytes, lay.words)) return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (scene view buffers)");
  char* stage = h->stage.as<char>();
  memset(stage, 0, o_map);
  memcpy(stage, rec.data(), sizeof(SceneView) * (size_t)n_views);
  int32_t* map = reinterpret_cast<int32_t*>(stage + o_map);
  for (int b = 0; b < n_views; ++b) {
    const int32_t end = b + 1 < n_views ? rec[(size_t)b + 1].blk0 : (int32_t)n_blocks;
    for (int32_t k = rec[(size_t)b].blk0; k < end; ++k) map[k] = b;
  }
  SceneViewArgs a;
  memset(&a, 0, sizeof(a));
  a.tree = tree_of(h);
  a.views = h->in.as<SceneView>();
  a.blk_view = reinterpret_cast<const int32_t*>(h->in.as<char>() + o_map);
  a.buf = h->out.as<uint32_t>();
  const int32_t rq = round_trip(h, in_bytes, lay.words, [&](hipStream_t s) { launch_scene_views(s, a, (int32_t)n_blocks); });
  if (rq != TEASER_HIP_OK) return rq;
  for (int b = 0; b < n_views; ++b)
    hand_out(h, h->back.as<uint32_t>(), rec[(size_t)b].out, (size_t)views[b].width * (size_t)views[b].height, entry(t_hit, b),
             entry(geometry_ids, b), entry(primitive_ids, b), entry(primitive_uvs, b), entry(primitive_normals, b), nullptr);
  return TEASER_HIP_OK;
}

}  // extern "C"
