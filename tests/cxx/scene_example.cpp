// teaser::RaycastingScene (include/teaser/scene.h) used like Open3D's RaycastingScene on the 9 x 9 lattice sheet of
// tests/scene_reference.py: rays through the lattice vertices and oblique ones, closest points, an occlusion test and a
// view that must equal castRays on createRaysPinhole.  The record printed -- counts and FNV-1a hashes of the bytes of
// every array -- is what tests/test_gpu_scene_cxx.py compares with the Python calls'.
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cstdio>
#include <cstring>
#include <vector>

#include "teaser/scene.h"

static int fail(const char* what) {
  std::fprintf(stderr, "scene_example: %s\n", what);
  return 1;
}

static unsigned long long fnv(const void* p, size_t bytes) {
  unsigned long long h = 1469598103934665603ull;
  const unsigned char* b = (const unsigned char*)p;
  for (size_t k = 0; k < bytes; ++k) h = (h ^ b[k]) * 1099511628211ull;
  return h;
}
template <class T>
static unsigned long long fnv(const std::vector<T>& v) { return fnv(v.data(), sizeof(T) * v.size()); }

int main() {
  try {
    const int n = 9;
    std::vector<float> vert;
    std::vector<uint32_t> tri;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) vert.insert(vert.end(), {(float)i, (float)j, 0.0f});
    for (int i = 0; i + 1 < n; ++i)
      for (int j = 0; j + 1 < n; ++j) {
        const uint32_t a = (uint32_t)(i * n + j), b = (uint32_t)((i + 1) * n + j), c = b + 1, d = a + 1;
        tri.insert(tri.end(), {a, b, c, a, c, d});
      }
    std::vector<float> rays, pts;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        rays.insert(rays.end(), {(float)i, (float)j, 5.0f, 0.0f, 0.0f, -1.0f});
        rays.insert(rays.end(), {(float)i - 2.0f, (float)j + 0.25f, 3.0f, 0.5f, 0.125f, -1.0f});
        pts.insert(pts.end(), {(float)i + 0.5f, (float)j * 1.25f - 1.0f, (float)(i - j) * 0.5f});
      }
    teaser::RaycastingScene scene;
    if (scene.triangleCount() != 0 || scene.castRays(rays).t_hit[0] != std::numeric_limits<float>::infinity())
      return fail("an empty scene shows nothing");
    if (scene.addTriangles(vert, tri) != 0 || scene.triangleCount() != 128) return fail("addTriangles");
    const teaser::SceneRayResult hit = scene.castRays(rays);
    if (hit.t_hit[0] != 5.0f || hit.primitive_ids[0] != 0 || hit.geometry_ids[0] != 0) return fail("the first ray meets triangle 0 at t = 5");
    const std::vector<uint8_t> occ = scene.testOcclusions(rays, 5.0, 5.0);
    const teaser::SceneClosestResult near = scene.computeClosestPoints(pts);
    if (scene.computeDistance(pts) != near.distance) return fail("computeDistance");
    const teaser::PinholeCameraIntrinsic K(17, 9, 12.0, 12.0, 8.0, 4.0);
    teaser::Matrix4 E = teaser::Matrix4::Identity();
    E(0, 3) = -4.0, E(1, 3) = 3.0, E(2, 3) = 6.0;
    E(1, 1) = -1.0, E(2, 2) = -1.0;  // looks down on the sheet from z = 6
    const teaser::SceneRayResult view = scene.castViews(K, {E}, 0.5)[0];
    const teaser::SceneRayResult same = scene.castRays(teaser::RaycastingScene::createRaysPinhole(K, E, 0.5));
    if (view.t_hit != same.t_hit || view.primitive_ids != same.primitive_ids || view.primitive_uvs != same.primitive_uvs ||
        view.primitive_normals != same.primitive_normals || view.geometry_ids != same.geometry_ids)
      return fail("castViews equals castRays on createRaysPinhole");
    int64_t hits = 0, occluded = 0;
    for (float t : hit.t_hit) hits += t < std::numeric_limits<float>::infinity();
    for (uint8_t o : occ) occluded += o;
    std::printf("hits %lld\noccluded %lld\n", (long long)hits, (long long)occluded);
    std::printf("t_bits %016llx\ngeometry_bits %016llx\nprimitive_bits %016llx\nuv_bits %016llx\nnormal_bits %016llx\n", fnv(hit.t_hit), fnv(hit.geometry_ids),
                fnv(hit.primitive_ids), fnv(hit.primitive_uvs), fnv(hit.primitive_normals));
    std::printf("closest_bits %016llx\ndistance_bits %016llx\nclosest_primitive_bits %016llx\nclosest_uv_bits %016llx\n", fnv(near.points), fnv(near.distance),
                fnv(near.primitive_ids), fnv(near.primitive_uvs));
    std::printf("view_t_bits %016llx\nview_normal_bits %016llx\nchecks 1\n", fnv(view.t_hit), fnv(view.primitive_normals));
    return 0;
  } catch (const teaser::SceneError& e) {
    std::fprintf(stderr, "scene_example: %s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  }
}
