// scene_device.h -- the per-item rules of the ray-casting scene (include/teaser_hip.h, "Ray casting scene"; kernels:
// kernels_scene.hip, host side: scene.hip, design, the margins argument and the resource report: DESIGN.md section 41):
// the triangle record, the ray-triangle test, Ericson's closest point, the ray of a view's pixel, the Morton key, one
// node of the radix-tree hierarchy (Karras 2012), the boxes, the two conservative box tests and the stackless
// traversals.  Nothing here uses a wave operation or LDS, so tests/scene_host_driver.cpp runs this very source in serial
// loops.
//
// The library is compiled with -ffp-contract=off: no product-add is fused, and every sum is written out as the
// contract states it.  Pruning decides only which triangles are visited; every number that reaches an output comes from
// scene_ray_tri / scene_point_tri / scene_normal alone.
#pragma once

#include <math.h>
#include <stdint.h>

namespace thip {

constexpr uint32_t kSceneNone = 0xFFFFFFFFu;  // the id of a miss
constexpr int32_t kSceneEnd = -1;             // the rope that leaves the tree
constexpr int32_t kSceneUnset = 2147483647;   // the level of a node whose box has not been formed
constexpr int kSceneBlock = 256;
constexpr int kSceneTile = 16;  // a block of the view launch serves 16 x 16 pixels of one view
constexpr int kSceneMaxBoundsBlocks = 1024;
constexpr int kSceneCounterWords = 64;  // the head of the output buffer: word 0 counts lanes that reached the visit cap
// The margins: a ray tests every box grown by pad = kScenePadRel (|o|_inf + B) on all sides, a
// point prunes a box only when lb (1 - kSceneLbRel) - kSceneLbAbs B^2 exceeds its best d2; B = the largest absolute
// vertex coordinate of the scene.
constexpr double kScenePadRel = 1.0 / 65536.0;               // 2^-16
constexpr double kSceneLbRel = 1.0 / 1073741824.0;           // 2^-30
constexpr double kSceneLbAbs = 1.0 / 1125899906842624.0;     // 2^-50

// A node of the tree: the box of its triangles, `a` = the node index of the left child (an inner node, a >= 0) or ~g
// of its one triangle (a leaf, a < 0), rope = the node a traversal goes to when it is done with this subtree.  The
// right child of an inner node is the rope of its left child.  Inner node i is nodes[i], 0 <= i < n - 1; the leaf of the
// j-th key in sorted order is nodes[n - 1 + j].  The root is nodes[0] (also when n = 1: the only leaf).
struct SceneNode {
  float lo[3], hi[3];
  int32_t a, rope;
};

struct SceneTree {
  const float* tri;        // 9 floats per triangle (v0, v1, v2) in global order
  const SceneNode* nodes;  // 2 n - 1
  const float* bounds;     // lo[3], hi[3] of all vertices, B, 0
  int32_t n;               // triangles
  int32_t pad;
  int64_t cap;             // node visits allowed per traversal (host: 4 n + 64)
};

// Where a call's outputs lie in the output buffer, in 4-byte words; -1: not wanted.
struct SceneOut {
  int64_t off_t, off_g, off_uv, off_n, off_c;  // t_hit or distance; global triangle index; uv; normals; closest points
};

struct SceneView {
  double fx, fy, cx, cy, pixel_offset;
  double E[9];  // E[3 j + k] = extrinsic[j][k], j, k < 3
  float o[3];   // the camera centre
  int32_t width, height, tiles_x, blk0;
  int32_t pad;
  SceneOut out;
};

struct SceneRayArgs {
  SceneTree tree;
  const float* rays;  // n x 6
  int64_t n;
  SceneOut out;
  uint32_t* buf;
  double tnear, tfar;  // the occlusion test alone
};

struct SceneViewArgs {
  SceneTree tree;
  const SceneView* views;
  const int32_t* blk_view;
  uint32_t* buf;
};

struct ScenePointArgs {
  SceneTree tree;
  const float* points;  // n x 3
  int64_t n;
  SceneOut out;
  uint32_t* buf;
};

// What the build passes share (all device memory).
struct SceneBuild {
  const float* tri;
  float* bounds;
  float* partial;  // kSceneMaxBoundsBlocks x 8
  uint64_t* keys[2];
  uint32_t* vals[2];
  SceneNode* nodes;
  int32_t* last;         // inner node i: the last key of its range
  int32_t* rope_target;  // split position gamma: the right child of the node that splits there
  int32_t* level;        // per node: the pass that formed its box (leaves 0)
  int32_t n;
};

// ---- the arithmetic of the contract ----------------------------------------------------------------------------------

__host__ __device__ __forceinline__ void scene_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__host__ __device__ __forceinline__ double scene_dot(const double* a, const double* b) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

struct SceneTri {
  double v0[3], v1[3], v2[3], e1[3], e2[3], n[3];
  bool dead;
};

__host__ __device__ __forceinline__ void scene_load_tri(const float* tri, uint32_t g, SceneTri* T) {
  const float* p = tri + 9 * (size_t)g;
  for (int k = 0; k < 3; ++k) {
    T->v0[k] = (double)p[k], T->v1[k] = (double)p[3 + k], T->v2[k] = (double)p[6 + k];
    T->e1[k] = T->v1[k] - T->v0[k];
    T->e2[k] = T->v2[k] - T->v0[k];
  }
  scene_cross(T->e1, T->e2, T->n);
  T->dead = T->n[0] == 0.0 && T->n[1] == 0.0 && T->n[2] == 0.0;
}

// n / sqrt(n . n), rounded to float32
__host__ __device__ __forceinline__ void scene_normal(const SceneTri& T, float* out) {
  const double len = sqrt(scene_dot(T.n, T.n));
  for (int k = 0; k < 3; ++k) out[k] = (float)(T.n[k] / len);
}

// A ray that takes part: six finite components and a direction that is not (0, 0, 0).
__host__ __device__ __forceinline__ bool scene_ray_valid(const float* r) {
  for (int k = 0; k < 6; ++k)
    if (!(r[k] - r[k] == 0.0f)) return false;  // inf - inf and NaN - NaN are NaN
  return r[3] != 0.0f || r[4] != 0.0f || r[5] != 0.0f;
}

// The ray-triangle test of the contract.
__host__ __device__ __forceinline__ bool scene_ray_tri(const SceneTri& T, const double* o, const double* d, double* t,
                                                       double* u, double* v) {
  if (T.dead) return false;
  double p[3], q[3], s[3];
  scene_cross(d, T.e2, p);
  const double det = scene_dot(T.e1, p);
  if (det == 0.0) return false;
  const double inv = 1.0 / det;
  for (int k = 0; k < 3; ++k) s[k] = o[k] - T.v0[k];
  const double uu = scene_dot(s, p) * inv;
  if (!(uu >= 0.0 && uu <= 1.0)) return false;
  scene_cross(s, T.e1, q);
  const double vv = scene_dot(d, q) * inv;
  if (!(vv >= 0.0 && uu + vv <= 1.0)) return false;
  const double tt = scene_dot(T.e2, q) * inv;
  if (!(tt >= 0.0 && tt < (double)INFINITY)) return false;
  *t = tt, *u = uu, *v = vv;
  return true;
}

// Ericson, Real-Time Collision Detection 5.1.5, ClosestPtPointTriangle, in the order of the book: the closest point c,
// the weights (v, w) of v1 and v2, and d2.  False for a DEAD triangle and for a d2 that is not < +inf.
__host__ __device__ __forceinline__ bool scene_point_tri(const SceneTri& T, const double* p, double* c, double* v,
                                                         double* w, double* d2) {
  if (T.dead) return false;
  const double* a = T.v0;
  const double* b = T.v1;
  const double* cc = T.v2;
  const double* ab = T.e1;
  const double* ac = T.e2;
  double ap[3], bp[3], cp[3];
  double vv = 0.0, ww = 0.0;
  int region = 0;  // 0 A, 1 B, 2 AB, 3 C, 4 AC, 5 BC, 6 face
  for (int k = 0; k < 3; ++k) ap[k] = p[k] - a[k];
  const double d1 = scene_dot(ab, ap), d2_ = scene_dot(ac, ap);
  if (d1 <= 0.0 && d2_ <= 0.0) {
    region = 0;
  } else {
    for (int k = 0; k < 3; ++k) bp[k] = p[k] - b[k];
    const double d3 = scene_dot(ab, bp), d4 = scene_dot(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) {
      region = 1, vv = 1.0;
    } else {
      const double vc = d1 * d4 - d3 * d2_;
      if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        region = 2, vv = d1 / (d1 - d3);
      } else {
        for (int k = 0; k < 3; ++k) cp[k] = p[k] - cc[k];
        const double d5 = scene_dot(ab, cp), d6 = scene_dot(ac, cp);
        if (d6 >= 0.0 && d5 <= d6) {
          region = 3, ww = 1.0;
        } else {
          const double vb = d5 * d2_ - d1 * d6;
          if (vb <= 0.0 && d2_ >= 0.0 && d6 <= 0.0) {
            region = 4, ww = d2_ / (d2_ - d6);
          } else {
            const double va = d3 * d6 - d5 * d4;
            if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
              region = 5, ww = (d4 - d3) / ((d4 - d3) + (d5 - d6)), vv = 1.0 - ww;
            } else {
              const double denom = 1.0 / ((va + vb) + vc);
              region = 6, vv = vb * denom, ww = vc * denom;
            }
          }
        }
      }
    }
  }
  for (int k = 0; k < 3; ++k) {
    switch (region) {
      case 0: c[k] = a[k]; break;
      case 1: c[k] = b[k]; break;
      case 2: c[k] = a[k] + vv * ab[k]; break;
      case 3: c[k] = cc[k]; break;
      case 4: c[k] = a[k] + ww * ac[k]; break;
      case 5: c[k] = b[k] + ww * (cc[k] - b[k]); break;
      default: c[k] = (a[k] + ab[k] * vv) + ac[k] * ww; break;
    }
  }
  const double x = c[0] - p[0], y = c[1] - p[1], z = c[2] - p[2];
  const double dd = (x * x + y * y) + z * z;
  if (!(dd < (double)INFINITY)) return false;
  *v = vv, *w = ww, *d2 = dd;
  return true;
}

// The ray of pixel (row v, column u) of a view, rounded to float32.
__host__ __device__ __forceinline__ void scene_view_ray(const SceneView& w, int v, int u, float* r) {
  const double a = (((double)u + w.pixel_offset) - w.cx) / w.fx;
  const double b = (((double)v + w.pixel_offset) - w.cy) / w.fy;
  for (int k = 0; k < 3; ++k) {
    r[k] = w.o[k];
    r[3 + k] = (float)((w.E[k] * a + w.E[3 + k] * b) + w.E[6 + k]);
  }
}

// The pixel of thread `thread` of the view's tile `tile`: false outside the image.  A wave serves an 8 x 8 quadrant of
// the tile, so that its rays walk the tree together; no bit depends on the mapping.
__host__ __device__ __forceinline__ bool scene_view_pixel(const SceneView& w, int tile, int thread, int* v, int* u) {
  const int ty = tile / w.tiles_x, tx = tile - ty * w.tiles_x;
  const int wave = thread >> 6, lane = thread & 63;
  *u = tx * kSceneTile + ((wave & 1) << 3) + (lane & 7);
  *v = ty * kSceneTile + ((wave >> 1) << 3) + (lane >> 3);
  return *u < w.width && *v < w.height;
}

// ---- the build -------------------------------------------------------------------------------------------------------

// The box of a triangle (exact: minima and maxima of float32 numbers).
__host__ __device__ __forceinline__ void scene_tri_box(const float* tri, uint32_t g, float* lo, float* hi) {
  const float* p = tri + 9 * (size_t)g;
  for (int k = 0; k < 3; ++k) {
    const float a = p[k], b = p[3 + k], c = p[6 + k];
    float m = a < b ? a : b, M = a < b ? b : a;
    m = c < m ? c : m, M = c > M ? c : M;
    lo[k] = m, hi[k] = M;
  }
}

__host__ __device__ __forceinline__ uint64_t scene_spread21(uint64_t x) {  // bit i of x to bit 3 i
  x &= 0x1fffffull;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}

// The 63-bit Morton code of the centroid in the scene's bounds.  It shapes the tree and reaches no output.
__host__ __device__ __forceinline__ uint64_t scene_morton(const float* tri, uint32_t g, const float* bounds) {
  const float* p = tri + 9 * (size_t)g;
  uint64_t code = 0;
  for (int k = 0; k < 3; ++k) {
    const double c = (((double)p[k] + (double)p[3 + k]) + (double)p[6 + k]) / 3.0;
    const double lo = (double)bounds[k], ext = (double)bounds[3 + k] - lo;
    double x = ext > 0.0 ? (c - lo) / ext : 0.0;
    x = x * 2097152.0;
    uint64_t q = x >= 2097151.0 ? 2097151ull : (x > 0.0 ? (uint64_t)x : 0ull);
    code |= scene_spread21(q) << (2 - k);
  }
  return code;
}

__host__ __device__ __forceinline__ int scene_clz64(uint64_t x) {
  int n = 0;
  for (uint64_t bit = 1ull << 63; bit && !(x & bit); bit >>= 1) ++n;
  return n;
}

// The length of the common prefix of keys i and j in sorted order, -1 outside the array.  Equal codes fall back on the
// position, so the key (code, position) is total; the sort is stable over values 0, 1, 2, ..., so the position orders
// equal codes by global triangle index.
__host__ __device__ __forceinline__ int scene_delta(const uint64_t* keys, int32_t n, int64_t i, int64_t j) {
  if (j < 0 || j >= n) return -1;
  const uint64_t x = keys[i] ^ keys[j];
#if defined(__HIP_DEVICE_COMPILE__)
  if (x != 0) return __clzll((long long)x);
  return 64 + __clz((int)((uint32_t)i ^ (uint32_t)j));
#else
  if (x != 0) return scene_clz64(x);
  return 64 + (scene_clz64((uint64_t)((uint32_t)i ^ (uint32_t)j)) - 32);
#endif
}

// Inner node i of the radix tree over the sorted keys (Karras 2012, Algorithm 1 lines 2-25): its range, its split and its
// children.  Writes the left child, the range's end and, at the split, the right child.
__host__ __device__ __forceinline__ void scene_hierarchy_node(const SceneBuild& b, int32_t i) {
  const uint64_t* keys = b.keys[1];
  const int32_t n = b.n;
  const int d = scene_delta(keys, n, i, (int64_t)i + 1) - scene_delta(keys, n, i, (int64_t)i - 1) < 0 ? -1 : 1;
  const int dmin = scene_delta(keys, n, i, (int64_t)i - d);
  int64_t lmax = 2;
  while (scene_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;  // ends: outside the array delta is -1
  int64_t l = 0;
  for (int64_t t = lmax / 2; t >= 1; t /= 2)
    if (scene_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
  const int64_t j = i + l * d;
  const int dnode = scene_delta(keys, n, i, j);
  int64_t s = 0, t = l;
  do {
    t = (t + 1) / 2;
    if (scene_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
  } while (t > 1);
  const int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
  const int64_t first = i < j ? i : j, lastk = i < j ? j : i;
  b.nodes[i].a = (int32_t)(first == gamma ? (n - 1) + gamma : gamma);
  b.rope_target[gamma] = (int32_t)(lastk == gamma + 1 ? (n - 1) + gamma + 1 : gamma + 1);
  b.last[i] = (int32_t)lastk;
}

// After the hierarchy: thread i < n forms leaf i (its triangle, its box, its rope), thread i < n - 1 also the rope of
// inner node i.  The rope of a node whose range ends at key e is the right child of the node that splits at e.
__host__ __device__ __forceinline__ void scene_init_node(const SceneBuild& b, int32_t i) {
  const int32_t n = b.n;
  SceneNode& leaf = b.nodes[n - 1 + i];
  const uint32_t g = b.vals[1][i];
  scene_tri_box(b.tri, g, leaf.lo, leaf.hi);
  leaf.a = ~(int32_t)g;
  leaf.rope = i == n - 1 ? kSceneEnd : b.rope_target[i];
  b.level[n - 1 + i] = 0;
  if (i < n - 1) {
    const int32_t e = b.last[i];
    b.nodes[i].rope = e == n - 1 ? kSceneEnd : b.rope_target[e];
    b.level[i] = kSceneUnset;
  }
}

// Pass p >= 1 of the refit: inner node i forms its box once both children have theirs from an EARLIER pass (a level
// below p; a child formed in this very pass has level p, and a launch boundary lies between its box and this read).
__host__ __device__ __forceinline__ void scene_refit_node(const SceneBuild& b, int32_t i, int32_t p) {
  if (b.level[i] != kSceneUnset) return;
  const int32_t L = b.nodes[i].a, R = b.nodes[L].rope;
  if (!(b.level[L] < p && b.level[R] < p)) return;
  const SceneNode& x = b.nodes[L];
  const SceneNode& y = b.nodes[R];
  for (int k = 0; k < 3; ++k) {
    b.nodes[i].lo[k] = x.lo[k] < y.lo[k] ? x.lo[k] : y.lo[k];
    b.nodes[i].hi[k] = x.hi[k] > y.hi[k] ? x.hi[k] : y.hi[k];
  }
  b.level[i] = p;
}

// ---- the conservative box tests --------------------------------------------------------------------------------------

// The slab test against the box grown by pad: [tmin, tmax] is the computed parameter interval inside, clipped to
// t >= 0.  An axis with d_k == 0 divides nothing: the origin lies between the grown planes or the ray misses.
__host__ __device__ __forceinline__ bool scene_ray_box(const SceneNode& N, const double* o, const double* d,
                                                       const double* inv, double pad, double* tmin_out,
                                                       double* tmax_out) {
  double tmin = 0.0, tmax = (double)INFINITY;
  for (int k = 0; k < 3; ++k) {
    const double lo = (double)N.lo[k] - pad, hi = (double)N.hi[k] + pad;
    if (d[k] != 0.0) {
      double t1 = (lo - o[k]) * inv[k], t2 = (hi - o[k]) * inv[k];
      if (t2 < t1) {
        const double s = t1;
        t1 = t2, t2 = s;
      }
      tmin = t1 > tmin ? t1 : tmin;
      tmax = t2 < tmax ? t2 : tmax;
    } else if (!(o[k] >= lo && o[k] <= hi)) {
      return false;
    }
  }
  *tmin_out = tmin, *tmax_out = tmax;
  return tmin <= tmax;
}

// The computed squared distance from p to the box, less the slack: never above the computed d2 of a triangle inside.
__host__ __device__ __forceinline__ double scene_point_box(const SceneNode& N, const double* p, double abs_slack) {
  double s = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double lo = (double)N.lo[k], hi = (double)N.hi[k];
    const double g = p[k] < lo ? lo - p[k] : (p[k] > hi ? p[k] - hi : 0.0);
    s = s + g * g;
  }
  return s * (1.0 - kSceneLbRel) - abs_slack;
}

// ---- the traversals: one ray or point per lane, no stack -------------------------------------------------------------

struct SceneHit {
  double t, u, v;  // a point: t = d2, (u, v) = the weights
  double c[3];     // a point: the closest point
  uint32_t g;
};

// Closest hit: the minimum of (t, g).  A lane that reaches the visit cap adds 1 to *err.
__host__ __device__ __forceinline__ void scene_trace(const SceneTree& S, const float* ray, SceneHit* h, uint32_t* err) {
  h->t = (double)INFINITY, h->u = 0.0, h->v = 0.0, h->g = kSceneNone;
  if (S.n <= 0 || !scene_ray_valid(ray)) return;
  double o[3], d[3], inv[3];
  double om = 0.0;
  for (int k = 0; k < 3; ++k) {
    o[k] = (double)ray[k], d[k] = (double)ray[3 + k];
    inv[k] = 1.0 / d[k];
    om = fabs(o[k]) > om ? fabs(o[k]) : om;
  }
  const double pad = kScenePadRel * (om + (double)S.bounds[6]);
  int32_t node = 0;
  int64_t visits = 0;
  while (node != kSceneEnd) {
    if (++visits > S.cap) {
      atomicAdd(err, 1u);
      break;
    }
    const SceneNode N = S.nodes[node];
    double tmin, tmax;
    if (scene_ray_box(N, o, d, inv, pad, &tmin, &tmax) && !(tmin > h->t)) {
      if (N.a >= 0) {
        node = N.a;
        continue;
      }
      const uint32_t g = (uint32_t)~N.a;
      SceneTri T;
      scene_load_tri(S.tri, g, &T);
      double t, u, v;
      if (scene_ray_tri(T, o, d, &t, &u, &v) && (t < h->t || (t == h->t && g < h->g))) h->t = t, h->u = u, h->v = v, h->g = g;
    }
    node = N.rope;
  }
}

// Any hit with tnear <= t <= tfar.
__host__ __device__ __forceinline__ bool scene_occluded(const SceneTree& S, const float* ray, double tnear, double tfar,
                                                        uint32_t* err) {
  if (S.n <= 0 || !scene_ray_valid(ray)) return false;
  double o[3], d[3], inv[3];
  double om = 0.0;
  for (int k = 0; k < 3; ++k) {
    o[k] = (double)ray[k], d[k] = (double)ray[3 + k];
    inv[k] = 1.0 / d[k];
    om = fabs(o[k]) > om ? fabs(o[k]) : om;
  }
  const double pad = kScenePadRel * (om + (double)S.bounds[6]);
  int32_t node = 0;
  int64_t visits = 0;
  while (node != kSceneEnd) {
    if (++visits > S.cap) {
      atomicAdd(err, 1u);
      break;
    }
    const SceneNode N = S.nodes[node];
    double tmin, tmax;
    if (scene_ray_box(N, o, d, inv, pad, &tmin, &tmax) && !(tmin > tfar) && !(tmax < tnear)) {
      if (N.a >= 0) {
        node = N.a;
        continue;
      }
      SceneTri T;
      scene_load_tri(S.tri, (uint32_t)~N.a, &T);
      double t, u, v;
      if (scene_ray_tri(T, o, d, &t, &u, &v) && tnear <= t && t <= tfar) return true;
    }
    node = N.rope;
  }
  return false;
}

__host__ __device__ __forceinline__ void scene_point_visit(const SceneTree& S, uint32_t g, const double* p, SceneHit* h) {
  SceneTri T;
  scene_load_tri(S.tri, g, &T);
  double c[3], v, w, d2;
  if (scene_point_tri(T, p, c, &v, &w, &d2) && (d2 < h->t || (d2 == h->t && g < h->g))) {
    h->t = d2, h->u = v, h->v = w, h->g = g;
    for (int k = 0; k < 3; ++k) h->c[k] = c[k];
  }
}

// Closest point: the minimum of (d2, g).  A descent towards the nearer child seeds the best d2 with a real triangle;
// the sweep then visits every node whose bound does not exceed it (the seed again among them, which changes nothing).
__host__ __device__ __forceinline__ void scene_closest(const SceneTree& S, const float* point, SceneHit* h, uint32_t* err) {
  h->t = (double)INFINITY, h->u = 0.0, h->v = 0.0, h->g = kSceneNone;
  h->c[0] = h->c[1] = h->c[2] = 0.0;
  if (S.n <= 0) return;
  double p[3];
  for (int k = 0; k < 3; ++k) {
    if (!(point[k] - point[k] == 0.0f)) return;  // a point with a non-finite component has no closest point
    p[k] = (double)point[k];
  }
  const double B = (double)S.bounds[6];
  const double slack = kSceneLbAbs * (B * B);
  int32_t node = 0;
  int64_t visits = 0;
  for (;;) {
    if (++visits > S.cap) {
      atomicAdd(err, 1u);
      return;
    }
    const int32_t a = S.nodes[node].a;
    if (a < 0) {
      scene_point_visit(S, (uint32_t)~a, p, h);
      break;
    }
    const int32_t r = S.nodes[a].rope;
    node = scene_point_box(S.nodes[r], p, slack) < scene_point_box(S.nodes[a], p, slack) ? r : a;
  }
  node = 0;
  while (node != kSceneEnd) {
    if (++visits > S.cap) {
      atomicAdd(err, 1u);
      break;
    }
    const SceneNode N = S.nodes[node];
    if (!(scene_point_box(N, p, slack) > h->t)) {
      if (N.a >= 0) {
        node = N.a;
        continue;
      }
      scene_point_visit(S, (uint32_t)~N.a, p, h);
    }
    node = N.rope;
  }
}

// ---- the outputs -----------------------------------------------------------------------------------------------------

__host__ __device__ __forceinline__ uint32_t scene_bits(float f) {
  union {
    float f;
    uint32_t u;
  } x;
  x.f = f;
  return x.u;
}

// Item idx of a ray call or of a view: t_hit, the global index, uv, the normal; a miss is +inf, kSceneNone, 0, 0.
__host__ __device__ __forceinline__ void scene_store_ray(const SceneTree& S, uint32_t* buf, const SceneOut& o, int64_t idx,
                                                         const SceneHit& h) {
  const bool hit = h.g != kSceneNone;
  if (o.off_t >= 0) buf[o.off_t + idx] = scene_bits(hit ? (float)h.t : INFINITY);
  if (o.off_g >= 0) buf[o.off_g + idx] = h.g;
  if (o.off_uv >= 0) {
    buf[o.off_uv + 2 * idx] = scene_bits(hit ? (float)h.u : 0.0f);
    buf[o.off_uv + 2 * idx + 1] = scene_bits(hit ? (float)h.v : 0.0f);
  }
  if (o.off_n >= 0) {
    float nrm[3] = {0.0f, 0.0f, 0.0f};
    if (hit) {
      SceneTri T;
      scene_load_tri(S.tri, h.g, &T);
      scene_normal(T, nrm);
    }
    for (int k = 0; k < 3; ++k) buf[o.off_n + 3 * idx + k] = scene_bits(nrm[k]);
  }
}

// Item idx of a closest-point call: the distance (float)sqrt(d2), the closest point and the maps of a ray call.
__host__ __device__ __forceinline__ void scene_store_point(const SceneTree& S, uint32_t* buf, const SceneOut& o, int64_t idx,
                                                           const SceneHit& h) {
  SceneHit r = h;
  const bool hit = h.g != kSceneNone;
  r.t = hit ? sqrt(h.t) : (double)INFINITY;
  scene_store_ray(S, buf, o, idx, r);
  if (o.off_c >= 0)
    for (int k = 0; k < 3; ++k) buf[o.off_c + 3 * idx + k] = scene_bits(hit ? (float)h.c[k] : 0.0f);
}

// ---- one thread of each launch ---------------------------------------------------------------------------------------

__host__ __device__ __forceinline__ void scene_ray_thread(const SceneRayArgs& a, int64_t i) {
  if (i >= a.n) return;
  SceneHit h;
  scene_trace(a.tree, a.rays + 6 * i, &h, a.buf);
  scene_store_ray(a.tree, a.buf, a.out, i, h);
}

__host__ __device__ __forceinline__ void scene_occlusion_thread(const SceneRayArgs& a, int64_t i) {
  if (i >= a.n) return;
  const bool occ = scene_occluded(a.tree, a.rays + 6 * i, a.tnear, a.tfar, a.buf);
  reinterpret_cast<uint8_t*>(a.buf + a.out.off_t)[i] = occ ? 1 : 0;
}

__host__ __device__ __forceinline__ void scene_point_thread(const ScenePointArgs& a, int64_t i) {
  if (i >= a.n) return;
  SceneHit h;
  scene_closest(a.tree, a.points + 3 * i, &h, a.buf);
  scene_store_point(a.tree, a.buf, a.out, i, h);
}

__host__ __device__ __forceinline__ void scene_view_thread(const SceneViewArgs& a, int block, int thread) {
  const int b = a.blk_view[block];
  const SceneView& w = a.views[b];
  int v, u;
  if (!scene_view_pixel(w, block - w.blk0, thread, &v, &u)) return;
  float ray[6];
  scene_view_ray(w, v, u, ray);
  SceneHit h;
  scene_trace(a.tree, ray, &h, a.buf);
  scene_store_ray(a.tree, a.buf, w.out, (int64_t)v * w.width + u, h);
}

}  // namespace thip
