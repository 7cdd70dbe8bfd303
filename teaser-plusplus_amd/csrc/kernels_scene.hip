// kernels_scene.hip -- the ray-casting scene for gfx950 (include/teaser_hip.h, "Ray casting scene"; device code:
// scene_device.h; host side: scene.hip; design, the margins argument, bounds and the resource report: DESIGN.md section
// 40).
//
// The build, all on the device and on the handle's stream:
//   bounds     two launches: the blocks' minima, maxima and largest absolute coordinate over a grid-stride sweep of the
//              triangles (LDS tree), then one block over the blocks' partials.  Minima and maxima do not depend on the
//              order, so there is no atomic;
//   morton     63-bit Morton code of every centroid and the values 0, 1, 2, ... beside it;
//   sort       rocprim's stable LSD radix sort of (code, g): equal codes stay in index order, so the key is total;
//   hierarchy  ONE launch, a thread per inner node (Karras 2012);
//   init       leaves, ropes, levels;
//   refit      bottom-up in passes: a node forms its box from children that had theirs before the launch.  A launch
//              boundary lies between every box and its reader, so no fence, no flag and no atomic carries data between
//              workgroups.  The height is at most 63 + bits(n - 1) (scene.hip), which is the number of passes.
// The traversals are one ray or point per lane and keep no stack: a node's rope names where to go on after its subtree,
// so a lane holds a node index and its best hit, all in registers.  A wave's lanes run the loop together and diverge
// only in which of them skip a node.  The visit cap comes from the host; a lane that reaches it counts itself in word 0
// of the output buffer (an integer atomic, the only one) and the call fails.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "scene_device.h"

namespace thip {

__device__ __forceinline__ void bounds_merge(float* a, const float* b) {
  for (int k = 0; k < 3; ++k) {
    a[k] = b[k] < a[k] ? b[k] : a[k];
    a[3 + k] = b[3 + k] > a[3 + k] ? b[3 + k] : a[3 + k];
  }
  a[6] = b[6] > a[6] ? b[6] : a[6];
}

// The block's record to out[0 .. 7]: every thread brings its own in r.
__device__ __forceinline__ void bounds_block(float* r, float* out) {
  __shared__ float sh[kSceneBlock][8];
  for (int k = 0; k < 7; ++k) sh[threadIdx.x][k] = r[k];
  __syncthreads();
  for (int o = kSceneBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) bounds_merge(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x < 8) out[threadIdx.x] = threadIdx.x < 7 ? sh[0][threadIdx.x] : 0.0f;
}

__device__ __forceinline__ void bounds_empty(float* r) {
  for (int k = 0; k < 3; ++k) r[k] = INFINITY, r[3 + k] = -INFINITY;
  r[6] = 0.0f;
}

__global__ __launch_bounds__(kSceneBlock) void scene_bounds_partial_kernel(const SceneBuild b) {
  float r[7];
  bounds_empty(r);
  for (int64_t g = (int64_t)blockIdx.x * kSceneBlock + threadIdx.x; g < b.n; g += (int64_t)gridDim.x * kSceneBlock) {
    float t[7];
    scene_tri_box(b.tri, (uint32_t)g, t, t + 3);
    t[6] = 0.0f;
    for (int k = 0; k < 6; ++k) t[6] = fabsf(t[k]) > t[6] ? fabsf(t[k]) : t[6];
    bounds_merge(r, t);
  }
  bounds_block(r, b.partial + 8 * (size_t)blockIdx.x);
}

__global__ __launch_bounds__(kSceneBlock) void scene_bounds_final_kernel(const SceneBuild b, const int blocks) {
  float r[7];
  bounds_empty(r);
  for (int k = threadIdx.x; k < blocks; k += kSceneBlock) bounds_merge(r, b.partial + 8 * (size_t)k);
  bounds_block(r, b.bounds);
}

__global__ __launch_bounds__(kSceneBlock) void scene_morton_kernel(const SceneBuild b) {
  const int64_t g = (int64_t)blockIdx.x * kSceneBlock + threadIdx.x;
  if (g >= b.n) return;
  b.keys[0][g] = scene_morton(b.tri, (uint32_t)g, b.bounds);
  b.vals[0][g] = (uint32_t)g;
}

__global__ __launch_bounds__(kSceneBlock) void scene_hierarchy_kernel(const SceneBuild b) {
  const int64_t i = (int64_t)blockIdx.x * kSceneBlock + threadIdx.x;
  if (i < b.n - 1) scene_hierarchy_node(b, (int32_t)i);
}

__global__ __launch_bounds__(kSceneBlock) void scene_init_kernel(const SceneBuild b) {
  const int64_t i = (int64_t)blockIdx.x * kSceneBlock + threadIdx.x;
  if (i < b.n) scene_init_node(b, (int32_t)i);
}

__global__ __launch_bounds__(kSceneBlock) void scene_refit_kernel(const SceneBuild b, const int32_t pass) {
  const int64_t i = (int64_t)blockIdx.x * kSceneBlock + threadIdx.x;
  if (i < b.n - 1) scene_refit_node(b, (int32_t)i, pass);
}

__global__ __launch_bounds__(kSceneBlock) void scene_rays_kernel(const SceneRayArgs a) {
  scene_ray_thread(a, (int64_t)blockIdx.x * kSceneBlock + threadIdx.x);
}

__global__ __launch_bounds__(kSceneBlock) void scene_occlusion_kernel(const SceneRayArgs a) {
  scene_occlusion_thread(a, (int64_t)blockIdx.x * kSceneBlock + threadIdx.x);
}

__global__ __launch_bounds__(kSceneBlock) void scene_points_kernel(const ScenePointArgs a) {
  scene_point_thread(a, (int64_t)blockIdx.x * kSceneBlock + threadIdx.x);
}

__global__ __launch_bounds__(kSceneBlock) void scene_views_kernel(const SceneViewArgs a) {
  scene_view_thread(a, (int)blockIdx.x, (int)threadIdx.x);
}

static unsigned blocks_of(int64_t n) { return (unsigned)((n + kSceneBlock - 1) / kSceneBlock); }

size_t scene_sort_temp_bytes(int64_t n) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (size_t)n, 0, 63, (hipStream_t)0);
  return bytes;
}

// bounds, the keys (keys[0], vals[0]) and their sorted order (keys[1], vals[1]).  n >= 1.
hipError_t launch_scene_keys(hipStream_t s, const SceneBuild& b, void* d_temp, size_t temp_bytes) {
  const int blocks = (int)std::min<int64_t>(blocks_of(b.n), kSceneMaxBoundsBlocks);
  hipLaunchKernelGGL(scene_bounds_partial_kernel, dim3((unsigned)blocks), dim3(kSceneBlock), 0, s, b);
  hipLaunchKernelGGL(scene_bounds_final_kernel, dim3(1), dim3(kSceneBlock), 0, s, b, blocks);
  hipLaunchKernelGGL(scene_morton_kernel, dim3(blocks_of(b.n)), dim3(kSceneBlock), 0, s, b);
  size_t tb = temp_bytes;
  return rocprim::radix_sort_pairs(d_temp, tb, (const uint64_t*)b.keys[0], b.keys[1], (const uint32_t*)b.vals[0], b.vals[1],
                                   (size_t)b.n, 0, 63, s);
}

// The hierarchy in one launch, the leaves and ropes, and `passes` refit passes.  n >= 1.
void launch_scene_tree(hipStream_t s, const SceneBuild& b, int passes) {
  if (b.n > 1) hipLaunchKernelGGL(scene_hierarchy_kernel, dim3(blocks_of(b.n - 1)), dim3(kSceneBlock), 0, s, b);
  hipLaunchKernelGGL(scene_init_kernel, dim3(blocks_of(b.n)), dim3(kSceneBlock), 0, s, b);
  for (int p = 1; p <= passes && b.n > 1; ++p)
    hipLaunchKernelGGL(scene_refit_kernel, dim3(blocks_of(b.n - 1)), dim3(kSceneBlock), 0, s, b, (int32_t)p);
}

void launch_scene_rays(hipStream_t s, const SceneRayArgs& a) {
  hipLaunchKernelGGL(scene_rays_kernel, dim3(blocks_of(a.n)), dim3(kSceneBlock), 0, s, a);
}
void launch_scene_occlusions(hipStream_t s, const SceneRayArgs& a) {
  hipLaunchKernelGGL(scene_occlusion_kernel, dim3(blocks_of(a.n)), dim3(kSceneBlock), 0, s, a);
}
void launch_scene_points(hipStream_t s, const ScenePointArgs& a) {
  hipLaunchKernelGGL(scene_points_kernel, dim3(blocks_of(a.n)), dim3(kSceneBlock), 0, s, a);
}
void launch_scene_views(hipStream_t s, const SceneViewArgs& a, int32_t n_blocks) {
  hipLaunchKernelGGL(scene_views_kernel, dim3((unsigned)n_blocks), dim3(kSceneBlock), 0, s, a);
}

}  // namespace thip
