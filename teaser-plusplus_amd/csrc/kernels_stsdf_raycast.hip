// kernels_stsdf_raycast.hip -- the ray cast of the scalable TSDF volume for gfx950 (include/teaser_hip.h, "Scalable
// TSDF ray casting"; device code: stsdf_raycast_device.h; host side: stsdf_raycast.hip; design, bounds and the resource
// report: DESIGN.md section 38).
//
// The launch shape is the dense ray cast's (kernels_tsdf_raycast.hip): one launch over all pixels of all views, a block
// is 16 x 16 pixels of one view, a thread is a ray and a wave takes an 8 x 8 quadrant of the tile, so that its rays cross
// the same few blocks of 16^3 voxels at a step and their samples (tsdf at `at`, weight 16 KiB behind it) fall into few
// lines.  What is new is where a sample lies: the directory of open blocks is a sorted array of keys, searched by
// bisection -- about log2(blocks) dependent 8-byte loads -- so a lane keeps the block it looked up last and searches
// again only when its ray has left it; in a block that is not open the ray jumps to the block's exit face.  The march
// diverges in its trip count and in the searches; the maps of a hit are formed after the loop by the hit lanes alone.
// The block's number of hits is counted with a barrier and written by one thread: the host adds the blocks of a view, so
// there is no atomic of any kind.
#include "stsdf_raycast_device.h"

namespace thip {

__global__ __launch_bounds__(kTsdfRayBlock) void stsdf_raycast_kernel(const TsdfGrid g, const StsdfDir dir,
                                                                      const StsdfRayArgs a) {
  const bool hit = stsdf_ray_thread(g, dir, a, (int)blockIdx.x, (int)threadIdx.x);
  const int hits = __syncthreads_count(hit);  // every thread of the block arrives: stsdf_ray_thread returns, never exits
  if (threadIdx.x == 0) a.blk_hits[blockIdx.x] = hits;
}

void launch_stsdf_raycast(hipStream_t s, const TsdfGrid& g, const StsdfDir& dir, const StsdfRayArgs& a, int32_t n_blocks) {
  hipLaunchKernelGGL(stsdf_raycast_kernel, dim3((unsigned)n_blocks), dim3(kTsdfRayBlock), 0, s, g, dir, a);
}

}  // namespace thip
