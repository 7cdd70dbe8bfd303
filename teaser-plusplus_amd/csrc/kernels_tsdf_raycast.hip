// kernels_tsdf_raycast.hip -- the ray cast of the TSDF volume for gfx950 (include/teaser_hip.h, "TSDF ray casting";
// device code: tsdf_raycast_device.h; host side: tsdf_raycast.hip; design, bounds and the resource report: DESIGN.md
// section 35).
//
// One launch serves all pixels of all views of a call: a block is 16 x 16 pixels of one view, the block map names the
// view of every block and the view's record says where its blocks begin and where its maps lie.  A thread is a ray.  A
// wave takes an 8 x 8 quadrant of the tile (tsdf_ray_pixel), not a 64 x 1 row: its rays then sample voxels that are
// neighbours along all three axes of the (z R + x) R + y layout at every step, so the two loads of a step (tsdf, weight)
// fall into few lines.  The march diverges in its trip count only; the maps of a hit -- the 48 loads of a normal, the
// corners of a colour -- are formed after the loop by the hit lanes alone.  The block's number of hits is counted with a
// barrier and written by one thread: the host adds the blocks of a view, so there is no atomic of any kind.
#include "tsdf_raycast_device.h"

namespace thip {

__global__ __launch_bounds__(kTsdfRayBlock) void tsdf_raycast_kernel(const TsdfGrid g, const TsdfFields v,
                                                                     const TsdfRayArgs a) {
  const bool hit = tsdf_ray_thread(g, v, a, (int)blockIdx.x, (int)threadIdx.x);
  const int hits = __syncthreads_count(hit);  // every thread of the block arrives: tsdf_ray_thread returns, never exits
  if (threadIdx.x == 0) a.blk_hits[blockIdx.x] = hits;
}

void launch_tsdf_raycast(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, const TsdfRayArgs& a, int32_t n_blocks) {
  hipLaunchKernelGGL(tsdf_raycast_kernel, dim3((unsigned)n_blocks), dim3(kTsdfRayBlock), 0, s, g, v, a);
}

}  // namespace thip
