// icp_fps_device.h -- the device code of farthest-point down-sampling that does not depend on the launch shape
// (include/teaser_hip.h, "Farthest-point down-sampling"; kernels: kernels_fps.hip, host side: icp_fps.hip, design:
// DESIGN.md section 27): the descriptor of a cloud, the d2 expression, the min update and the combine of two
// (distance, index) candidates.  Nothing here uses a wave operation or LDS, so tests/fps_host_driver.cpp runs this very
// source in serial loops.
//
// Why both routes give the same bits: a round is d[j] = min(d[j], d2(j, cur)) per point, which involves no other point,
// and then the maximum of the (d[j], j) under the TOTAL order "larger d first, then smaller j" (fps_better).  No point
// is NaN (the coordinates are finite; an overflowing difference squares to +inf, and no infinities are subtracted), so
// the order is total, its maximum is unique, and every reduction tree -- a lane's register tile, a wave, sixteen waves,
// the blocks of a launch -- returns that one element.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icp_internal.h"

namespace thip {

constexpr int kFpsResidentThreads = 1024;  // one workgroup per resident cloud
constexpr int kFpsResidentTile = 10;       // points per lane, in registers for the whole loop
static_assert(kFpsResidentCap == kFpsResidentThreads * kFpsResidentTile, "the compiled capacity (icp_internal.h)");
constexpr int kFpsBlock = 256;             // streamed route: threads per block
constexpr int kFpsBlockPoints = 1024;      // and points per block (4 per thread)

// One cloud of a call (host-built, read-only on the device).
struct FpsDesc {
  int32_t n, k;       // points, samples (0 <= k <= n)
  int32_t start;      // the first sample
  int32_t nblk;       // streamed route: ceil(n / kFpsBlockPoints) blocks per round; resident route: 0
  int64_t off;        // first point in the packed points and in final_dist
  int64_t out_off;    // first sample in the packed index and sel_dist
  int32_t blk_off;    // streamed route: first block of the cloud in a round's grid
  int32_t pad;
};

// A candidate of the arg-max: the running distance of point i of its cloud.
struct FpsBest {
  double d;
  int32_t i;
  int32_t pad;
};

// The identity of the combine: below every point (d >= 0 always).
__host__ __device__ inline FpsBest fps_none() { return FpsBest{-1.0, INT32_MAX, 0}; }

// d2 of the contract: ((dx dx + dy dy) + dz dz), differences point minus centre, nothing fused (-ffp-contract=off).
__host__ __device__ inline double fps_d2(double px, double py, double pz, double cx, double cy, double cz) {
  const double dx = px - cx, dy = py - cy, dz = pz - cz;
  return (dx * dx + dy * dy) + dz * dz;
}

// The update of a running distance.
__host__ __device__ inline double fps_min(double d, double v) { return v < d ? v : d; }

// Whether candidate (da, ia) precedes (db, ib): the larger distance, then the smaller index.
__host__ __device__ inline bool fps_better(double da, int32_t ia, double db, int32_t ib) {
  return da > db || (da == db && ia < ib);
}

__host__ __device__ inline FpsBest fps_combine(FpsBest a, FpsBest b) { return fps_better(b.d, b.i, a.d, a.i) ? b : a; }

// The next centre from the winner m of a round (Open3D's max_dist = 0 with its strict >): m, or the centre stays.
__host__ __device__ inline int32_t fps_next(int32_t cur, FpsBest m) { return m.d > 0 ? m.i : cur; }

// ---- launchers (kernels_fps.hip) ------------------------------------------------------------------------------------
// Resident route: block b serves cloud res_map[b] (n <= kFpsResidentCap, k >= 1) with its whole loop.  fin may be NULL.
void launch_fps_resident(hipStream_t s, const FpsDesc* d_desc, const int32_t* d_res_map, int n_res, const double* d_pts,
                         int32_t* d_index, double* d_sel, double* d_fin);
// Streamed route, round r of every streamed cloud: block b serves cloud blk_map[b].  part: 2 x n_blk candidates, the
// halves written in turn; fin holds the running distances between the rounds.
void launch_fps_round(hipStream_t s, const FpsDesc* d_desc, const int32_t* d_blk_map, int n_blk, int round,
                      const double* d_pts, int32_t* d_index, double* d_sel, double* d_fin, FpsBest* d_part);

}  // namespace thip
