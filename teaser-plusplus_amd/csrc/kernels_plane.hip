// kernels_plane.hip -- the kernels of RANSAC plane segmentation (contract: include/teaser_hip.h, "Plane segmentation";
// design: DESIGN.md section 25).  FP64 throughout, -ffp-contract=off, no floating-point atomics and no atomics at all:
// every partial is stored by (block, trial) or (group, trial) and combined in the contract's order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "plane_device.h"

namespace thip {

// Model: one lane per trial of the chunk.  The plane, the flag and a zero score go out by trial index.
__global__ void __launch_bounds__(PL_BLOCK) plane_model_kernel(const PlDesc* __restrict__ desc,
                                                               const double* __restrict__ pts, PlSlot slot, int chunk,
                                                               int64_t first) {
  const int b = blockIdx.y;
  const int n = slot.n[b];
  const int t = blockIdx.x * PL_BLOCK + threadIdx.x;
  if (t >= n) return;
  const PlDesc D = desc[b];
  const int64_t at = (int64_t)b * chunk + t;
  int32_t smp[PL_MAX_N];
  double w[4] = {0.0, 0.0, 0.0, 0.0};
  int flags = 0;
  if (D.run) flags = pl_model(D, pts + 3 * D.pt_off, first + t, smp, w);
  for (int k = 0; k < 4; ++k) slot.model[4 * at + k] = w[k];
  slot.flags[at] = (uint8_t)flags;
  slot.count[at] = 0;
  slot.E[at] = 0.0;
  if (slot.samples)
    for (int k = 0; k < PL_MAX_N; ++k) slot.samples[PL_MAX_N * at + k] = D.run ? smp[k] : -1;
}

// Score, the hot path: grid (four point blocks, tile of 64 hypotheses, problem).  A lane owns one hypothesis with its
// four coefficients in registers; each of the four waves stages ONE block of 256 points in LDS and walks it in index
// order, every lane reading the same address (a broadcast): the four waves share the tile's hypotheses and differ in
// the block.  (count, block sum) go out by (block, trial).
__global__ void __launch_bounds__(PL_BLOCK) plane_score_kernel(const PlDesc* __restrict__ desc,
                                                               const double* __restrict__ pts, PlSlot slot, PlPart part,
                                                               int chunk, int g0) {
  __shared__ double xyz[PL_WAVES][3 * PL_BLOCK];
  const int b = blockIdx.z;
  const int nt = slot.n[b];
  if ((int)(blockIdx.y * PL_TILE) >= nt) return;  // uniform
  const PlDesc D = desc[b];
  const int64_t nblk = pl_blocks(D.n);
  const int64_t blk0 = (int64_t)g0 * PL_GROUP + (int64_t)blockIdx.x * PL_WAVES;
  if (blk0 >= nblk) return;  // uniform
  const int wave = threadIdx.x / PL_TILE, lane = threadIdx.x % PL_TILE;
  const int64_t blk = blk0 + wave;
  const int m = blk < nblk ? (int)min((int64_t)PL_BLOCK, (int64_t)D.n - blk * PL_BLOCK) : 0;
  const double* P = pts + 3 * (D.pt_off + blk * PL_BLOCK);
  for (int k = lane; k < 3 * m; k += PL_TILE) xyz[wave][k] = P[k];
  __syncthreads();
  const int t = blockIdx.y * PL_TILE + lane;
  if (m == 0 || t >= nt) return;
  const int64_t at = (int64_t)b * chunk + t;
  const bool live = (slot.flags[at] & PL_FLAG_VALID) != 0;
  double w[4];
  for (int k = 0; k < 4; ++k) w[k] = slot.model[4 * at + k];
  int32_t cnt;
  double bs;
  pl_score_block(w, D.d, xyz[wave], m, &cnt, &bs);
  const int64_t slot_blk = (D.part_grp + (blk / PL_GROUP - g0)) * PL_GROUP + blk % PL_GROUP;
  part.bcnt[slot_blk * chunk + t] = live ? cnt : 0;
  part.bsum[slot_blk * chunk + t] = live ? bs : 0.0;
}

// Groups: a lane per (trial, group of the wave, problem) adds the group's block sums in block order from 0.
__global__ void __launch_bounds__(PL_BLOCK) plane_group_kernel(const PlDesc* __restrict__ desc, PlSlot slot, PlPart part,
                                                               int chunk, int g0) {
  const int b = blockIdx.z;
  const int t = blockIdx.x * PL_BLOCK + threadIdx.x;
  if (t >= slot.n[b]) return;
  const PlDesc D = desc[b];
  const int64_t nblk = pl_blocks(D.n);
  const int64_t g = (int64_t)g0 + blockIdx.y;
  if (g * PL_GROUP >= nblk) return;
  const int kb = (int)min((int64_t)PL_GROUP, nblk - g * PL_GROUP);
  const int64_t gs = D.part_grp + blockIdx.y;
  int32_t c = 0;
  double s = 0.0;
  for (int k = 0; k < kb; ++k) {
    c += part.bcnt[(gs * PL_GROUP + k) * chunk + t];
    s += part.bsum[(gs * PL_GROUP + k) * chunk + t];
  }
  part.gcnt[gs * chunk + t] = c;
  part.gsum[gs * chunk + t] = s;
}

// Total: a lane per (trial, problem) adds the wave's group sums, in group order, onto what the earlier waves left.
__global__ void __launch_bounds__(PL_BLOCK) plane_total_kernel(const PlDesc* __restrict__ desc, PlSlot slot, PlPart part,
                                                               int chunk, int g0, int W) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * PL_BLOCK + threadIdx.x;
  if (t >= slot.n[b]) return;
  const PlDesc D = desc[b];
  const int64_t ng = pl_groups(D.n);
  const int kg = (int)min((int64_t)W, ng - g0);
  if (kg <= 0) return;
  const int64_t at = (int64_t)b * chunk + t;
  int32_t c = slot.count[at];
  double s = slot.E[at];
  for (int k = 0; k < kg; ++k) {
    c += part.gcnt[(D.part_grp + k) * chunk + t];
    s += part.gsum[(D.part_grp + k) * chunk + t];
  }
  slot.count[at] = c;
  slot.E[at] = s;
}

// Finish.  Winner: a lane per problem recomputes the winning trial's plane (the same one-lane function, the same bits).
__global__ void __launch_bounds__(PL_TILE) plane_winner_kernel(const PlDesc* __restrict__ desc,
                                                               const double* __restrict__ pts, PlFin fin, int batch) {
  const int b = blockIdx.x * PL_TILE + threadIdx.x;
  if (b >= batch) return;
  const PlDesc D = desc[b];
  double w[4] = {0.0, 0.0, 0.0, 0.0};
  int32_t smp[PL_MAX_N];
  if (D.run && fin.best[b] >= 0) pl_model(D, pts + 3 * D.pt_off, fin.best[b], smp, w);
  for (int k = 0; k < 4; ++k) fin.win[4 * b + k] = w[k];
}

// Blocks of the finish: a lane per block of 256 positions walks it in index order.  PASS 0: the mask and the three
// coordinate sums; PASS 1: the six product sums of the centred inliers.
template <int PASS>
__global__ void __launch_bounds__(PL_BLOCK) plane_fin_block_kernel(const PlDesc* __restrict__ desc,
                                                                   const double* __restrict__ pts, PlFin fin) {
  const int b = blockIdx.y;
  const PlDesc D = desc[b];
  const int64_t blk = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x;
  if (blk >= pl_blocks(D.n)) return;
  const int m = (int)min((int64_t)PL_BLOCK, (int64_t)D.n - blk * PL_BLOCK);
  const int64_t p0 = D.pt_off + blk * PL_BLOCK;
  double S[6];
  if (PASS == 0) {
    int32_t c;
    pl_fin_block_mask(fin.best[b] >= 0, fin.win + 4 * b, D.d, pts + 3 * p0, m, fin.mask + p0, &c, S);
    fin.bcnt[D.blk_off + blk] = c;
  } else {
    pl_fin_block_cov(fin.centroid + 3 * b, pts + 3 * p0, m, fin.mask + p0, S);
  }
  for (int k = 0; k < 6; ++k) fin.bsum[6 * (D.blk_off + blk) + k] = S[k];
}

// Groups of the finish: a lane per group adds its block sums in block order from 0.
__global__ void __launch_bounds__(PL_BLOCK) plane_fin_group_kernel(const PlDesc* __restrict__ desc, PlFin fin) {
  const int b = blockIdx.y;
  const PlDesc D = desc[b];
  const int64_t g = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x;
  const int64_t nblk = pl_blocks(D.n);
  if (g * PL_GROUP >= nblk) return;
  const int kb = (int)min((int64_t)PL_GROUP, nblk - g * PL_GROUP);
  double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int32_t c = 0;
  for (int k = 0; k < kb; ++k) {
    const int64_t at = D.blk_off + g * PL_GROUP + k;
    c += fin.bcnt[at];
    for (int q = 0; q < 6; ++q) S[q] += fin.bsum[6 * at + q];
  }
  fin.gcnt[D.grp_off + g] = c;
  for (int q = 0; q < 6; ++q) fin.gsum[6 * (D.grp_off + g) + q] = S[q];
}

// The end of either pass: a lane per problem adds the group sums in group order from 0.  PASS 0: the centroid;
// PASS 1: the determinant step.
template <int PASS>
__global__ void __launch_bounds__(PL_TILE) plane_fin_total_kernel(const PlDesc* __restrict__ desc, PlFin fin, int batch) {
  const int b = blockIdx.x * PL_TILE + threadIdx.x;
  if (b >= batch) return;
  const PlDesc D = desc[b];
  const int64_t ng = pl_groups(D.n);
  double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int32_t c = 0;
  for (int64_t g = 0; g < ng; ++g) {
    c += fin.gcnt[D.grp_off + g];
    for (int q = 0; q < 6; ++q) S[q] += fin.gsum[6 * (D.grp_off + g) + q];
  }
  if (PASS == 0) {
    fin.m[b] = c;
    for (int q = 0; q < 3; ++q) fin.centroid[3 * b + q] = c > 0 ? S[q] / (double)c : 0.0;
  } else {
    double w[4] = {0.0, 0.0, 0.0, 0.0};
    if (fin.m[b] > 0) pl_from_sums(fin.centroid + 3 * b, S, w);
    for (int q = 0; q < 4; ++q) fin.plane[4 * b + q] = w[q];
  }
}

void launch_plane_models(hipStream_t s, int batch, int chunk, int max_n, const PlDesc* desc, const double* pts,
                         const PlSlot& slot, int64_t first) {
  if (batch <= 0 || max_n <= 0) return;
  hipLaunchKernelGGL(plane_model_kernel, dim3((max_n + PL_BLOCK - 1) / PL_BLOCK, batch), dim3(PL_BLOCK), 0, s, desc, pts,
                     slot, chunk, first);
}

void launch_plane_score(hipStream_t s, int batch, int chunk, int max_n, const PlDesc* desc, const double* pts,
                        const PlSlot& slot, const PlPart& part, int g0, int W) {
  if (batch <= 0 || max_n <= 0 || W <= 0) return;
  const int tiles = (max_n + PL_TILE - 1) / PL_TILE, lanes = (max_n + PL_BLOCK - 1) / PL_BLOCK;
  hipLaunchKernelGGL(plane_score_kernel, dim3(W * (PL_GROUP / PL_WAVES), tiles, batch), dim3(PL_BLOCK), 0, s, desc, pts,
                     slot, part, chunk, g0);
  hipLaunchKernelGGL(plane_group_kernel, dim3(lanes, W, batch), dim3(PL_BLOCK), 0, s, desc, slot, part, chunk, g0);
  hipLaunchKernelGGL(plane_total_kernel, dim3(lanes, batch), dim3(PL_BLOCK), 0, s, desc, slot, part, chunk, g0, W);
}

void launch_plane_finish(hipStream_t s, int batch, int max_points, const PlDesc* desc, const double* pts,
                         const PlFin& fin) {
  if (batch <= 0) return;
  const dim3 per_problem((batch + PL_TILE - 1) / PL_TILE), tile(PL_TILE), block(PL_BLOCK);
  const int64_t nblk = pl_blocks(max_points), ngrp = pl_groups(max_points);
  const dim3 gb((unsigned)std::max<int64_t>(1, (nblk + PL_BLOCK - 1) / PL_BLOCK), batch);
  const dim3 gg((unsigned)std::max<int64_t>(1, (ngrp + PL_BLOCK - 1) / PL_BLOCK), batch);
  hipLaunchKernelGGL(plane_winner_kernel, per_problem, tile, 0, s, desc, pts, fin, batch);
  hipLaunchKernelGGL(plane_fin_block_kernel<0>, gb, block, 0, s, desc, pts, fin);
  hipLaunchKernelGGL(plane_fin_group_kernel, gg, block, 0, s, desc, fin);
  hipLaunchKernelGGL(plane_fin_total_kernel<0>, per_problem, tile, 0, s, desc, fin, batch);
  hipLaunchKernelGGL(plane_fin_block_kernel<1>, gb, block, 0, s, desc, pts, fin);
  hipLaunchKernelGGL(plane_fin_group_kernel, gg, block, 0, s, desc, fin);
  hipLaunchKernelGGL(plane_fin_total_kernel<1>, per_problem, tile, 0, s, desc, fin, batch);
}

}  // namespace thip
