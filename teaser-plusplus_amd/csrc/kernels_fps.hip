// kernels_fps.hip -- gfx950 kernels of farthest-point down-sampling (include/teaser_hip.h, "Farthest-point
// down-sampling"; host side: icp_fps.hip; design, capacity arithmetic and register table: DESIGN.md section 27).
//
// Two routes, the same bits (icp_fps_device.h says why):
//   resident   one 1 024-thread workgroup per cloud of n <= 10 240 points runs the whole K-round loop in one launch.
//              Lane t keeps points t, t + 1024, ... (ten at most) and their running distances in registers; HBM is read
//              once and written once.  Per round: the update and the lane's best over its tile, a wave reduction of
//              (d, index) by shuffles, the winning lane of each wave publishes (d, index, x, y, z) into its slot of a
//              double-buffered LDS table, ONE workgroup barrier, and every wave reduces the sixteen slots itself and reads
//              the next centre's coordinates from the winning slot.  A wave may be one round ahead of another and never
//              two: a slot written in round k is rewritten in round k + 2, behind the barrier of round k + 1, which no
//              wave passes before every wave has finished reading round k.
//   streamed   one launch per round over 256-thread blocks of 1 024 points.  Each block first reduces the candidates the
//              blocks of its cloud wrote in the previous round (redundantly, so no block waits for another and nothing is
//              atomic), updates its slice of d in memory and writes its own candidate into the other half of the table.
// No spin-wait, no grid-wide synchronisation, no atomics, no scratch.
#include <math.h>

#include "icp_fps_device.h"

namespace thip {

namespace {

// What a wave's winning lane publishes.
struct FpsSlot {
  double d;
  int32_t i;
  int32_t pad;
  double x, y, z;
};

__device__ __forceinline__ FpsBest fps_shuffle_xor(FpsBest b, int o) {
  return FpsBest{__shfl_xor(b.d, o, 64), __shfl_xor(b.i, o, 64), 0};
}

__device__ __forceinline__ FpsBest fps_wave_best(FpsBest b) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) b = fps_combine(b, fps_shuffle_xor(b, o));
  return b;
}

__global__ __launch_bounds__(kFpsResidentThreads) void fps_resident_kernel(const FpsDesc* __restrict__ descs,
                                                                           const int32_t* __restrict__ res_map,
                                                                           const double* __restrict__ pts,
                                                                           int32_t* __restrict__ index,
                                                                           double* __restrict__ sel,
                                                                           double* __restrict__ fin) {
  __shared__ FpsSlot slot[2][kFpsResidentThreads / 64];
  const FpsDesc D = descs[res_map[blockIdx.x]];
  const int t = threadIdx.x, wave = t >> 6;
  const double* __restrict__ P = pts + 3 * D.off;
  const int tiles = (D.n + kFpsResidentThreads - 1) / kFpsResidentThreads;  // workgroup-uniform
  double x[kFpsResidentTile], y[kFpsResidentTile], z[kFpsResidentTile], d[kFpsResidentTile];
#pragma unroll
  for (int i = 0; i < kFpsResidentTile; ++i) {
    const int j = t + kFpsResidentThreads * i;
    const bool in = j < D.n;
    // a slot without a point loads the cloud's last one (n >= 1), so that no load sits behind a branch; 32-bit offsets
    // from one scalar base, so that no load needs an address pair of its own
    const uint32_t o = 3u * (uint32_t)(in ? j : D.n - 1);
    x[i] = P[o];
    y[i] = P[o + 1];
    z[i] = P[o + 2];
    d[i] = in ? (double)INFINITY : -1.0;  // -1: a slot without a point never wins and min() leaves it alone
  }
  int32_t cur = D.start;
  double cd = (double)INFINITY;  // d[cur] before the update
  double cx = P[3 * (int64_t)cur], cy = P[3 * (int64_t)cur + 1], cz = P[3 * (int64_t)cur + 2];
  for (int k = 0;; ++k) {
    if (t == 0) {
      index[D.out_off + k] = cur;
      sel[D.out_off + k] = cd;
    }
    FpsBest b = fps_none();
#pragma unroll
    for (int i = 0; i < kFpsResidentTile; ++i)
      if (i < tiles) {
        d[i] = fps_min(d[i], fps_d2(x[i], y[i], z[i], cx, cy, cz));
        if (d[i] > b.d) {  // ascending index inside the tile: the strict > keeps the smallest
          b.d = d[i];
          b.i = t + kFpsResidentThreads * i;
        }
      }
    if (k == D.k - 1) break;
    b = fps_wave_best(b);
    // the wave's winner publishes; the tile slot is wave-uniform, so the coordinates are picked by a scalar branch
    // with constant register indices (a dynamic index would put the tile into scratch)
    const int32_t wi = __builtin_amdgcn_readfirstlane(b.i);
    if (wi != INT32_MAX) {  // (a wave without points publishes the identity)
      double px = 0, py = 0, pz = 0;
      switch (wi / kFpsResidentThreads) {
#define FPS_PICK(I) case I: px = x[I], py = y[I], pz = z[I]; break;
        FPS_PICK(0) FPS_PICK(1) FPS_PICK(2) FPS_PICK(3) FPS_PICK(4) FPS_PICK(5) FPS_PICK(6) FPS_PICK(7) FPS_PICK(8)
        FPS_PICK(9)
#undef FPS_PICK
        default: break;
      }
      static_assert(kFpsResidentTile == 10, "the switch above names every slot of the tile");
      if (t == wi % kFpsResidentThreads) slot[k & 1][wave] = FpsSlot{b.d, wi, 0, px, py, pz};
    } else if ((t & 63) == 0) {
      slot[k & 1][wave] = FpsSlot{-1.0, INT32_MAX, 0, 0.0, 0.0, 0.0};
    }
    __syncthreads();
    const FpsSlot* S = slot[k & 1];
    b = FpsBest{S[t & 15].d, S[t & 15].i, 0};
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) b = fps_combine(b, fps_shuffle_xor(b, o));
    cd = b.d;
    if (b.d > 0) {  // fps_next: workgroup-uniform
      const FpsSlot& w = S[(b.i % kFpsResidentThreads) >> 6];
      cur = b.i, cx = w.x, cy = w.y, cz = w.z;
    }
  }
  if (fin) {
#pragma unroll
    for (int i = 0; i < kFpsResidentTile; ++i) {
      const int j = t + kFpsResidentThreads * i;
      if (j < D.n) fin[D.off + j] = d[i];
    }
  }
}

// The best of a 256-thread block, in every thread.
__device__ __forceinline__ FpsBest fps_block_best(FpsBest b, FpsBest* red4) {
  b = fps_wave_best(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = b;
  __syncthreads();
  return fps_combine(fps_combine(red4[0], red4[1]), fps_combine(red4[2], red4[3]));
}

__global__ __launch_bounds__(kFpsBlock) void fps_round_kernel(const FpsDesc* __restrict__ descs,
                                                              const int32_t* __restrict__ blk_map, int n_blk, int round,
                                                              const double* __restrict__ pts,
                                                              int32_t* __restrict__ index, double* __restrict__ sel,
                                                              double* __restrict__ fin, FpsBest* __restrict__ part) {
  __shared__ FpsBest red4[4];
  const FpsDesc D = descs[blk_map[blockIdx.x]];
  if (round >= D.k) return;  // block-uniform: the cloud has its samples
  const int t = threadIdx.x, q = (int)blockIdx.x - D.blk_off;
  int32_t cur = D.start;
  double cd = (double)INFINITY;
  if (round > 0) {  // the winner of the previous round, from the candidates of this cloud's blocks
    const FpsBest* prev = part + (size_t)((round - 1) & 1) * n_blk + D.blk_off;
    FpsBest m = fps_none();
    for (int i = t; i < D.nblk; i += kFpsBlock) m = fps_combine(m, prev[i]);
    m = fps_block_best(m, red4);
    cd = m.d;
    cur = fps_next(index[D.out_off + round - 1], m);
  }
  if (q == 0 && t == 0) {
    index[D.out_off + round] = cur;
    sel[D.out_off + round] = cd;
  }
  const double* __restrict__ P = pts + 3 * D.off;
  double* __restrict__ dist = fin + D.off;
  const double cx = P[3 * (int64_t)cur], cy = P[3 * (int64_t)cur + 1], cz = P[3 * (int64_t)cur + 2];
  FpsBest b = fps_none();
#pragma unroll
  for (int u = 0; u < kFpsBlockPoints / kFpsBlock; ++u) {
    const int64_t j = (int64_t)q * kFpsBlockPoints + u * kFpsBlock + t;
    if (j < D.n) {
      const double v = fps_d2(P[3 * j], P[3 * j + 1], P[3 * j + 2], cx, cy, cz);
      const double dn = round == 0 ? v : fps_min(dist[j], v);  // min(+inf, v) = v: round 0 needs no cleared d
      dist[j] = dn;
      if (dn > b.d) {
        b.d = dn;
        b.i = (int32_t)j;
      }
    }
  }
  b = fps_block_best(b, red4);
  if (t == 0) part[(size_t)(round & 1) * n_blk + blockIdx.x] = b;
}

}  // namespace

void launch_fps_resident(hipStream_t s, const FpsDesc* d_desc, const int32_t* d_res_map, int n_res, const double* d_pts,
                         int32_t* d_index, double* d_sel, double* d_fin) {
  if (n_res <= 0) return;
  hipLaunchKernelGGL(fps_resident_kernel, dim3(n_res), dim3(kFpsResidentThreads), 0, s, d_desc, d_res_map, d_pts,
                     d_index, d_sel, d_fin);
}

void launch_fps_round(hipStream_t s, const FpsDesc* d_desc, const int32_t* d_blk_map, int n_blk, int round,
                      const double* d_pts, int32_t* d_index, double* d_sel, double* d_fin, FpsBest* d_part) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(fps_round_kernel, dim3(n_blk), dim3(kFpsBlock), 0, s, d_desc, d_blk_map, n_blk, round, d_pts,
                     d_index, d_sel, d_fin, d_part);
}

}  // namespace thip
