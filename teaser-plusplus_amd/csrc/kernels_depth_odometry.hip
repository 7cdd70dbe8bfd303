// kernels_depth_odometry.hip -- depth odometry for gfx950 (include/teaser_hip.h, "Depth odometry"; device code:
// icp_depth_odometry_device.h; host side: icp_depth_odometry.hip; design, bytes moved, launch counts and the resource
// report: DESIGN.md section 40).
//
// The block map is that of RGB-D odometry: the pixels of a pair's level are cut into blocks of kOdoBlock, the map names
// the pair of every block, a pair's descriptor says where its blocks begin; the blocks of level 0 of all pairs come
// first, then level 1, ...  The vertex and the normal kernel run over that whole list in one launch each.
//
// One iteration is two launches.  The sums run over the SOURCE pixels: every thread projects its own vertex, gathers the
// target vertex and normal (six float32) and forms its 29 values, so there is no key image and no atomic.  The 29 values
// of a wave are reduced by a split butterfly (dodo_wave_sums) that gives the bits of the contract's tree, then
// (w0 + w1) + (w2 + w3) through LDS, one partial per block.  The finishing kernel, one workgroup per pair, adds the
// partials in the order of groups, eight groups at a time, and thread 0 solves, updates the pose and tests convergence.
// A failed or converged pair carries a flag in its state: its blocks return at once.  Nothing is read back in the loop.
#include "icp_depth_odometry_device.h"
#include "wave_utils.h"

namespace thip {

namespace {

// The pair of block `blk` of level l and the pixel of this thread in it; false behind the level's last pixel.
__device__ __forceinline__ bool dodo_thread_pixel(const DodoArgs& a, int l, int blk, int* pair, int32_t* px) {
  const int p = a.blk_pair[a.level_blk0[l] + blk];
  *pair = p;
  *px = (blk - a.desc[p].blk_off[l]) * kOdoBlock + (int)threadIdx.x;
  return *px < dodo_n(a.desc[p], l);
}

// The level of block b of a launch over the blocks of all levels, and the block's index in its level.
__device__ __forceinline__ int dodo_block_level(const DodoArgs& a, int b, int* blk) {
  int l = 0;
  while (l + 1 < a.levels && b >= a.level_blk0[l + 1]) ++l;
  *blk = b - a.level_blk0[l];
  return l;
}

__global__ __launch_bounds__(kOdoBlock) void dodo_convert_kernel(const DodoArgs a) {
  int p;
  int32_t px;
  if (!dodo_thread_pixel(a, 0, (int)blockIdx.x, &p, &px)) return;
  const DodoDesc& d = a.desc[p];
  const int y = px / d.width, x = px - y * d.width;
  dodo_px_convert(d, a.in, a.img, 0, y, x);
  dodo_px_convert(d, a.in, a.img, 1, y, x);
}

// threads over the pixels of level l + 1
__global__ __launch_bounds__(kOdoBlock) void dodo_down_kernel(const DodoArgs a, int l) {
  int p;
  int32_t px;
  if (!dodo_thread_pixel(a, l + 1, (int)blockIdx.x, &p, &px)) return;
  const DodoDesc& d = a.desc[p];
  const int w = dodo_w(d, l + 1), y = px / w, x = px - y * w;
  dodo_px_down(d, a.img, l, 0, y, x);
  dodo_px_down(d, a.img, l, 1, y, x);
}

// threads over the pixels of all levels: the vertex maps (normal 0) or the target's normal map (normal 1)
__global__ __launch_bounds__(kOdoBlock) void dodo_maps_kernel(const DodoArgs a, int normal) {
  int blk, p;
  int32_t px;
  const int l = dodo_block_level(a, (int)blockIdx.x, &blk);
  if (!dodo_thread_pixel(a, l, blk, &p, &px)) return;
  const DodoDesc& d = a.desc[p];
  const int w = dodo_w(d, l), y = px / w, x = px - y * w;
  if (normal) {
    dodo_px_normal(d, a.img, l, y, x);
  } else {
    dodo_px_vertex(d, a.img, l, 0, y, x);
    dodo_px_vertex(d, a.img, l, 1, y, x);
  }
}

__device__ __forceinline__ double dodo_shfl_xor(double v, int o) {
  int2 w = __builtin_bit_cast(int2, v);
  w.x = __shfl_xor(w.x, o, 64);
  w.y = __shfl_xor(w.y, o, 64);
  return __builtin_bit_cast(double, w);
}

// One step of the split butterfly over the lanes' bit `o`: of the 2 kHalf values a lane holds, the lanes with the bit
// clear keep the first kHalf and the others the second, each adding what its partner (lane ^ o) held of them.  The tree
// of the contract adds v[i] + v[i + o] for i < o; the lane with the bit set adds the same two numbers the other way
// round, which are the same bits in IEEE arithmetic.
template <int kHalf>
__device__ __forceinline__ void dodo_split_step(double* v, int o, bool upper) {
#pragma unroll
  for (int j = 0; j < kHalf; ++j) {
    const double keep = upper ? v[j + kHalf] : v[j];
    const double give = upper ? v[j] : v[j + kHalf];
    v[j] = keep + dodo_shfl_xor(give, o);
  }
}

// The contract's tree over the 64 lanes of a wave for 32 values per lane (the values behind kOdoSums are zero) in
// 16 + 8 + 4 + 2 + 1 + 1 = 32 two-word exchanges: after the steps over the lane bits 5 .. 1 lane i holds value i >> 1
// summed over the lanes that agree with it in bit 0, and the last step adds the two.  Returns value lane >> 1 of the
// tree's v[0] in every lane.
__device__ __forceinline__ double dodo_wave_sums(double* v, int lane) {
  dodo_split_step<16>(v, 32, (lane & 32) != 0);
  dodo_split_step<8>(v, 16, (lane & 16) != 0);
  dodo_split_step<4>(v, 8, (lane & 8) != 0);
  dodo_split_step<2>(v, 4, (lane & 4) != 0);
  dodo_split_step<1>(v, 2, (lane & 2) != 0);
  const double other = dodo_shfl_xor(v[0], 1);
  return (lane & 1) ? other + v[0] : v[0] + other;
}

template <int kMode>
__global__ __launch_bounds__(kOdoBlock) void dodo_sums_kernel(const DodoArgs a, int l) {
  constexpr int kWaves = kOdoBlock / 64;
  __shared__ double runs[kWaves][32];
  int p;
  int32_t s;
  const bool in_level = dodo_thread_pixel(a, l, (int)blockIdx.x, &p, &s);
  const DodoState& st = a.state[p];
  if (st.failed || (kMode == kDodoSumIter && st.converged)) return;  // the whole block: a block serves one pair
  const DodoDesc& d = a.desc[p];
  double v[32];
  dodo_px_values(kMode, d, st, a.img, l, s, in_level, v);
  v[29] = v[30] = v[31] = 0.0;
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  const double t = dodo_wave_sums(v, lane);
  if ((lane & 1) == 0) runs[wave][lane >> 1] = t;
  __syncthreads();
  if (threadIdx.x < kOdoSums) {
    const int k = threadIdx.x;
    a.part[(d.part_off + ((int)blockIdx.x - d.blk_off[l])) * kOdoSums + k] = (runs[0][k] + runs[1][k]) + (runs[2][k] + runs[3][k]);
  }
}

// The sums of odo_sum_blocks (icp_odometry_device.h) in the same order, eight groups at a time: thread (slot, k) adds the
// blocks of group 8 c + slot for sum k, then the threads of slot 0 add the eight group sums in ascending order.
constexpr int kDodoFinishSlots = 8, kDodoFinishThreads = 32 * kDodoFinishSlots;

template <int kMode>
__global__ __launch_bounds__(kDodoFinishThreads) void dodo_finish_kernel(const DodoArgs a, int l, int iter, int first, int last) {
  __shared__ double tot[kOdoSums];
  __shared__ double gs[kDodoFinishSlots][32];
  const int p = blockIdx.x;
  DodoState& st = a.state[p];
  const DodoDesc& d = a.desc[p];
  const bool failed = st.failed != 0;
  if (kMode == kDodoSumIter) {
    if (failed) return;
    if (st.converged) {  // uniform over the workgroup: nobody else writes the flag in this launch
      __syncthreads();
      if (last && threadIdx.x == 0) st.converged = 0;
      return;
    }
  }
  const int k = threadIdx.x % 32, slot = threadIdx.x / 32;
  const double* part = a.part + d.part_off * kOdoSums;
  const int64_t nblk = failed ? 0 : dodo_blocks(d, l);
  const int64_t ngroups = (nblk + kOdoGroup - 1) / kOdoGroup;
  double total = 0.0;
  for (int64_t g0 = 0; g0 < ngroups; g0 += kDodoFinishSlots) {  // uniform over the workgroup
    const int64_t g = g0 + slot;
    if (g < ngroups && k < kOdoSums) {
      const int64_t b0 = g * kOdoGroup, b1 = b0 + kOdoGroup < nblk ? b0 + kOdoGroup : nblk;
      double s = 0.0;
#pragma unroll 8
      for (int64_t b = b0; b < b1; ++b) s += part[b * kOdoSums + k];
      gs[slot][k] = s;
    }
    __syncthreads();
    if (slot == 0 && k < kOdoSums)
      for (int q = 0; q < kDodoFinishSlots && g0 + q < ngroups; ++q) total += gs[q][k];
    __syncthreads();
  }
  if (slot == 0 && k < kOdoSums) tot[k] = total;
  __syncthreads();
  if (threadIdx.x != 0) return;
  teaser_icp_depth_odometry_trace_c* rec = (kMode == kDodoSumIter && d.trace_off >= 0) ? a.trace + d.trace_off + iter : nullptr;
  dodo_finish(kMode, d, st, tot, l, first, a.results + p, rec);
  if (kMode == kDodoSumIter && last) st.converged = 0;
}

template <int kMode>
void dodo_sums_and_finish(hipStream_t s, const DodoArgs& a, int l, int iter, int first, int last) {
  if (a.level_nblk[l] > 0) hipLaunchKernelGGL(dodo_sums_kernel<kMode>, dim3(a.level_nblk[l]), dim3(kOdoBlock), 0, s, a, l);
  hipLaunchKernelGGL(dodo_finish_kernel<kMode>, dim3(a.batch), dim3(kDodoFinishThreads), 0, s, a, l, iter, first, last);
}

}  // namespace

void launch_dodo_preprocess(hipStream_t s, const DodoArgs& a) {
  const dim3 b(kOdoBlock);
  int all = 0;
  for (int l = 0; l < a.levels; ++l) all += a.level_nblk[l];
  hipLaunchKernelGGL(dodo_convert_kernel, dim3(a.level_nblk[0]), b, 0, s, a);
  for (int l = 0; l + 1 < a.levels; ++l)
    if (a.level_nblk[l + 1] > 0) hipLaunchKernelGGL(dodo_down_kernel, dim3(a.level_nblk[l + 1]), b, 0, s, a, l);
  hipLaunchKernelGGL(dodo_maps_kernel, dim3(all), b, 0, s, a, 0);
  hipLaunchKernelGGL(dodo_maps_kernel, dim3(all), b, 0, s, a, 1);
}

void launch_dodo_iteration(hipStream_t s, const DodoArgs& a, int level, int iter, int first, int last) {
  dodo_sums_and_finish<kDodoSumIter>(s, a, level, iter, first, last);
}

void launch_dodo_information(hipStream_t s, const DodoArgs& a) { dodo_sums_and_finish<kDodoSumInfo>(s, a, 0, 0, 0, 0); }

}  // namespace thip
