// kernels_odometry.hip -- RGB-D odometry for gfx950 (include/teaser_hip.h, "RGB-D odometry"; device code:
// icp_odometry_device.h; host side: icp_odometry.hip; design, bytes moved, launch counts and the resource report:
// DESIGN.md section 33).
//
// Every image kernel runs one thread per pixel of one pyramid level over ALL pairs of the batch: the pixels of a pair's
// level are cut into blocks of kOdoBlock, the block map names the pair of every block, and a pair's descriptor says where
// its blocks begin.  The same cut is the summation order's: the sums kernel serves one block of target pixels per
// workgroup, reduces the kOdoSums values of its 256 pixels by the contract's tree (six shuffle steps inside a wave, then
// (w0 + w1) + (w2 + w3) through LDS) and writes one partial per block; the finishing kernel, one workgroup per pair, adds
// the partials in the order of groups, eight groups at a time, and thread 0 solves and updates the pose.
//
// One iteration is three launches: match (a 64-bit atomic minimum of (bits(zf) << 32) | s per target pixel), sums (which
// reads every key once and puts the empty key back, so that no clearing launch is needed) and finish.  A failed pair
// carries a flag in its state: its blocks return at once.  Nothing is read back inside the loop.
#include "icp_odometry_device.h"
#include "wave_utils.h"

namespace thip {

namespace {

// The pair of this block and the pixel of this thread in level l of it; false behind the level's last pixel.
__device__ __forceinline__ bool odo_thread_pixel(const OdoArgs& a, int l, int* pair, int32_t* px) {
  const int p = a.blk_pair[a.level_blk0[l] + (int)blockIdx.x];
  *pair = p;
  *px = ((int)blockIdx.x - a.desc[p].blk_off[l]) * kOdoBlock + (int)threadIdx.x;
  return *px < odo_n(a.desc[p], l);
}

__global__ __launch_bounds__(kOdoBlock) void odo_convert_kernel(const OdoArgs a) {
  int p;
  int32_t px;
  if (!odo_thread_pixel(a, 0, &p, &px)) return;
  const OdoDesc& d = a.desc[p];
  const int y = px / d.width, x = px - y * d.width;
  odo_px_convert(d, a.in, a.tmp, 0, y, x);
  odo_px_convert(d, a.in, a.tmp, 1, y, x);
}

__global__ __launch_bounds__(kOdoBlock) void odo_filter_kernel(const OdoArgs a, int l, int mode) {
  int p;
  int32_t px;
  if (!odo_thread_pixel(a, l, &p, &px)) return;
  const OdoDesc& d = a.desc[p];
  const int w = odo_w(d, l), y = px / w, x = px - y * w;
  odo_px_filter(d, a.img, a.tmp, l, mode, y, x);
}

// threads over the pixels of level l + 1
__global__ __launch_bounds__(kOdoBlock) void odo_down_kernel(const OdoArgs a, int l) {
  int p;
  int32_t px;
  if (!odo_thread_pixel(a, l + 1, &p, &px)) return;
  const OdoDesc& d = a.desc[p];
  const int w = odo_w(d, l + 1), y = px / w, x = px - y * w;
  odo_px_down(d, a.img, a.tmp, l, y, x);
}

__global__ __launch_bounds__(kOdoBlock) void odo_scale_xyz_kernel(const OdoArgs a) {
  int p;
  int32_t px;
  if (!odo_thread_pixel(a, 0, &p, &px)) return;
  const OdoDesc& d = a.desc[p];
  const int y = px / d.width, x = px - y * d.width;
  odo_px_scale_xyz(d, a.state[p], a.img, y, x);
}

__global__ __launch_bounds__(kOdoBlock) void odo_match_kernel(const OdoArgs a, int l) {
  int p;
  int32_t s;
  if (!odo_thread_pixel(a, l, &p, &s)) return;
  const OdoState& st = a.state[p];
  if (st.failed) return;
  const OdoDesc& d = a.desc[p];
  int32_t pixel;
  uint64_t key;
  if (odo_px_match(d, st, a.img, l, s, &pixel, &key))
    atomicMin((unsigned long long*)a.keys + d.key_off + pixel, (unsigned long long)key);
}

__device__ __forceinline__ double odo_shfl_down(double v, int o) {
  int2 w = __builtin_bit_cast(int2, v);
  w.x = __shfl_down(w.x, o, 64);
  w.y = __shfl_down(w.y, o, 64);
  return __builtin_bit_cast(double, w);
}

template <int kMode>
__global__ __launch_bounds__(kOdoBlock) void odo_sums_kernel(const OdoArgs a, int l) {
  constexpr int kWaves = kOdoBlock / 64;
  __shared__ double runs[kWaves][kOdoSums];
  int p;
  int32_t tp;
  const bool in_level = odo_thread_pixel(a, l, &p, &tp);
  const OdoState& st = a.state[p];
  if (st.failed) return;  // the whole block: a block serves one pair
  const OdoDesc& d = a.desc[p];
  uint64_t key = kOdoEmptyKey;
  if (in_level) {
    uint64_t* at = a.keys + d.key_off + tp;
    key = *at;
    if (key != kOdoEmptyKey) *at = kOdoEmptyKey;  // the next match launch finds the keys empty
  }
  double v[kOdoSums];
  odo_px_values(kMode, d, st, a.img, l, tp, key, v);
  constexpr int kLive = kMode == kOdoSumNorm ? 2 : (kMode == kOdoSumInfo ? 21 : 28);  // the sums behind are zero
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
#pragma unroll
  for (int k = 0; k < kOdoSums; ++k) {
    if (k >= kLive && k != kOdoSums - 1) continue;
    double t = v[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t = t + odo_shfl_down(t, o);  // lane i < o ends with the tree's v[i]
    if (lane == 0) runs[wave][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < kOdoSums) {
    const int k = threadIdx.x;
    const bool live = k < kLive || k == kOdoSums - 1;
    const double t = live ? (runs[0][k] + runs[1][k]) + (runs[2][k] + runs[3][k]) : 0.0;
    a.part[(d.part_off + ((int)blockIdx.x - d.blk_off[l])) * kOdoSums + k] = t;
  }
}

// The sums of odo_sum_blocks (icp_odometry_device.h) in the same order, eight groups at a time: thread (slot, k) adds the
// blocks of group 8 c + slot for sum k, then the threads of slot 0 add the eight group sums in ascending order.
constexpr int kOdoFinishSlots = 8, kOdoFinishThreads = 32 * kOdoFinishSlots;

template <int kMode>
__global__ __launch_bounds__(kOdoFinishThreads) void odo_finish_kernel(const OdoArgs a, int l, int next_level, int iter) {
  __shared__ double tot[kOdoSums];
  __shared__ double gs[kOdoFinishSlots][32];
  const int p = blockIdx.x;
  OdoState& st = a.state[p];
  const OdoDesc& d = a.desc[p];
  const bool failed = st.failed != 0;
  if (failed && kMode != kOdoSumInfo) return;
  const int k = threadIdx.x % 32, slot = threadIdx.x / 32;
  const double* part = a.part + d.part_off * kOdoSums;
  const int64_t nblk = failed ? 0 : odo_blocks(d, l);
  const int64_t ngroups = (nblk + kOdoGroup - 1) / kOdoGroup;
  double total = 0.0;
  for (int64_t g0 = 0; g0 < ngroups; g0 += kOdoFinishSlots) {  // uniform over the workgroup
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
      for (int q = 0; q < kOdoFinishSlots && g0 + q < ngroups; ++q) total += gs[q][k];
    __syncthreads();
  }
  if (slot == 0 && k < kOdoSums) tot[k] = total;
  __syncthreads();
  if (threadIdx.x != 0) return;
  teaser_icp_odometry_trace_c* rec = (kMode == kOdoSumIter && d.trace_off >= 0) ? a.trace + d.trace_off + iter : nullptr;
  odo_finish(kMode, d, st, tot, l, next_level, a.results + p, rec);
}

inline void odo_level_launch(hipStream_t s, void (*kernel)(OdoArgs, int), const OdoArgs& a, int grid_level, int l) {
  if (a.level_nblk[grid_level] > 0)
    hipLaunchKernelGGL(kernel, dim3(a.level_nblk[grid_level]), dim3(kOdoBlock), 0, s, a, l);
}

template <int kMode>
void odo_sums_and_finish(hipStream_t s, const OdoArgs& a, int l, int next_level, int iter) {
  odo_level_launch(s, odo_match_kernel, a, l, l);
  odo_level_launch(s, odo_sums_kernel<kMode>, a, l, l);
  hipLaunchKernelGGL(odo_finish_kernel<kMode>, dim3(a.batch), dim3(kOdoFinishThreads), 0, s, a, l, next_level, iter);
}

}  // namespace

void launch_odo_preprocess(hipStream_t s, const OdoArgs& a, int levels, int next_level) {
  const dim3 g0(a.level_nblk[0]), b(kOdoBlock);
  hipLaunchKernelGGL(odo_convert_kernel, g0, b, 0, s, a);
  hipLaunchKernelGGL(odo_filter_kernel, g0, b, 0, s, a, 0, (int)kOdoGaussIn);
  odo_sums_and_finish<kOdoSumNorm>(s, a, 0, next_level, 0);
  hipLaunchKernelGGL(odo_scale_xyz_kernel, g0, b, 0, s, a);
  for (int l = 0; l + 1 < levels; ++l) {
    hipLaunchKernelGGL(odo_filter_kernel, dim3(a.level_nblk[l]), b, 0, s, a, l, (int)kOdoGaussLevel);
    odo_level_launch(s, odo_down_kernel, a, l + 1, l);
  }
  for (int l = 0; l < levels; ++l)
    hipLaunchKernelGGL(odo_filter_kernel, dim3(a.level_nblk[l]), b, 0, s, a, l, (int)kOdoSobel);
}

void launch_odo_iteration(hipStream_t s, const OdoArgs& a, int level, int next_level, int iter) {
  odo_sums_and_finish<kOdoSumIter>(s, a, level, next_level, iter);
}

void launch_odo_information(hipStream_t s, const OdoArgs& a) { odo_sums_and_finish<kOdoSumInfo>(s, a, 0, -1, 0); }

}  // namespace thip
