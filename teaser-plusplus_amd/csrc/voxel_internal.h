// voxel_internal.h -- structures shared by the voxel down-sampling host code (voxel.hip) and its gfx950 kernels
// (kernels_voxel.hip).  Kept apart from internal.h: the voxel handle shares nothing with teaser_hip_solver.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace thip {

constexpr int kVoxBlock = 256;   // points per key / scatter block (a block never straddles two problems)
constexpr int kVoxLaneRun = 64;  // runs up to this length are summed by one lane, longer ones by a whole wave
constexpr unsigned kVoxLongBlocks = 4096;  // grid of the long-run kernel (4 waves per block, grid-stride over runs)

// One problem of a batch (host-built, read-only on the device).  Its points occupy [off, off + n) of the packed
// arrays, both in input order and after the sort (the problem index is the most significant key field).
struct VoxDesc {
  int64_t off;
  int32_t n;
  int32_t blk_off;   // first key / scatter block of this problem
  double lo[3];      // min_bound - 0.5 v, per axis
  double v;          // voxel size
  int32_t shift[3];  // bit position of i_x, i_y, i_z inside the key (i_z at 0)
  int32_t pad;
};

// Voxel index of one coordinate: floor((x - lo) / v), an IEEE division (no reciprocal, nothing contracted).  The host
// (extent of each problem) and the device (keys) run this same expression; it is monotone in x, so the largest
// coordinate has the largest index.
__host__ __device__ inline uint64_t vox_index(double x, double lo, double v) { return (uint64_t)floor((x - lo) / v); }

// ORs `value` (< 2^32) into the 128-bit key (hi:lo) at bit `shift` (< 128).
__host__ __device__ inline void vox_put(uint64_t& lo, uint64_t& hi, uint64_t value, int shift) {
  lo |= shift < 64 ? value << shift : 0;
  hi |= shift == 0 ? 0 : (shift < 64 ? value >> (64 - shift) : value << (shift - 64));
}

// Scratch needed by launch_voxel_sort and launch_voxel_runs (radix sort, scan) for n keys.
size_t voxel_sort_temp_bytes(int64_t n);

// keys (hi:lo) and the identity permutation of every point.
void launch_voxel_keys(hipStream_t s, const VoxDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                       const double* d_pts, int prob_shift, uint64_t* d_key_lo, uint64_t* d_key_hi, int32_t* d_iota);
// Stable sort of the points by key over `bits` bits (one LSD pass per 64-bit word); perm receives the sorted order.
hipError_t launch_voxel_sort(hipStream_t s, void* d_temp, size_t temp_bytes, int64_t n, int bits,
                             const uint64_t* d_key_lo, const uint64_t* d_key_hi, const int32_t* d_iota,
                             uint64_t* d_sorted, uint64_t* d_gathered, int32_t* d_perm1, int32_t* d_perm);
// Sorted points, run heads, run ids (inclusive scan of the heads) and run starts (run_start[R] = n).
hipError_t launch_voxel_runs(hipStream_t s, void* d_temp, size_t temp_bytes, int64_t n, bool two_words,
                             const double* d_pts, const uint64_t* d_key_lo, const uint64_t* d_key_hi,
                             const int32_t* d_perm, double* d_sorted_pts, int32_t* d_head, int32_t* d_run_id,
                             int32_t* d_run_start);
// Per problem {first run, number of runs}, then the mean and count of every run.
void launch_voxel_reduce(hipStream_t s, const VoxDesc* d_desc, int batch, int64_t n, const int32_t* d_run_id,
                         const int32_t* d_run_start, const double* d_sorted_pts, int32_t* d_summary, double* d_mean,
                         int32_t* d_count);
// voxel_of_point[perm[j]] = run of sorted point j - first run of its problem.
void launch_voxel_trace(hipStream_t s, const VoxDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                        const int32_t* d_perm, const int32_t* d_run_id, const int32_t* d_summary, int32_t* d_trace);

}  // namespace thip
