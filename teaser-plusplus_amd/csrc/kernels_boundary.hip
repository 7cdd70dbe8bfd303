// kernels_boundary.hip -- boundary-point detection for gfx950 (include/teaser_hip.h, "Boundary points"; device code:
// icp_boundary_device.h; host side: icp_boundary.hip; design and the resource report: DESIGN.md section 30).
//
// The neighbour lists, the pieces and the block map are those of the Open3D-form FPFH (kernels_fpfh.hip).  One wave per
// point, four waves per block; a block serves the 64 points of a map block.  A list holds at most 99 neighbours behind
// position 0, so the angles fit two per lane: lane l owns the slots 2 l and 2 l + 1 (list positions 2 l + 1 and 2 l + 2).
// The unused slots hold +inf.  The 128 slots are sorted in registers by a bitonic network: the seven stages of distance 1
// stay inside a lane, the other 21 exchange a slot with the lane at distance 1 .. 32.  Afterwards slot e + 1 follows slot
// e, so the neighbour differences need the lane's own pair and one shift by a lane; lane 0 adds the wrap term, and a
// wave maximum ends the point.  No LDS, no scratch, no atomics on doubles; the boundary points of a wave are added to
// their cloud's int32 counter once per wave.
#include "icp_boundary_device.h"
#include "icp_internal.h"

namespace thip {

// One compare-exchange of the network with the lane at distance `dist` (a power of two below 64).
__device__ __forceinline__ double boundary_exchange(double a, int dist, bool keep_min) {
  const double o = __shfl_xor(a, dist, kIcpCovBlock);
  return keep_min ? (o < a ? o : a) : (o > a ? o : a);
}

// Ascending sort of the 128 slots (slot 2 l + s is a_s of lane l).  Equal keys are never exchanged, so no value is lost.
__device__ __forceinline__ void boundary_sort(double& a0, double& a1, int lane) {
#pragma unroll
  for (int k = 2; k <= kBoundarySlots; k <<= 1) {
    const bool up = ((2 * lane) & k) == 0;  // the direction of this lane's run of k slots
#pragma unroll
    for (int j = k >> 1; j >= 2; j >>= 1) {
      const bool keep_min = (((2 * lane) & j) == 0) == up;
      a0 = boundary_exchange(a0, j >> 1, keep_min);
      a1 = boundary_exchange(a1, j >> 1, keep_min);
    }
    const bool swap = up ? a1 < a0 : a1 > a0;  // distance 1: the lane's own pair
    const double lo = swap ? a1 : a0, hi = swap ? a0 : a1;
    a0 = lo;
    a1 = hi;
  }
}

__device__ __forceinline__ double boundary_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_xor(v, o, kIcpCovBlock);
    v = t > v ? t : v;
  }
  return v;
}

__global__ __launch_bounds__(kIcpCovBlock* kBoundaryWaves) void icp_boundary_kernel(
    const IcpDesc* __restrict__ descs, const IcpSearchDesc* __restrict__ sds, const IcpBoundaryDesc* __restrict__ bds,
    const int32_t* __restrict__ blk_prob, int n_hyb, const double* __restrict__ q, const double* __restrict__ normals,
    const int32_t* __restrict__ list_idx, uint8_t* __restrict__ mask, double* __restrict__ max_gap,
    int32_t* __restrict__ count, int32_t* __restrict__ n_boundary) {
  int64_t i0;
  const int p = list_block_piece(descs, blk_prob, n_hyb, &i0);
  const IcpDesc& d = descs[p];
  const IcpSearchDesc& sd = sds[p];
  const IcpBoundaryDesc& bd = bds[p];
  const int lane = threadIdx.x % kIcpCovBlock, wave = threadIdx.x / kIcpCovBlock;
  const double* P = q + 3 * d.t_off;  // the cloud's own arrays, by its own indices
  const double* N = normals + 3 * d.t_off;
  const int k0 = 2 * lane + 1, k1 = 2 * lane + 2;  // the list positions of this lane's slots
  int found = 0;
  for (int t = wave; t < kIcpCovBlock; t += kBoundaryWaves) {  // uniform over the wave
    const int64_t i = i0 + t;
    if (i >= d.n_s) break;
    const int64_t ci = (d.s_off - d.t_off) + i;  // the piece's point i is the cloud's point ci
    const int32_t* idx = list_idx + sd.out_off + i * sd.k;
    const int32_t j0 = k0 < sd.k ? idx[k0] : -1, j1 = k1 < sd.k ? idx[k1] : -1;
    // the valid entries stand at the front of a row, so counting them is fpfh_list_length
    const int cnt = __popcll(__ballot(j0 >= 0)) + __popcll(__ballot(j1 >= 0));  // the angles
    const int m = idx[0] >= 0 ? 1 + cnt : 0;
    const double pi3[3] = {P[3 * ci], P[3 * ci + 1], P[3 * ci + 2]};
    const double ni3[3] = {N[3 * ci], N[3 * ci + 1], N[3 * ci + 2]};
    double u[3], v[3];
    const double nan = __builtin_nan("");
    double gap = 0.0;
    if (!boundary_frame(ni3, u, v)) {
      gap = nan;
    } else if (m > 1) {
      double a0 = __builtin_inf(), a1 = __builtin_inf();
      if (j0 >= 0) a0 = boundary_angle(pi3, P + 3 * (int64_t)j0, u, v);
      if (j1 >= 0) a1 = boundary_angle(pi3, P + 3 * (int64_t)j1, u, v);
      if (__ballot(a0 != a0 || a1 != a1)) {
        gap = nan;
      } else {
        boundary_sort(a0, a1, lane);
        double g = 0.0;
        if (k0 < cnt) g = boundary_step(g, a1 - a0);               // slots 2 l and 2 l + 1
        const double next = __shfl_down(a0, 1, kIcpCovBlock);      // slot 2 l + 2
        if (k1 < cnt) g = boundary_step(g, next - a1);
        const int last = cnt - 1;
        const double al0 = __shfl(a0, last >> 1, kIcpCovBlock), al1 = __shfl(a1, last >> 1, kIcpCovBlock);
        const double first = __shfl(a0, 0, kIcpCovBlock);
        if (lane == 0) g = boundary_step(g, boundary_wrap(first, (last & 1) ? al1 : al0));
        gap = boundary_wave_max(g);
      }
    }
    if (lane == 0) {
      const bool is = boundary_is_boundary(gap, bd.threshold);
      mask[d.s_off + i] = is ? 1 : 0;
      if (max_gap) max_gap[d.s_off + i] = gap;
      if (count) count[d.s_off + i] = m;
      found += is ? 1 : 0;
    }
  }
  if (lane == 0 && found) atomicAdd(n_boundary + bd.cloud, found);
}

void launch_icp_boundary(hipStream_t s, const IcpDesc* d_desc, const IcpSearchDesc* d_sd, const IcpBoundaryDesc* d_bd,
                         const int32_t* d_blk_prob, int n_hyb, int n_knn, const double* d_q, const double* d_normals,
                         const int32_t* d_list_idx, uint8_t* d_mask, double* d_max_gap, int32_t* d_count,
                         int32_t* d_n_boundary) {
  if (n_hyb + n_knn <= 0) return;
  hipLaunchKernelGGL(icp_boundary_kernel, dim3(n_hyb + n_knn), dim3(kIcpCovBlock * kBoundaryWaves), 0, s, d_desc, d_sd,
                     d_bd, d_blk_prob, n_hyb, d_q, d_normals, d_list_idx, d_mask, d_max_gap, d_count, d_n_boundary);
}

}  // namespace thip
