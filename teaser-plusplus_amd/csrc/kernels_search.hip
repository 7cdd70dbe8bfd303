// kernels_search.hip -- nearest-neighbour search between two clouds for gfx950: k-NN, hybrid and uncapped radius
// search of a query set in an indexed data cloud (Open3D's KDTreeFlann / NearestNeighborSearch), on the hash grid of
// kernels_icp.hip.  The contract is written out in include/teaser_hip.h ("Neighbour search"), the design, the
// termination argument and the launch counts in DESIGN.md section 28.
//
// The data cloud of a problem is the "target" of its IcpDesc (n_t, t_off, the grid), the query set its "source" (n_s,
// s_off in the packed query array x).  Everything a self search takes for granted about its query -- that its cell is
// a cell of the grid -- is dropped here: a query's cell may lie anywhere in [-2, 2^40]^3.
//
// k-NN: icp_search_ring_kernel is the ring search of kernels_outlier.hip with three changes.  (1) Ring r is cut to the
// box [0, cmax] before it is enumerated, so a loop never runs over cells that hold nothing.  (2) The rings start at
// r0, the Chebyshev distance from the query's cell to that box (smaller rings hold no cell of the grid), and ring_cap
// rings are searched from there.  (3) A query with r0 > kIcpSearchR0Max goes straight to the worklist: ring r0 of such a
// query is a whole face of the grid.  The bound and the clamp argument: DESIGN.md section 17.  The two ring kernels
// stay written out, each in its file: as instantiations of one walk both measured slower (DESIGN.md section 17,
// profiles/knn_shared/); tests/search_kernel_emulation.cpp and tests/test_gpu_knn_shared.py hold them to the same
// bits on a cloud searched in itself.  icp_search_scan_kernel is icp_knn_scan of icp_knn_device.h with the query taken
// from x.  Both routes produce the min(k, n_data) smallest (d2, j) exactly, so the route never shows.
//
// Hybrid and radius search run on the grid built for the radius, over the 27 cells around the query's cell: a cell
// outside [0, cmax] holds no data point and is skipped, and a bucket is visited once (the rule of
// icp_radius_count_kernel: an offset whose bucket equals that of an earlier visited offset is skipped).  The radius
// search counts, scans the counts, writes each row in traversal order into a temporary, and then gives every ENTRY a
// thread that counts the entries of its row below it under (d2, j): no two entries of a row share a j, so these ranks
// are a permutation of the row, whatever order the buckets were traversed in.
#include <math.h>

#include "icp_internal.h"
#include "icp_knn_device.h"

namespace thip {

// Bucket of offset o (0 .. 26; x fastest) around the cell (c0, c1, c2); -1: the cell lies outside the grid.
__device__ __forceinline__ int32_t icp_search_bucket(const IcpDesc& d, int64_t c0, int64_t c1, int64_t c2, int o) {
  const int64_t cx = c0 + (o % 3 - 1), cy = c1 + (o / 3 % 3 - 1), cz = c2 + (o / 9 - 1);
  const bool inside = cx >= 0 && cy >= 0 && cz >= 0 && cx <= d.cmax[0] && cy <= d.cmax[1] && cz <= d.cmax[2];
  return inside ? (int32_t)icp_bucket(cx, cy, cz, d.tb_mask) : -1;  // tb_mask < 2^31
}

// Offset o is visited: its cell lies inside the grid and no earlier offset has its bucket.
__device__ __forceinline__ bool icp_search_fresh(const IcpDesc& d, int64_t c0, int64_t c1, int64_t c2, int o,
                                                 int32_t bk) {
  if (bk < 0) return false;
  for (int e = 0; e < o; ++e)
    if (icp_search_bucket(d, c0, c1, c2, e) == bk) return false;
  return true;
}

__device__ __forceinline__ double icp_search_d2(const double (&x)[3], const double* __restrict__ y) {
  const double e0 = x[0] - y[0], e1 = x[1] - y[1], e2 = x[2] - y[2];
  return (e0 * e0 + e1 * e1) + e2 * e2;
}

// The lane's finished list into row `base` of the n_query x k outputs.
__device__ __forceinline__ void icp_search_store_row(const double (*ld)[kIcpCovBlock], const int32_t (*lj)[kIcpCovBlock],
                                                     int lane, int m, int k, int64_t base, int32_t* __restrict__ idx_out,
                                                     double* __restrict__ d2_out) {
  for (int t = 0; t < k; ++t) {
    idx_out[base + t] = t < m ? lj[t][lane] : -1;
    d2_out[base + t] = t < m ? ld[t][lane] : INFINITY;
  }
}

// ---- k-NN ---------------------------------------------------------------------------------------------------------
template <int CAP>
__device__ __forceinline__ void icp_search_ring(double (*ld)[kIcpCovBlock], int32_t (*lj)[kIcpCovBlock],
                                                const IcpDesc* __restrict__ descs,
                                                const IcpSearchDesc* __restrict__ sds,
                                                const int32_t* __restrict__ blk_prob, const double* __restrict__ xq,
                                                const double* __restrict__ qs, const int32_t* __restrict__ qj,
                                                const int32_t* __restrict__ bstart, int32_t* __restrict__ idx_out,
                                                double* __restrict__ d2_out, int32_t* __restrict__ work,
                                                int32_t* __restrict__ work_count) {
  const int p = blk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const IcpSearchDesc& sd = sds[p];
  const int lane = threadIdx.x;
  const int64_t i = (int64_t)((int)blockIdx.x - d.blk_off) * kIcpCovBlock + lane;
  if (i >= d.n_s) return;
  const int64_t base = sd.out_off + i * sd.k;
  if (d.n_t == 0) {  // no data, no grid
    icp_search_store_row(ld, lj, lane, 0, sd.k, base, idx_out, d2_out);
    return;
  }
  int want = sd.k < d.n_t ? sd.k : d.n_t;
  want = want < CAP ? want : CAP;  // the launcher picks CAP >= every want: list indices stay inside
  const double* xp = xq + 3 * (d.s_off + i);
  const double x[3] = {xp[0], xp[1], xp[2]};
  const int64_t c0 = icp_cell(x[0], d.origin[0], d.inv_h), c1 = icp_cell(x[1], d.origin[1], d.inv_h),
                c2 = icp_cell(x[2], d.origin[2], d.inv_h);
  // r0: the Chebyshev distance from the cell to the box [0, cmax]; rings below it hold no cell of the grid
  int64_t r0 = 0;
  r0 = -c0 > r0 ? -c0 : r0;
  r0 = -c1 > r0 ? -c1 : r0;
  r0 = -c2 > r0 ? -c2 : r0;
  r0 = c0 - d.cmax[0] > r0 ? c0 - d.cmax[0] : r0;
  r0 = c1 - d.cmax[1] > r0 ? c1 - d.cmax[1] : r0;
  r0 = c2 - d.cmax[2] > r0 ? c2 - d.cmax[2] : r0;
  int m = 0;
  bool done = false;
  if (r0 <= kIcpSearchR0Max) {  // every offset below is at most kIcpSearchR0Max + kIcpKnnRingCapMax
    for (int t = 0; t < sd.ring_cap && !done; ++t) {
      const int r = (int)r0 + t;
      // ring r cut to the box: the offsets whose cell lies in [0, cmax], per axis
      const int zlo = -c2 > -r ? (int)-c2 : -r, zhi = d.cmax[2] - c2 < r ? (int)(d.cmax[2] - c2) : r;
      const int ylo = -c1 > -r ? (int)-c1 : -r, yhi = d.cmax[1] - c1 < r ? (int)(d.cmax[1] - c1) : r;
      const int xlo = -c0 > -r ? (int)-c0 : -r, xhi = d.cmax[0] - c0 < r ? (int)(d.cmax[0] - c0) : r;
      for (int dz = zlo; dz <= zhi; ++dz) {
        for (int dy = ylo; dy <= yhi; ++dy) {
          // on the shell's z or y faces every dx belongs to ring r; elsewhere only dx = -r and dx = r
          const bool face = dz == -r || dz == r || dy == -r || dy == r;
          const int step = face ? 1 : 2 * r;  // r > 0 off the faces
          for (int dx = face ? xlo : -r; dx <= xhi; dx += step) {
            if (dx < xlo) continue;
            const int64_t b = d.b_off + icp_bucket(c0 + dx, c1 + dy, c2 + dz, d.tb_mask);
            const int32_t k1 = bstart[b + 1];
            for (int32_t k = bstart[b]; k < k1; ++k)
              icp_knn_insert<CAP>(ld, lj, lane, want, m, icp_search_d2(x, qs + 3 * (int64_t)k), qj[k]);
          }
        }
      }
      const double rh = (double)r * sd.edge;
      const bool covered = c0 - r <= 0 && c1 - r <= 0 && c2 - r <= 0 && c0 + r >= d.cmax[0] && c1 + r >= d.cmax[1] &&
                           c2 + r >= d.cmax[2];
      done = covered || (m == want && ld[want - 1][lane] <= rh * rh);
    }
  }
  if (!done) {  // the whole-cloud route finishes this query
    const int32_t w = atomicAdd(work_count, 1);
    work[2 * (int64_t)w] = p;
    work[2 * (int64_t)w + 1] = (int32_t)i;
    return;
  }
  icp_search_store_row(ld, lj, lane, m, sd.k, base, idx_out, d2_out);
}

template <int CAP>
__global__ __launch_bounds__(kIcpCovBlock) void icp_search_ring_kernel(
    const IcpDesc* __restrict__ descs, const IcpSearchDesc* __restrict__ sds, const int32_t* __restrict__ blk_prob,
    const double* __restrict__ xq, const double* __restrict__ qs, const int32_t* __restrict__ qj,
    const int32_t* __restrict__ bstart, int32_t* __restrict__ idx_out, double* __restrict__ d2_out,
    int32_t* __restrict__ work, int32_t* __restrict__ work_count) {
  __shared__ double ld[CAP][kIcpCovBlock];  // slot-major: lane l owns ld[.][l]
  __shared__ int32_t lj[CAP][kIcpCovBlock];
  icp_search_ring<CAP>(ld, lj, descs, sds, blk_prob, xq, qs, qj, bstart, idx_out, d2_out, work, work_count);
}

// The whole-cloud route: icp_knn_scan (icp_knn_device.h) with the query taken from xq and the rows as the sink.
template <int CAP>
__global__ __launch_bounds__(kIcpCovBlock) void icp_search_scan_kernel(
    const IcpDesc* __restrict__ descs, const IcpSearchDesc* __restrict__ sds, const double* __restrict__ xq,
    const double* __restrict__ q, int32_t* __restrict__ idx_out, double* __restrict__ d2_out,
    const int32_t* __restrict__ work, const int32_t* __restrict__ work_count) {
  __shared__ double ld[CAP][kIcpCovBlock];
  __shared__ int32_t lj[CAP][kIcpCovBlock];
  const IcpKnnListOut out = {idx_out, d2_out, nullptr};
  icp_knn_scan<CAP>(ld, lj, descs, sds, IcpKnnCloudQuery{xq}, q, out, work, work_count);
}

// ---- hybrid -------------------------------------------------------------------------------------------------------
template <int CAP>
__global__ __launch_bounds__(kIcpCovBlock) void icp_search_hybrid_kernel(
    const IcpDesc* __restrict__ descs, const IcpSearchDesc* __restrict__ sds, const int32_t* __restrict__ blk_prob,
    const double* __restrict__ xq, const double* __restrict__ qs, const int32_t* __restrict__ qj,
    const int32_t* __restrict__ bstart, int32_t* __restrict__ idx_out, double* __restrict__ d2_out,
    int32_t* __restrict__ cnt_out) {
  __shared__ double ld[CAP][kIcpCovBlock];
  __shared__ int32_t lj[CAP][kIcpCovBlock];
  const int p = blk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const IcpSearchDesc& sd = sds[p];
  const int lane = threadIdx.x;
  const int64_t i = (int64_t)((int)blockIdx.x - d.blk_off) * kIcpCovBlock + lane;
  if (i >= d.n_s) return;
  const int cap = sd.k < CAP ? sd.k : CAP;  // the launcher picks CAP >= every max_nn
  int m = 0;
  if (d.n_t > 0) {
    const double* xp = xq + 3 * (d.s_off + i);
    const double x[3] = {xp[0], xp[1], xp[2]};
    const int64_t c0 = icp_cell(x[0], d.origin[0], d.inv_h), c1 = icp_cell(x[1], d.origin[1], d.inv_h),
                  c2 = icp_cell(x[2], d.origin[2], d.inv_h);
    const double r2 = d.r2;
    for (int o = 0; o < 27; ++o) {
      const int32_t bk = icp_search_bucket(d, c0, c1, c2, o);
      if (!icp_search_fresh(d, c0, c1, c2, o, bk)) continue;
      const int64_t b = d.b_off + bk;
      const int32_t k1 = bstart[b + 1];
      for (int32_t k = bstart[b]; k < k1; ++k) {
        const double d2 = icp_search_d2(x, qs + 3 * (int64_t)k);
        if (d2 < r2) icp_knn_insert<CAP>(ld, lj, lane, cap, m, d2, qj[k]);
      }
    }
  }
  icp_search_store_row(ld, lj, lane, m, sd.k, sd.out_off + i * sd.k, idx_out, d2_out);
  cnt_out[d.s_off + i] = m;
}

// ---- radius -------------------------------------------------------------------------------------------------------
// The gather both passes share, one query per thread.  kFill 0: the number of j with d2 < r2.  kFill 1: the same
// traversal, entry t of the row to slot at + t of tmp_d2 / tmp_j.
template <int kFill>
__device__ __forceinline__ int32_t icp_search_gather(const IcpDesc& d, const double (&x)[3],
                                                     const double* __restrict__ qs, const int32_t* __restrict__ qj,
                                                     const int32_t* __restrict__ bstart, int64_t at,
                                                     double* __restrict__ tmp_d2, int32_t* __restrict__ tmp_j) {
  const int64_t c0 = icp_cell(x[0], d.origin[0], d.inv_h), c1 = icp_cell(x[1], d.origin[1], d.inv_h),
                c2 = icp_cell(x[2], d.origin[2], d.inv_h);
  const double r2 = d.r2;
  int32_t cnt = 0;
  for (int o = 0; o < 27; ++o) {
    const int32_t bk = icp_search_bucket(d, c0, c1, c2, o);
    if (!icp_search_fresh(d, c0, c1, c2, o, bk)) continue;
    const int64_t b = d.b_off + bk;
    const int32_t k1 = bstart[b + 1];
    for (int32_t k = bstart[b]; k < k1; ++k) {
      const double d2 = icp_search_d2(x, qs + 3 * (int64_t)k);
      if (!(d2 < r2)) continue;
      if (kFill) {
        tmp_d2[at + cnt] = d2;
        tmp_j[at + cnt] = qj[k];
      }
      ++cnt;
    }
  }
  return cnt;
}

__global__ __launch_bounds__(256) void icp_search_count_kernel(
    const IcpDesc* __restrict__ descs, const int32_t* __restrict__ blk_prob, const double* __restrict__ xq,
    const double* __restrict__ qs, const int32_t* __restrict__ bstart, int32_t* __restrict__ count) {
  const int p = blk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const int64_t i = (int64_t)((int)blockIdx.x - d.blk_off) * 256 + threadIdx.x;
  if (i >= d.n_s) return;
  int32_t cnt = 0;
  if (d.n_t > 0) {
    const double* xp = xq + 3 * (d.s_off + i);
    const double x[3] = {xp[0], xp[1], xp[2]};
    cnt = icp_search_gather<0>(d, x, qs, nullptr, bstart, 0, nullptr, nullptr);
  }
  count[d.s_off + i] = cnt;
}

// One block per problem: prefix[s_off + i] = the exclusive sum of the problem's counts, total[p] = their sum.
__global__ __launch_bounds__(kIcpScanThreads) void icp_search_prefix_kernel(const IcpDesc* __restrict__ descs,
                                                                            const int32_t* __restrict__ count,
                                                                            int64_t* __restrict__ prefix,
                                                                            int64_t* __restrict__ total) {
  __shared__ int64_t s[kIcpScanThreads];
  const IcpDesc& d = descs[blockIdx.x];
  const int64_t n = d.n_s;
  const int64_t chunk = (n + kIcpScanThreads - 1) / kIcpScanThreads;
  const int64_t lo0 = (int64_t)threadIdx.x * chunk;
  const int64_t lo = lo0 < n ? lo0 : n, hi = lo + chunk < n ? lo + chunk : n;
  int64_t sum = 0;
  for (int64_t k = lo; k < hi; ++k) sum += count[d.s_off + k];
  s[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < kIcpScanThreads; o <<= 1) {  // inclusive Hillis-Steele scan of the per-thread sums
    const int64_t add = threadIdx.x >= (unsigned)o ? s[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  int64_t run = s[threadIdx.x] - sum;
  for (int64_t k = lo; k < hi; ++k) {
    prefix[d.s_off + k] = run;
    run += count[d.s_off + k];
  }
  if (threadIdx.x == kIcpScanThreads - 1) total[blockIdx.x] = s[threadIdx.x];
}

// A problem is filled when the caller gave arrays and they hold its total.
__device__ __forceinline__ bool icp_search_filled(const IcpSearchDesc& sd, int64_t total) {
  return sd.fill != 0 && sd.capacity >= total;
}

__global__ __launch_bounds__(256) void icp_search_fill_kernel(
    const IcpDesc* __restrict__ descs, const IcpSearchDesc* __restrict__ sds, const int32_t* __restrict__ blk_prob,
    const double* __restrict__ xq, const double* __restrict__ qs, const int32_t* __restrict__ qj,
    const int32_t* __restrict__ bstart, const int64_t* __restrict__ prefix, const int64_t* __restrict__ total,
    double* __restrict__ tmp_d2, int32_t* __restrict__ tmp_j) {
  const int p = blk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const IcpSearchDesc& sd = sds[p];
  const int64_t i = (int64_t)((int)blockIdx.x - d.blk_off) * 256 + threadIdx.x;
  if (i >= d.n_s || d.n_t == 0 || !icp_search_filled(sd, total[p])) return;
  const double* xp = xq + 3 * (d.s_off + i);
  const double x[3] = {xp[0], xp[1], xp[2]};
  // the same traversal as the count pass: prefix[i] + count[i] <= total <= the entries reserved for the problem
  icp_search_gather<1>(d, x, qs, qj, bstart, sd.out_off + prefix[d.s_off + i], tmp_d2, tmp_j);
}

// One thread per entry e of the reserved range: its problem (the last one whose range begins at or before e), its row
// (the last one whose prefix is at or below e's place in the problem), its rank in the row, and the store.
__global__ __launch_bounds__(256) void icp_search_rank_kernel(
    const IcpDesc* __restrict__ descs, const IcpSearchDesc* __restrict__ sds, int batch, int64_t entries,
    const int32_t* __restrict__ count, const int64_t* __restrict__ prefix, const int64_t* __restrict__ total,
    const double* __restrict__ tmp_d2, const int32_t* __restrict__ tmp_j, int32_t* __restrict__ idx_out,
    double* __restrict__ d2_out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  int p = 0;
  for (int hi = batch; hi - p > 1;) {
    const int mid = p + (hi - p) / 2;
    if (sds[mid].out_off <= e) p = mid; else hi = mid;
  }
  const IcpDesc& d = descs[p];
  const IcpSearchDesc& sd = sds[p];
  const int64_t el = e - sd.out_off, tot = total[p];
  if (!icp_search_filled(sd, tot) || el >= tot) return;  // tot > 0 from here on, so n_s > 0
  const int64_t* pre = prefix + d.s_off;
  int64_t i = 0;
  for (int64_t hi = d.n_s; hi - i > 1;) {
    const int64_t mid = i + (hi - i) / 2;
    if (pre[mid] <= el) i = mid; else hi = mid;
  }
  const int64_t row = sd.out_off + pre[i];
  const int32_t m = count[d.s_off + i];
  const double md = tmp_d2[e];
  const int32_t mj = tmp_j[e];
  int32_t rank = 0;
  for (int32_t t = 0; t < m; ++t) {
    const double od = tmp_d2[row + t];
    rank += (od < md || (od == md && tmp_j[row + t] < mj)) ? 1 : 0;
  }
  idx_out[row + rank] = mj;  // rank < m: the entry does not precede itself
  d2_out[row + rank] = md;
}

// ---- launchers ------------------------------------------------------------------------------------------------
void launch_icp_search_knn(hipStream_t s, const IcpDesc* d_desc, const IcpSearchDesc* d_sd, const int32_t* d_blk_prob,
                           int n_blk, int top_k, const double* d_x, const double* d_q, const double* d_qs,
                           const int32_t* d_qj, const int32_t* d_bstart, int32_t* d_idx, double* d_d2, int32_t* d_work,
                           int32_t* d_work_count) {
  icp_knn_launch(n_blk, top_k, [&](auto cap, dim3 ring, dim3 scan) {
    hipLaunchKernelGGL(icp_search_ring_kernel<cap()>, ring, dim3(kIcpCovBlock), 0, s, d_desc, d_sd, d_blk_prob, d_x,
                       d_qs, d_qj, d_bstart, d_idx, d_d2, d_work, d_work_count);
    hipLaunchKernelGGL(icp_search_scan_kernel<cap()>, scan, dim3(kIcpCovBlock), 0, s, d_desc, d_sd, d_x, d_q, d_idx,
                       d_d2, d_work, d_work_count);
  });
}

void launch_icp_search_hybrid(hipStream_t s, const IcpDesc* d_desc, const IcpSearchDesc* d_sd,
                              const int32_t* d_blk_prob, int n_blk, int top_nn, const double* d_x, const double* d_qs,
                              const int32_t* d_qj, const int32_t* d_bstart, int32_t* d_idx, double* d_d2,
                              int32_t* d_cnt) {
  if (n_blk <= 0) return;
  if (top_nn <= kIcpKnnSmall)
    hipLaunchKernelGGL(icp_search_hybrid_kernel<kIcpKnnSmall>, dim3(n_blk), dim3(kIcpCovBlock), 0, s, d_desc, d_sd,
                       d_blk_prob, d_x, d_qs, d_qj, d_bstart, d_idx, d_d2, d_cnt);
  else
    hipLaunchKernelGGL(icp_search_hybrid_kernel<kIcpKnnMax>, dim3(n_blk), dim3(kIcpCovBlock), 0, s, d_desc, d_sd,
                       d_blk_prob, d_x, d_qs, d_qj, d_bstart, d_idx, d_d2, d_cnt);
}

void launch_icp_search_radius(hipStream_t s, const IcpDesc* d_desc, const IcpSearchDesc* d_sd,
                              const int32_t* d_blk_prob, int n_blk, int batch, int64_t entries, const double* d_x,
                              const double* d_qs, const int32_t* d_qj, const int32_t* d_bstart, int32_t* d_count,
                              int64_t* d_prefix, int64_t* d_total, double* d_tmp_d2, int32_t* d_tmp_j, int32_t* d_idx,
                              double* d_d2) {
  if (n_blk > 0)
    hipLaunchKernelGGL(icp_search_count_kernel, dim3(n_blk), dim3(256), 0, s, d_desc, d_blk_prob, d_x, d_qs, d_bstart,
                       d_count);
  hipLaunchKernelGGL(icp_search_prefix_kernel, dim3(batch), dim3(kIcpScanThreads), 0, s, d_desc, d_count, d_prefix,
                     d_total);
  if (n_blk <= 0 || entries <= 0) return;  // the count half only
  hipLaunchKernelGGL(icp_search_fill_kernel, dim3(n_blk), dim3(256), 0, s, d_desc, d_sd, d_blk_prob, d_x, d_qs, d_qj,
                     d_bstart, d_prefix, d_total, d_tmp_d2, d_tmp_j);
  hipLaunchKernelGGL(icp_search_rank_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, d_desc, d_sd,
                     batch, entries, d_count, d_prefix, d_total, d_tmp_d2, d_tmp_j, d_idx, d_d2);
}

}  // namespace thip
