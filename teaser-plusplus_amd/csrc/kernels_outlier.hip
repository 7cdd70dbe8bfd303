// kernels_outlier.hip -- self k-nearest-neighbours without a radius, and statistical / radius outlier removal
// (Open3D's remove_statistical_outlier / remove_radius_outlier) for gfx950, on the hash grid of kernels_icp.hip.  The
// contracts are written out in include/teaser_hip.h ("Self k-NN", "Outlier removal"), the design in DESIGN.md section 17.
//
// Self k-NN: the grid of a cloud is built with a cell edge chosen on the host from the bounding box, n and k (a cell
// holds O(k) points) instead of from a radius.  icp_knn_ring_kernel gives one query to one lane and keeps the
// min(k, n) smallest (d2, j) in a per-lane insertion-sorted list in LDS (slot-major, as icp_cov_kernel), visiting the
// cells ring by ring: ring r is the shell of cells at Chebyshev offset r.  After ring r every point not yet seen
// lies more than r cell edges away (its cell differs by more than r on some axis), so a full list whose last d2 is at
// most (r h)^2, h below the cell edge by set_grid's margin, is final.  A query also ends when the rings have covered
// the whole grid.  A query that is still open after IcpKnnDesc::ring_cap rings (a far outlier) goes on a worklist and
// icp_knn_scan_kernel serves it: one wave per query, every lane keeps the list of its stride of the WHOLE cloud, and
// the 64 lists are merged by repeated wave-wide minima of (d2, j).  Both routes produce the min(k, n) smallest
// (d2, j) of the cloud exactly and consume them in that order, so the route never shows in a result.
//
// Hash collisions bring points of other cells into a visited bucket and make a bucket reachable twice: a candidate is
// a real point of the cloud with its true d2 either way, and a repeated (d2, j) is recognised at its place in the
// list (or lies beyond a full list's end, like the first time).
#include <math.h>

#include "icp_internal.h"
#include "icp_knn_device.h"

namespace thip {

// icp_knn_insert, the per-lane list: icp_cov_device.h.  What the kernels do with a query's finished neighbours, in
// ascending (d2, j), is the template argument Out (icp_knn_device.h): IcpKnnListOut writes them (avg == nullptr) or
// the mean of their distances (statistical removal); IcpKnnNormalOut feeds them to the covariance sums of normal
// estimation.  The ring walk is written out here; the scan is icp_knn_scan of that header.
template <int CAP, class Out>
__device__ __forceinline__ void icp_knn_ring(double (*ld)[kIcpCovBlock], int32_t (*lj)[kIcpCovBlock],
                                             const IcpDesc* __restrict__ descs, const IcpKnnDesc* __restrict__ knns,
                                             const int32_t* __restrict__ blk_prob, const double* __restrict__ q,
                                             const double* __restrict__ qs, const int32_t* __restrict__ qj,
                                             const int32_t* __restrict__ bstart, const Out& out,
                                             int32_t* __restrict__ work, int32_t* __restrict__ work_count) {
  const int p = blk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const IcpKnnDesc& kd = knns[p];
  const int lane = threadIdx.x;
  const int64_t i = (int64_t)((int)blockIdx.x - d.blk_off) * kIcpCovBlock + lane;
  if (i >= d.n_t) return;
  int want = kd.k < d.n_t ? kd.k : d.n_t;
  want = want < CAP ? want : CAP;  // the launcher picks CAP >= every want: list indices stay inside
  const double* xp = q + 3 * (d.t_off + i);
  const double x[3] = {xp[0], xp[1], xp[2]};
  const int64_t c0 = icp_cell(x[0], d.origin[0], d.inv_h), c1 = icp_cell(x[1], d.origin[1], d.inv_h),
                c2 = icp_cell(x[2], d.origin[2], d.inv_h);
  int m = 0;
  bool done = false;
  for (int r = 0; r < kd.ring_cap && !done; ++r) {
    for (int dz = -r; dz <= r; ++dz) {
      const int64_t cz = c2 + dz;
      if (cz < 0 || cz > d.cmax[2]) continue;  // every point of the cloud lies in [0, cmax]
      for (int dy = -r; dy <= r; ++dy) {
        const int64_t cy = c1 + dy;
        if (cy < 0 || cy > d.cmax[1]) continue;
        // on the shell's z or y faces every dx belongs to ring r; elsewhere only dx = -r and dx = r
        const bool face = dz == -r || dz == r || dy == -r || dy == r;
        const int step = face || r == 0 ? 1 : 2 * r;
        for (int dx = -r; dx <= r; dx += step) {
          const int64_t cx = c0 + dx;
          if (cx < 0 || cx > d.cmax[0]) continue;
          const int64_t b = d.b_off + icp_bucket(cx, cy, cz, d.tb_mask);
          const int32_t k1 = bstart[b + 1];
          for (int32_t k = bstart[b]; k < k1; ++k) {
            const double e0 = x[0] - qs[3 * (int64_t)k], e1 = x[1] - qs[3 * (int64_t)k + 1],
                         e2 = x[2] - qs[3 * (int64_t)k + 2];
            const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
            icp_knn_insert<CAP>(ld, lj, lane, want, m, d2, qj[k]);
          }
        }
      }
    }
    const double rh = (double)r * kd.edge;
    const bool covered = c0 - r <= 0 && c1 - r <= 0 && c2 - r <= 0 && c0 + r >= d.cmax[0] && c1 + r >= d.cmax[1] &&
                         c2 + r >= d.cmax[2];
    done = covered || (m == want && ld[want - 1][lane] <= rh * rh);
  }
  if (!done) {  // the whole-cloud route finishes this query
    const int32_t w = atomicAdd(work_count, 1);
    work[2 * (int64_t)w] = p;
    work[2 * (int64_t)w + 1] = (int32_t)i;
    return;
  }
  if constexpr (Out::kNormals) {  // the list in ascending (d2, j) into the sums of the covariance contract
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (m >= 3) icp_list_cov(lj, lane, m, q + 3 * d.t_off, x, a);
    icp_normal_store(out, out.nd[p], i, x, m, a);
  } else {
    int32_t* __restrict__ idx_out = out.idx;
    double* __restrict__ d2_out = out.d2;
    double* __restrict__ avg_out = out.avg;
    if (avg_out) {  // statistical removal: the distances one at a time in ascending (d2, j), from 0.0
      double acc = 0.0;
      for (int t = 0; t < m; ++t) acc += sqrt(ld[t][lane]);
      avg_out[d.t_off + i] = acc / (double)m;
    } else {
      const int64_t base = kd.out_off + i * kd.k;
      for (int t = 0; t < kd.k; ++t) {
        idx_out[base + t] = t < m ? lj[t][lane] : -1;
        d2_out[base + t] = t < m ? ld[t][lane] : INFINITY;
      }
    }
  }
}

template <int CAP>
__global__ __launch_bounds__(kIcpCovBlock) void icp_knn_ring_kernel(
    const IcpDesc* __restrict__ descs, const IcpKnnDesc* __restrict__ knns, const int32_t* __restrict__ blk_prob,
    const double* __restrict__ q, const double* __restrict__ qs, const int32_t* __restrict__ qj,
    const int32_t* __restrict__ bstart, int32_t* __restrict__ idx_out, double* __restrict__ d2_out,
    double* __restrict__ avg_out, int32_t* __restrict__ work, int32_t* __restrict__ work_count) {
  __shared__ double ld[CAP][kIcpCovBlock];  // slot-major: lane l owns ld[.][l]
  __shared__ int32_t lj[CAP][kIcpCovBlock];
  const IcpKnnListOut out = {idx_out, d2_out, avg_out};
  icp_knn_ring<CAP>(ld, lj, descs, knns, blk_prob, q, qs, qj, bstart, out, work, work_count);
}

template <int CAP>
__global__ __launch_bounds__(kIcpCovBlock) void icp_knn_ring_normals_kernel(
    const IcpDesc* __restrict__ descs, const IcpKnnDesc* __restrict__ knns, const int32_t* __restrict__ blk_prob,
    const double* __restrict__ q, const double* __restrict__ qs, const int32_t* __restrict__ qj,
    const int32_t* __restrict__ bstart, const IcpKnnNormalOut out, int32_t* __restrict__ work,
    int32_t* __restrict__ work_count) {
  __shared__ double ld[CAP][kIcpCovBlock];
  __shared__ int32_t lj[CAP][kIcpCovBlock];
  icp_knn_ring<CAP>(ld, lj, descs, knns, blk_prob, q, qs, qj, bstart, out, work, work_count);
}

// The whole-cloud route: icp_knn_scan (icp_knn_device.h) with the query a point of the cloud.
template <int CAP>
__global__ __launch_bounds__(kIcpCovBlock) void icp_knn_scan_kernel(
    const IcpDesc* __restrict__ descs, const IcpKnnDesc* __restrict__ knns, const double* __restrict__ q,
    int32_t* __restrict__ idx_out, double* __restrict__ d2_out, double* __restrict__ avg_out,
    const int32_t* __restrict__ work, const int32_t* __restrict__ work_count) {
  __shared__ double ld[CAP][kIcpCovBlock];
  __shared__ int32_t lj[CAP][kIcpCovBlock];
  const IcpKnnListOut out = {idx_out, d2_out, avg_out};
  icp_knn_scan<CAP>(ld, lj, descs, knns, IcpKnnSelfQuery{q}, q, out, work, work_count);
}

template <int CAP>
__global__ __launch_bounds__(kIcpCovBlock) void icp_knn_scan_normals_kernel(
    const IcpDesc* __restrict__ descs, const IcpKnnDesc* __restrict__ knns, const double* __restrict__ q,
    const IcpKnnNormalOut out, const int32_t* __restrict__ work, const int32_t* __restrict__ work_count) {
  __shared__ double ld[CAP][kIcpCovBlock];
  __shared__ int32_t lj[CAP][kIcpCovBlock];
  icp_knn_scan<CAP>(ld, lj, descs, knns, IcpKnnSelfQuery{q}, q, out, work, work_count);
}

// ---- statistical removal: mean, std, threshold, mask -----------------------------------------------------------
// One thread per block of 256 consecutive points: the block's sum in ascending index from 0.0 over the points with
// avg > 0; kPass 0: of avg, kPass 1: of (avg - mean)^2.
template <int kPass>
__global__ __launch_bounds__(256) void icp_stat_block_kernel(const IcpDesc* __restrict__ descs,
                                                             const int32_t* __restrict__ tblk_prob, int n_tblk,
                                                             const double* __restrict__ avg,
                                                             const double* __restrict__ stats,
                                                             double* __restrict__ partials) {
  const int t = (int)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tblk) return;
  const int p = tblk_prob[t];
  const IcpDesc& d = descs[p];
  const int64_t lo = (int64_t)(t - d.tblk_off) * 256;
  const int64_t hi = lo + 256 < d.n_t ? lo + 256 : d.n_t;
  const double mean = kPass ? stats[3 * (int64_t)p] : 0.0;
  double s = 0.0;
  for (int64_t i = lo; i < hi; ++i) {
    const double a = avg[d.t_off + i];
    if (!(a > 0.0)) continue;
    if (kPass) {
      const double e = a - mean;
      s += e * e;
    } else {
      s += a;
    }
  }
  partials[t] = s;
}

// One thread per cloud: the block sums in ascending block order from 0.0, then mean (kPass 0) or std and threshold.
template <int kPass>
__global__ __launch_bounds__(256) void icp_stat_reduce_kernel(const IcpDesc* __restrict__ descs,
                                                              const IcpKnnDesc* __restrict__ knns, int batch,
                                                              const double* __restrict__ partials,
                                                              double* __restrict__ stats) {
  const int p = (int)blockIdx.x * 256 + threadIdx.x;
  if (p >= batch) return;
  const IcpDesc& d = descs[p];
  if (d.n_t == 0) return;
  const int nb = (d.n_t + 255) / 256;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += partials[d.tblk_off + b];
  const double valid = (double)d.n_t;
  double* st = stats + 3 * (int64_t)p;
  if (kPass == 0) {
    st[0] = s / valid;
  } else {
    const double sd = sqrt(s / (valid - 1.0));
    st[1] = sd;
    st[2] = st[0] + knns[p].ratio * sd;
  }
}

__global__ __launch_bounds__(256) void icp_stat_keep_kernel(const IcpDesc* __restrict__ descs,
                                                            const int32_t* __restrict__ tblk_prob,
                                                            const double* __restrict__ avg,
                                                            const double* __restrict__ stats,
                                                            uint8_t* __restrict__ keep, int32_t* __restrict__ kept) {
  const int p = tblk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const int64_t i = (int64_t)((int)blockIdx.x - d.tblk_off) * 256 + threadIdx.x;
  bool k = false;
  if (i < d.n_t) {
    const double a = avg[d.t_off + i];
    k = a > 0.0 && a < stats[3 * (int64_t)p + 2];
    keep[d.t_off + i] = k ? 1 : 0;
  }
  const unsigned long long bal = __ballot(k);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&kept[p], (int32_t)__popcll(bal));
}

// ---- radius removal ---------------------------------------------------------------------------------------------
// count[i] = |{j : d2(i, j) < r2}| over the buckets of the 27 cells around i's cell of the grid built for r.  Every
// point closer than r lies in one of those cells, hence in one of those buckets; a bucket is visited once -- an offset
// whose bucket equals that of an earlier visited offset is skipped -- so a point is counted once, and a point of a
// foreign cell that shares a bucket counts like any other when its d2 < r2.  The 27 bucket ids are kept in registers:
// the offset loop is fully unrolled, every index below is a compile-time constant.
__global__ __launch_bounds__(256) void icp_radius_count_kernel(
    const IcpDesc* __restrict__ descs, const IcpKnnDesc* __restrict__ knns, const int32_t* __restrict__ tblk_prob,
    const double* __restrict__ q, const double* __restrict__ qs, const int32_t* __restrict__ bstart,
    int32_t* __restrict__ count, uint8_t* __restrict__ keep, int32_t* __restrict__ kept) {
  const int p = tblk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const int64_t i = (int64_t)((int)blockIdx.x - d.tblk_off) * 256 + threadIdx.x;
  bool k = false;
  if (i < d.n_t) {
    const double* xp = q + 3 * (d.t_off + i);
    const double x[3] = {xp[0], xp[1], xp[2]};
    const int64_t c0 = icp_cell(x[0], d.origin[0], d.inv_h), c1 = icp_cell(x[1], d.origin[1], d.inv_h),
                  c2 = icp_cell(x[2], d.origin[2], d.inv_h);
    const double r2 = d.r2;
    int32_t cnt = 0;
    int32_t seen[27];  // bucket of offset o, -1 when the cell lies outside the grid (tb_mask < 2^31)
#pragma unroll
    for (int o = 0; o < 27; ++o) {
      const int64_t cx = c0 + (o % 3 - 1), cy = c1 + (o / 3 % 3 - 1), cz = c2 + (o / 9 - 1);
      const bool inside = cx >= 0 && cy >= 0 && cz >= 0 && cx <= d.cmax[0] && cy <= d.cmax[1] && cz <= d.cmax[2];
      const int32_t bk = inside ? (int32_t)icp_bucket(cx, cy, cz, d.tb_mask) : -1;
      seen[o] = bk;
      bool fresh = inside;
#pragma unroll
      for (int e = 0; e < o; ++e) fresh = fresh && seen[e] != bk;
      if (!fresh) continue;
      const int64_t b = d.b_off + bk;
      const int32_t k1 = bstart[b + 1];
      for (int32_t s = bstart[b]; s < k1; ++s) {
        const double e0 = x[0] - qs[3 * (int64_t)s], e1 = x[1] - qs[3 * (int64_t)s + 1],
                     e2 = x[2] - qs[3 * (int64_t)s + 2];
        const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
        if (d2 < r2) ++cnt;
      }
    }
    count[d.t_off + i] = cnt;
    k = cnt > knns[p].k;
    keep[d.t_off + i] = k ? 1 : 0;
  }
  const unsigned long long bal = __ballot(k);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&kept[p], (int32_t)__popcll(bal));
}

// ---- launchers ------------------------------------------------------------------------------------------------
void launch_icp_self_knn(hipStream_t s, const IcpDesc* d_desc, const IcpKnnDesc* d_knn, const int32_t* d_blk_prob,
                         int n_blk, int top_k, const double* d_q, const double* d_qs, const int32_t* d_qj,
                         const int32_t* d_bstart, int32_t* d_idx, double* d_d2, double* d_avg, int32_t* d_work,
                         int32_t* d_work_count) {
  icp_knn_launch(n_blk, top_k, [&](auto cap, dim3 ring, dim3 scan) {
    hipLaunchKernelGGL(icp_knn_ring_kernel<cap()>, ring, dim3(kIcpCovBlock), 0, s, d_desc, d_knn, d_blk_prob, d_q,
                       d_qs, d_qj, d_bstart, d_idx, d_d2, d_avg, d_work, d_work_count);
    hipLaunchKernelGGL(icp_knn_scan_kernel<cap()>, scan, dim3(kIcpCovBlock), 0, s, d_desc, d_knn, d_q, d_idx, d_d2,
                       d_avg, d_work, d_work_count);
  });
}

void launch_icp_normals_knn(hipStream_t s, const IcpDesc* d_desc, const IcpKnnDesc* d_knn, const IcpNormalDesc* d_nd,
                            const int32_t* d_blk_prob, int n_blk, int top_k, const double* d_q, const double* d_qs,
                            const int32_t* d_qj, const int32_t* d_bstart, double* d_nrm, double* d_cov, double* d_eig,
                            int32_t* d_work, int32_t* d_work_count) {
  IcpKnnNormalOut out;
  out.nd = d_nd, out.nrm = d_nrm, out.cov = d_cov, out.eig = d_eig;
  icp_knn_launch(n_blk, top_k, [&](auto cap, dim3 ring, dim3 scan) {
    hipLaunchKernelGGL(icp_knn_ring_normals_kernel<cap()>, ring, dim3(kIcpCovBlock), 0, s, d_desc, d_knn, d_blk_prob,
                       d_q, d_qs, d_qj, d_bstart, out, d_work, d_work_count);
    hipLaunchKernelGGL(icp_knn_scan_normals_kernel<cap()>, scan, dim3(kIcpCovBlock), 0, s, d_desc, d_knn, d_q, out,
                       d_work, d_work_count);
  });
}

void launch_icp_statistical(hipStream_t s, const IcpDesc* d_desc, const IcpKnnDesc* d_knn,
                            const int32_t* d_tblk_prob, int n_tblk, int batch, const double* d_avg,
                            double* d_partials, double* d_stats, uint8_t* d_keep, int32_t* d_kept) {
  if (n_tblk <= 0) return;
  const dim3 gb((n_tblk + 255) / 256), gp((batch + 255) / 256);
  hipLaunchKernelGGL(icp_stat_block_kernel<0>, gb, dim3(256), 0, s, d_desc, d_tblk_prob, n_tblk, d_avg, d_stats,
                     d_partials);
  hipLaunchKernelGGL(icp_stat_reduce_kernel<0>, gp, dim3(256), 0, s, d_desc, d_knn, batch, d_partials, d_stats);
  hipLaunchKernelGGL(icp_stat_block_kernel<1>, gb, dim3(256), 0, s, d_desc, d_tblk_prob, n_tblk, d_avg, d_stats,
                     d_partials);
  hipLaunchKernelGGL(icp_stat_reduce_kernel<1>, gp, dim3(256), 0, s, d_desc, d_knn, batch, d_partials, d_stats);
  hipLaunchKernelGGL(icp_stat_keep_kernel, dim3(n_tblk), dim3(256), 0, s, d_desc, d_tblk_prob, d_avg, d_stats, d_keep,
                     d_kept);
}

void launch_icp_radius_count(hipStream_t s, const IcpDesc* d_desc, const IcpKnnDesc* d_knn,
                             const int32_t* d_tblk_prob, int n_tblk, const double* d_q, const double* d_qs,
                             const int32_t* d_bstart, int32_t* d_count, uint8_t* d_keep, int32_t* d_kept) {
  if (n_tblk <= 0) return;
  hipLaunchKernelGGL(icp_radius_count_kernel, dim3(n_tblk), dim3(256), 0, s, d_desc, d_knn, d_tblk_prob, d_q, d_qs,
                     d_bstart, d_count, d_keep, d_kept);
}

}  // namespace thip
