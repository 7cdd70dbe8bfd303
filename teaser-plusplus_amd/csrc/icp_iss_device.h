// icp_iss_device.h -- the lane-independent device code of ISS keypoint detection (include/teaser_hip.h, "ISS
// keypoints"; kernels: kernels_keypoints.hip, host side: icp_keypoints.hip, design: DESIGN.md section 19): the
// descriptors, the cell keys of the sorted index, the walk over the 27 cells of a query in ascending key, and the
// bodies of the key, gather, saliency, suppression and resolution kernels.  Nothing here uses a wave operation or LDS,
// so tests/keypoints_host_driver.cpp runs this very source one lane at a time.
//
// The sorted index: every point has one entry per grid (the grid of r_s and the grid of r_n) with the key
// (grid id, c_x, c_y, c_z), c_z in the lowest bits; a stable sort of (key, entry) puts the points of a cell into one
// contiguous run, in ascending point index inside it, and the three z-neighbours of a column next to each other.
// Entry e < total belongs to the grid of r_s of point e, entry total + i to the grid of r_n of point i; the grid id is
// the cloud's index b for r_s and batch + b for r_n, so the sorted entries of cloud b's two grids are the ranges
// [off, off + n) and [total + off, total + off + n).
#pragma once

#include <math.h>

#include "icp_cov_device.h"
#include "icp_internal.h"

namespace thip {

constexpr int kIssBlock = 256;  // queries per block (a block never straddles two clouds)

// One grid of one cloud.  cmax = 0 and inv_h = 0 for a cloud without neighbours (every point in cell 0).
struct IssGrid {
  double origin[3];
  double inv_h;
  double r2;
  int64_t cmax[3];   // largest cell coordinate per axis (the points lie in [0, cmax])
  int64_t base;      // first sorted entry of this grid
  uint64_t id;       // the grid id, already shifted to its place in the key
  int32_t shift[2];  // bit position of c_x and of c_y inside the key (c_z at 0)
};

// One cloud of an ISS call (host-built, read-only on the device).
struct IssDesc {
  int32_t n;
  int32_t min_nb;
  int64_t off;      // first point of this cloud in the packed arrays
  int32_t blk_off;  // first block of this cloud
  int32_t active;   // 0: a radius whose square is not > 0 -- no neighbours, no keypoints, the kernels skip the cloud
  double g21, g32;
  IssGrid gs, gn;   // the grids of r_s and r_n
};

__host__ __device__ inline uint64_t iss_key(const IssGrid& g, int64_t cx, int64_t cy, int64_t cz) {
  return g.id | ((uint64_t)cx << g.shift[0]) | ((uint64_t)cy << g.shift[1]) | (uint64_t)cz;
}

__host__ __device__ inline uint64_t iss_point_key(const IssGrid& g, const double* x) {
  return iss_key(g, icp_cell(x[0], g.origin[0], g.inv_h), icp_cell(x[1], g.origin[1], g.inv_h),
                 icp_cell(x[2], g.origin[2], g.inv_h));
}

// Calls f(e, y) for every sorted entry e of grid g (a cloud of n points) whose point y has d2(x, y) < r2, in ascending
// (c_x, c_y, c_z, point index): the 9 columns around x's cell in ascending (c_x, c_y), inside a column the run of keys
// from c_z - 1 to c_z + 1, found by one lower bound and left at the first larger key.  The cell edge exceeds the radius
// by set_grid's margin, so every such point lies in these cells.
template <class F>
__device__ __forceinline__ void iss_ball(const IssGrid& g, int32_t n, const double (&x)[3],
                                         const uint64_t* __restrict__ skey, const double* __restrict__ spts, F&& f) {
  const int64_t c0 = icp_cell(x[0], g.origin[0], g.inv_h), c1 = icp_cell(x[1], g.origin[1], g.inv_h),
                c2 = icp_cell(x[2], g.origin[2], g.inv_h);
  const int64_t zlo = c2 > 0 ? c2 - 1 : 0, zhi = c2 < g.cmax[2] ? c2 + 1 : g.cmax[2];
  const int64_t end = g.base + n;
  const double r2 = g.r2;
  for (int dx = -1; dx <= 1; ++dx) {
    const int64_t cx = c0 + dx;
    if (cx < 0 || cx > g.cmax[0]) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int64_t cy = c1 + dy;
      if (cy < 0 || cy > g.cmax[1]) continue;
      const uint64_t klo = iss_key(g, cx, cy, zlo), khi = iss_key(g, cx, cy, zhi);
      int64_t lo = g.base, hi = end;  // the first entry of [base, end) whose key is >= klo
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skey[mid] < klo) lo = mid + 1; else hi = mid;
      }
      for (int64_t e = lo; e < end && skey[e] <= khi; ++e) {
        const double* yp = spts + 3 * e;
        const double e0 = x[0] - yp[0], e1 = x[1] - yp[1], e2 = x[2] - yp[2];
        const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
        if (d2 < r2) f(e, yp);
      }
    }
  }
}

// The cloud and the position inside it of this thread (block = kIssBlock consecutive positions of one cloud).
__device__ __forceinline__ bool iss_locate(const IssDesc* __restrict__ descs, const int32_t* __restrict__ blk_prob,
                                           int& p, int64_t& k) {
  p = blk_prob[blockIdx.x];
  k = (int64_t)((int)blockIdx.x - descs[p].blk_off) * kIssBlock + threadIdx.x;
  return k < descs[p].n;
}

// keys: the entries of point k of its cloud in its first `grids` grids (2: the grid of r_s and the grid of r_n; 1: the
// grid gs alone, as DBSCAN clustering keeps one grid per cloud -- icp_dbscan_device.h), and the identity permutation
__device__ __forceinline__ void iss_keys_grids_body(const IssDesc* __restrict__ descs,
                                                    const int32_t* __restrict__ blk_prob,
                                                    const double* __restrict__ pts, int64_t total, int grids,
                                                    uint64_t* __restrict__ key, int32_t* __restrict__ iota) {
  int p;
  int64_t k;
  if (!iss_locate(descs, blk_prob, p, k)) return;
  const IssDesc& d = descs[p];
  const int64_t i = d.off + k;
  key[i] = iss_point_key(d.gs, pts + 3 * i);
  iota[i] = (int32_t)i;
  if (grids < 2) return;
  key[total + i] = iss_point_key(d.gn, pts + 3 * i);
  iota[total + i] = (int32_t)(total + i);
}

__device__ __forceinline__ void iss_keys_body(const IssDesc* __restrict__ descs, const int32_t* __restrict__ blk_prob,
                                              const double* __restrict__ pts, int64_t total,
                                              uint64_t* __restrict__ key, int32_t* __restrict__ iota) {
  iss_keys_grids_body(descs, blk_prob, pts, total, 2, key, iota);
}

// the points in sorted order: entry e of `entries` (2 total for ISS, total for one grid per cloud)
__device__ __forceinline__ void iss_gather_entries_body(int64_t total, int64_t entries, const double* __restrict__ pts,
                                                        const int32_t* __restrict__ sidx, double* __restrict__ spts) {
  const int64_t e = (int64_t)blockIdx.x * kIssBlock + threadIdx.x;
  if (e >= entries) return;
  const int64_t s = sidx[e], i = s >= total ? s - total : s;
  spts[3 * e] = pts[3 * i];
  spts[3 * e + 1] = pts[3 * i + 1];
  spts[3 * e + 2] = pts[3 * i + 2];
}

__device__ __forceinline__ void iss_gather_body(int64_t total, const double* __restrict__ pts,
                                                const int32_t* __restrict__ sidx, double* __restrict__ spts) {
  iss_gather_entries_body(total, 2 * total, pts, sidx, spts);
}

// saliency: the query at sorted position k of the grid of r_s.  m, S1 and S2 live in registers; every array below is
// indexed by compile-time constants only.
__device__ __forceinline__ void iss_saliency_body(const IssDesc* __restrict__ descs,
                                                  const int32_t* __restrict__ blk_prob,
                                                  const uint64_t* __restrict__ skey, const int32_t* __restrict__ sidx,
                                                  const double* __restrict__ spts, double* __restrict__ sal,
                                                  int32_t* __restrict__ count) {
  int p;
  int64_t k;
  if (!iss_locate(descs, blk_prob, p, k)) return;
  const IssDesc& d = descs[p];
  if (!d.active) return;
  const int64_t e = d.gs.base + k, i = sidx[e];
  const double x[3] = {spts[3 * e], spts[3 * e + 1], spts[3 * e + 2]};
  int32_t m = 0;
  double s1[3] = {0.0, 0.0, 0.0}, s2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  iss_ball(d.gs, d.n, x, skey, spts, [&](int64_t, const double* yp) {
    icp_cov_add(s1, s2, yp, x);
    ++m;
  });
  double s = 0.0;
  if (m >= d.min_nb) {
    const double dm = (double)m;
    double a[6], V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};  // V is never read: its arithmetic is dropped
    a[0] = (s2[0] - (s1[0] * s1[0]) / dm) / dm;
    a[1] = (s2[1] - (s1[0] * s1[1]) / dm) / dm;
    a[2] = (s2[2] - (s1[0] * s1[2]) / dm) / dm;
    a[3] = (s2[3] - (s1[1] * s1[1]) / dm) / dm;
    a[4] = (s2[4] - (s1[1] * s1[2]) / dm) / dm;
    a[5] = (s2[5] - (s1[2] * s1[2]) / dm) / dm;
    for (int sweep = 0; sweep < 16; ++sweep) {
      bool rotated = icp_jacobi_rotate<0, 1, 2>(a, V);
      rotated |= icp_jacobi_rotate<0, 2, 1>(a, V);
      rotated |= icp_jacobi_rotate<1, 2, 0>(a, V);
      if (!rotated) break;
    }
    double e3 = a[0], e2 = a[3], e1 = a[5];  // ascending by three exchanges
    if (e2 < e3) { const double t = e3; e3 = e2; e2 = t; }
    if (e1 < e2) { const double t = e2; e2 = e1; e1 = t; }
    if (e2 < e3) { const double t = e3; e3 = e2; e2 = t; }
    if (e2 / e1 < d.g21 && e3 / e2 < d.g32) s = e3;
  }
  sal[i] = s;
  count[2 * i] = m;
}

// suppression: the query at sorted position k of the grid of r_n.  Returns whether the point is a keypoint.
__device__ __forceinline__ bool iss_suppress_body(const IssDesc* __restrict__ descs,
                                                  const int32_t* __restrict__ blk_prob, int64_t total,
                                                  const uint64_t* __restrict__ skey, const int32_t* __restrict__ sidx,
                                                  const double* __restrict__ spts, const double* __restrict__ sal,
                                                  int32_t* __restrict__ count, uint8_t* __restrict__ keep, int& p) {
  int64_t k;
  if (!iss_locate(descs, blk_prob, p, k)) return false;
  const IssDesc& d = descs[p];
  if (!d.active) return false;
  const int64_t e = d.gn.base + k, i = (int64_t)sidx[e] - total;
  const double x[3] = {spts[3 * e], spts[3 * e + 1], spts[3 * e + 2]};
  const double si = sal[i];
  int32_t cnt = 0;
  bool beaten = false;
  iss_ball(d.gn, d.n, x, skey, spts, [&](int64_t ej, const double*) {
    ++cnt;
    beaten = beaten || sal[(int64_t)sidx[ej] - total] > si;
  });
  const bool kp = si > 0.0 && cnt >= d.min_nb && !beaten;
  count[2 * i + 1] = cnt;
  keep[i] = kp ? 1 : 0;
  return kp;
}

// resolution, pass 0: thread t = one block of 256 consecutive points of a cloud of the self k-NN call (k = 2): the sum of
// sqrt(d2 of slot 1) in ascending index from 0.0
__device__ __forceinline__ void iss_res_block_body(const IcpDesc* __restrict__ descs,
                                                   const IcpKnnDesc* __restrict__ knns,
                                                   const int32_t* __restrict__ tblk_prob, int n_tblk,
                                                   const double* __restrict__ d2, double* __restrict__ partials) {
  const int t = (int)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tblk) return;
  const int p = tblk_prob[t];
  const IcpDesc& d = descs[p];
  const int64_t lo = (int64_t)(t - d.tblk_off) * 256;
  const int64_t hi = lo + 256 < d.n_t ? lo + 256 : d.n_t;
  double s = 0.0;
  for (int64_t i = lo; i < hi; ++i) s += sqrt(d2[knns[p].out_off + 2 * i + 1]);
  partials[t] = s;
}

// resolution, pass 1: thread p = one cloud: the block sums in ascending block order from 0.0, over n
__device__ __forceinline__ void iss_res_reduce_body(const IcpDesc* __restrict__ descs, int batch,
                                                    const double* __restrict__ partials, double* __restrict__ res) {
  const int p = (int)blockIdx.x * 256 + threadIdx.x;
  if (p >= batch) return;
  const IcpDesc& d = descs[p];
  if (d.n_t == 0) return;
  const int nb = (d.n_t + 255) / 256;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += partials[d.tblk_off + b];
  res[p] = s / (double)d.n_t;
}

// ---- launchers (kernels_keypoints.hip) --------------------------------------------------------------------------------
// Scratch of launch_iss_sort for `entries` keys; the stable sort of (key, entry) over the low `bits` bits.
size_t iss_sort_temp_bytes(int64_t entries);
hipError_t launch_iss_sort(hipStream_t s, void* d_temp, size_t temp_bytes, int64_t entries, int bits,
                           const uint64_t* d_key, const int32_t* d_iota, uint64_t* d_skey, int32_t* d_sidx);
void launch_iss_keys(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk, const double* d_pts,
                     int64_t total, uint64_t* d_key, int32_t* d_iota);
void launch_iss_gather(hipStream_t s, int64_t total, const double* d_pts, const int32_t* d_sidx, double* d_spts);
// The same two kernels for a call with `grids` (1 or 2) grids per cloud, grids * total entries
void launch_iss_keys_grids(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                           const double* d_pts, int64_t total, int grids, uint64_t* d_key, int32_t* d_iota);
void launch_iss_gather_entries(hipStream_t s, int64_t total, int64_t entries, const double* d_pts,
                               const int32_t* d_sidx, double* d_spts);
// sal[i] and count[2 i] = m of every point of the active clouds (the rest is left as the caller cleared it)
void launch_iss_saliency(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, double* d_sal,
                         int32_t* d_count);
// count[2 i + 1] = cnt, the mask, and the keypoint count per cloud (cleared by the caller)
void launch_iss_suppress(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk, int64_t total,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, const double* d_sal,
                         int32_t* d_count, uint8_t* d_keep, int32_t* d_kept);
// res[p] of every cloud of a self k-NN call with k = 2 (d2: its packed n x 2 output); partials: one double per block
// of 256 points
void launch_iss_resolution(hipStream_t s, const IcpDesc* d_desc, const IcpKnnDesc* d_knn, const int32_t* d_tblk_prob,
                           int n_tblk, int batch, const double* d_d2, double* d_partials, double* d_res);

}  // namespace thip
