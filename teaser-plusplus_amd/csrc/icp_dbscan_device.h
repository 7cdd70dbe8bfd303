// icp_dbscan_device.h -- the lane-independent device code of DBSCAN clustering (include/teaser_hip.h, "DBSCAN
// clustering"; kernels: kernels_cluster.hip, host side: icp_cluster.hip, design: DESIGN.md section 26): the bodies of
// the count, union, flatten and label kernels on the sorted cell index of icp_iss_device.h (IssGrid, iss_ball), and the
// lock-free union-find they share.  Nothing here uses a wave operation or LDS, so tests/dbscan_host_driver.cpp runs this
// very source one lane at a time.
//
// A call keeps ONE grid per cloud (IssDesc::gs, cell edge from eps; gn is unused; min_nb holds min_points), so sorted
// entry e and point index are both numbers in [0, total): sidx[e] is the packed index g = off + i of the point at e.
// parent[], is_root[] and scan[] are indexed by g; count[], root[] and label[] too, root[] holding the index i INSIDE
// the cloud (what the caller gets).
//
// Union-find.  parent[g] <= g holds at every instant: the count kernel writes parent[g] = g, a hook writes the smaller
// of two roots into the larger root's slot (one compare-and-swap that succeeds only while that slot still holds
// itself), path halving stores into parent[x] a value read further along x's own path, which is an ancestor of x and so
// not larger.  Every walk therefore descends strictly and ends after fewer than n steps, no cycle can form, and a
// failed compare-and-swap means another lane hooked that very root in the meantime: at most n - 1 hooks succeed per
// cloud, so the retries are bounded by them.  A retry continues from the value the compare-and-swap returned, which is
// smaller than the root it was tried on, so a + b falls with every retry whatever a load returns.  No lane ever waits
// for another.
#pragma once

#include "icp_iss_device.h"

namespace thip {

// ---- the three memory operations of the union-find.  A program that runs the lanes one after the other defines
// THIP_DBSCAN_HOST_ATOMICS and supplies plain ones (tests/hip_stub has no atomics).
#ifndef THIP_DBSCAN_HOST_ATOMICS
__device__ __forceinline__ int32_t dbscan_load(const int32_t* a) {
  return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void dbscan_store(int32_t* a, int32_t v) {
  __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Returns what *a held; *a = v iff that was `expect`.
__device__ __forceinline__ int32_t dbscan_cas(int32_t* a, int32_t expect, int32_t v) { return atomicCAS(a, expect, v); }
#endif

// The root of x's tree at some instant of the walk, halving the path on the way (plain stores of values read from
// further along the path).
__device__ __forceinline__ int32_t dbscan_find_halving(int32_t* __restrict__ parent, int32_t x) {
  for (;;) {
    const int32_t p = dbscan_load(parent + x);
    if (p == x) return x;
    const int32_t g = dbscan_load(parent + p);
    if (g == p) return p;
    dbscan_store(parent + x, g);
    x = g;
  }
}

// The root of x's tree, reading only (after the union kernel: the trees no longer change).
__device__ __forceinline__ int32_t dbscan_find(const int32_t* __restrict__ parent, int32_t x) {
  for (;;) {
    const int32_t p = parent[x];
    if (p == x) return x;
    x = p;
  }
}

// Joins the trees of a and b: the larger root goes under the smaller one.  Returns the root of the joined tree as this
// lane last saw it (an ancestor of both, from which the lane's next find starts).
__device__ __forceinline__ int32_t dbscan_unite(int32_t* __restrict__ parent, int32_t a, int32_t b) {
  for (;;) {
    a = dbscan_find_halving(parent, a);
    b = dbscan_find_halving(parent, b);
    if (a == b) return a;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const int32_t was = dbscan_cas(parent + hi, hi, lo);
    if (was == hi) return lo;
    a = was, b = lo;  // another lane hooked hi first, under was < hi: start over from there and from lo
  }
}

// count: the query at sorted position k of its cloud.  count[g] = the neighbours of g, itself included; parent[g] = g.
__device__ __forceinline__ void dbscan_count_body(const IssDesc* __restrict__ descs,
                                                  const int32_t* __restrict__ blk_prob,
                                                  const uint64_t* __restrict__ skey, const int32_t* __restrict__ sidx,
                                                  const double* __restrict__ spts, int32_t* __restrict__ count,
                                                  int32_t* __restrict__ parent) {
  int p;
  int64_t k;
  if (!iss_locate(descs, blk_prob, p, k)) return;
  const IssDesc& d = descs[p];
  if (!d.active) return;
  const int64_t e = d.gs.base + k;
  const int32_t g = sidx[e];
  const double x[3] = {spts[3 * e], spts[3 * e + 1], spts[3 * e + 2]};
  int32_t m = 0;
  iss_ball(d.gs, d.n, x, skey, spts, [&](int64_t, const double*) { ++m; });
  count[g] = m;
  parent[g] = g;
}

// union: a core point g unites itself with every core neighbour of smaller index (the pair's other lane skips it).
__device__ __forceinline__ void dbscan_union_body(const IssDesc* __restrict__ descs,
                                                  const int32_t* __restrict__ blk_prob,
                                                  const uint64_t* __restrict__ skey, const int32_t* __restrict__ sidx,
                                                  const double* __restrict__ spts, const int32_t* __restrict__ count,
                                                  int32_t* __restrict__ parent) {
  int p;
  int64_t k;
  if (!iss_locate(descs, blk_prob, p, k)) return;
  const IssDesc& d = descs[p];
  if (!d.active) return;
  const int64_t e = d.gs.base + k;
  const int32_t g = sidx[e], min_pts = d.min_nb;
  if (count[g] < min_pts) return;
  const double x[3] = {spts[3 * e], spts[3 * e + 1], spts[3 * e + 2]};
  int32_t top = g;  // an ancestor of g (or g): uniting it with j unites g's tree with j's, and its walk is shorter
  iss_ball(d.gs, d.n, x, skey, spts, [&](int64_t ej, const double*) {
    const int32_t j = sidx[ej];
    if (j < g && count[j] >= min_pts) top = dbscan_unite(parent, top, j);
  });
}

// flatten: point k of its cloud (original order).  root = the root's index inside the cloud for a core point, else -1.
__device__ __forceinline__ void dbscan_flatten_body(const IssDesc* __restrict__ descs,
                                                    const int32_t* __restrict__ blk_prob,
                                                    const int32_t* __restrict__ count,
                                                    const int32_t* __restrict__ parent, int32_t* __restrict__ root,
                                                    int32_t* __restrict__ is_root) {
  int p;
  int64_t k;
  if (!iss_locate(descs, blk_prob, p, k)) return;
  const IssDesc& d = descs[p];
  if (!d.active) return;
  const int32_t g = (int32_t)(d.off + k);
  const bool core = count[g] >= d.min_nb;
  const int32_t r = core ? dbscan_find(parent, g) : -1;
  root[g] = core ? (int32_t)(r - d.off) : -1;
  is_root[g] = r == g ? 1 : 0;
}

// label: the query at sorted position k of its cloud; scan = the exclusive scan of is_root over total + 1 entries.  The
// numbers are monotone in the root inside a cloud, so the smallest root among the core neighbours gives the smallest
// label.  The lane of position 0 writes the cloud's cluster count.
__device__ __forceinline__ void dbscan_label_body(const IssDesc* __restrict__ descs,
                                                  const int32_t* __restrict__ blk_prob,
                                                  const uint64_t* __restrict__ skey, const int32_t* __restrict__ sidx,
                                                  const double* __restrict__ spts, const int32_t* __restrict__ root,
                                                  const int32_t* __restrict__ scan, int32_t* __restrict__ label,
                                                  int32_t* __restrict__ n_clusters) {
  int p;
  int64_t k;
  if (!iss_locate(descs, blk_prob, p, k)) return;
  const IssDesc& d = descs[p];
  if (!d.active) return;
  const int32_t first = scan[d.off];
  if (k == 0) n_clusters[p] = scan[d.off + d.n] - first;
  const int64_t e = d.gs.base + k;
  const int32_t g = sidx[e];
  int32_t best = root[g];
  if (best < 0) {
    const double x[3] = {spts[3 * e], spts[3 * e + 1], spts[3 * e + 2]};
    int32_t lowest = INT32_MAX;
    iss_ball(d.gs, d.n, x, skey, spts, [&](int64_t ej, const double*) {
      const int32_t r = root[sidx[ej]];
      if (r >= 0 && r < lowest) lowest = r;
    });
    best = lowest == INT32_MAX ? -1 : lowest;
  }
  label[g] = best < 0 ? -1 : scan[d.off + best] - first;
}

// ---- launchers (kernels_cluster.hip) ----------------------------------------------------------------------------------
// Scratch of launch_dbscan_scan for `entries` flags; scan[e] = the sum of flag[0 .. e).
size_t dbscan_scan_temp_bytes(int64_t entries);
hipError_t launch_dbscan_scan(hipStream_t s, void* d_temp, size_t temp_bytes, int64_t entries, const int32_t* d_flag,
                              int32_t* d_scan);
void launch_dbscan_count(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, int32_t* d_count,
                         int32_t* d_parent);
void launch_dbscan_union(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, const int32_t* d_count,
                         int32_t* d_parent);
void launch_dbscan_flatten(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                           const int32_t* d_count, const int32_t* d_parent, int32_t* d_root, int32_t* d_is_root);
void launch_dbscan_label(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, const int32_t* d_root,
                         const int32_t* d_scan, int32_t* d_label, int32_t* d_n_clusters);

}  // namespace thip
