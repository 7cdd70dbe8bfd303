// icp_host.h -- what the host files of the ICP handle share (icp.hip: the iteration loop and covariance estimation;
// icp_outlier.hip: self k-NN, outlier removal and the options; icp_normals.hip: normal estimation and the
// self-estimating point-to-plane entry; icp_keypoints.hip: ISS keypoints; icp_cluster.hip: DBSCAN clustering; icp_fps.hip: farthest-point down-sampling; icp_color.hip: Colored ICP;
// icp_search.hip: neighbour search between two clouds; icp_fpfh.hip: the Open3D-form FPFH and the neighbour lists in
// pieces; icp_boundary.hip: boundary points; icp_rgbd.hip: depth frames; icp_odometry.hip: RGB-D odometry): the handle and its buffers, and the scaffold
// of a cloud call -- the entry checks (begin_cloud_call), the per-call index under construction (IcpIndex,
// add_problem), the sizes of the index buffers by name (index_bytes, ensure_buffers), the packing and the uploads
// (upload_points, upload_inputs), the index build (launch_index), the one copy back (copy_back, read_fallbacks) and
// the self k-NN stage that outlier removal and the keypoints' resolution run (run_self_knn).  An entry point writes
// itself what is its own: its argument checks, its records, the layout of B_X, its launches and the scatter of the
// results.
#pragma once

#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_common.h"
#include "icp_internal.h"
#include "teaser_hip.h"

namespace thip {

// B_N*: the descriptors, records and block maps of the normal estimation that precedes the iterations of
// teaser_hip_icp_batch_auto (its other buffers are the ICP's own).  B_K*: the sorted cell index of ISS keypoint
// detection (icp_keypoints.hip): descriptors, block map, keys and entries before and after the sort, the sorted points
// and the sort's scratch; DBSCAN clustering (icp_cluster.hip) builds the same index with one grid per cloud, shares
// B_KTEMP between the sort and the scan, and adds B_DPARENT (the union-find), B_DFLAG ("is a root", total + 1 entries)
// and B_DSCAN (its exclusive scan).  B_COLOR_*: Colored ICP (icp_color.hip): the per-problem IcpColorDesc records, one intensity per
// source point, and per target point the {gradient, intensity} record; its gradient pass keeps its descriptors, records
// and block maps in B_N* (a coloured call estimates no normals).  B_SEARCH_TMP: the radius search's rows before they are
// ordered (icp_search.hip).  B_FPFH_*: the Open3D-form FPFH (icp_fpfh.hip): the pieces' descriptors, search records and
// block map and the list scratch (d2, then indices); boundary points (icp_boundary.hip) run on the same four and add
// B_BND_DESC, the pieces' IcpBoundaryDesc records.  B_RGBD_*: the depth-frame calls (icp_rgbd.hip): the records of the
// frames or projections, the packed images (unprojection) or colours (projection), and the tiles' counts and starts
// (unprojection) or the key image (projection).  B_ODO_*: RGB-D odometry (icp_odometry.hip): the image pyramids of all
// pairs and the level-0 scratch planes; its records, inputs, keys and partials live in B_RGBD_*, B_STATE, B_BLK, B_PARTIALS
enum { B_DESC, B_STATE, B_BLK, B_TBLK, B_X, B_Q, B_TBUCKET, B_BCOUNT, B_BSTART, B_CURSOR, B_QS, B_QJ, B_MATCH,
       B_PARTIALS, B_LIVE, B_NORMALS, B_COV_S, B_COV_T, B_NDESC, B_NKNN, B_NREC, B_NBLK, B_NTBLK, B_KDESC, B_KBLK,
       B_KKEY, B_KIOTA, B_KSKEY, B_KSIDX, B_KSPTS, B_KTEMP, B_DPARENT, B_DFLAG, B_DSCAN, B_COLOR_DESC, B_COLOR_S, B_COLOR_T, B_SEARCH_TMP,
       B_FPFH_DESC, B_FPFH_SD, B_FPFH_BLK, B_FPFH_LIST, B_BND_DESC, B_RGBD_DESC, B_RGBD_IN, B_RGBD_WORK, B_ODO_IMG, B_ODO_TMP, B_COUNT };

}  // namespace thip

struct teaser_hip_icp : thip::HandleBase {
  int32_t* h_live = nullptr;  // page-locked: the one copy per iteration group
  thip::DevBuf buf[thip::B_COUNT];
  std::vector<double> stage;  // host packing of the points
  std::vector<double> back;   // self k-NN / outlier removal: the one copy back of a call
  std::vector<double> cstage; // Colored ICP: host packing of the intensities and the {gradient, intensity} records
  int32_t knn_ring_cap = thip::kIcpKnnRingCap;  // option "knn_ring_cap"
  int64_t knn_fallbacks = 0;              // option "knn_fallbacks": queries of the last call served by the whole-cloud route
  int32_t fps_resident_max = thip::kFpsResidentCap;  // option "fps_resident_max" (icp_fps.hip)
  int64_t fpfh_list_bytes = thip::kFpfhListBytes;    // option "fpfh_list_bytes" (icp_fpfh.hip)
  ~teaser_hip_icp() {
    if (h_live) (void)hipHostFree(h_live);
  }
};

namespace thip {

inline int64_t next_pow2(int64_t v) {
  int64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

// The hash grid of one cloud q (d.n_t > 0 points) for search radius r: origin, cell edge, extent, bucket count, and
// the centre the sums are taken about.
inline void set_grid(IcpDesc& d, const double* q, double r) {
  double lo[3], hi[3];
  for (int c = 0; c < 3; ++c) lo[c] = hi[c] = q[c];
  for (int64_t j = 1; j < d.n_t; ++j)
    for (int c = 0; c < 3; ++c) {
      lo[c] = std::min(lo[c], q[3 * j + c]);
      hi[c] = std::max(hi[c], q[3 * j + c]);
    }
  double mag = 0;
  for (int c = 0; c < 3; ++c) mag = std::max(mag, std::max(fabs(lo[c]), fabs(hi[c])));
  // cell edge slightly above r: two points closer than r then differ by at most one cell per axis although
  // their cell coordinates are rounded (relative margin 1e-6; absolute 1e-12 of the coordinates' magnitude)
  const double cell = r * (1 + 1e-6) + 1e-12 * mag;
  d.inv_h = 1.0 / cell;
  for (int c = 0; c < 3; ++c) {
    d.origin[c] = lo[c];
    d.centre[c] = 0.5 * (lo[c] + hi[c]);
    d.cmax[c] = icp_cell(hi[c], lo[c], d.inv_h);
  }
  d.tb_mask = next_pow2(2 * (int64_t)d.n_t) - 1;
}

// What the calls on the sorted cell index share (icp_keypoints.hip, icp_cluster.hip; the grid type is IssGrid of
// icp_iss_device.h).  The bits a value needs:
inline int key_bits_for(uint64_t v) {
  int b = 0;
  while (b < 64 && (v >> b) != 0) ++b;
  return b;
}

// A radius as given: not negative, finite like its square.
inline bool radius_ok(double r) { return std::isfinite(r) && r >= 0 && std::isfinite(r * r); }

// The grid of radius r over the cloud q (n > 0 points), and the bits its three cell coordinates need.
template <class Grid>
void make_sorted_grid(Grid& g, const double* q, int32_t n, double r, int (&bits)[3]) {
  IcpDesc d;
  memset(&d, 0, sizeof(d));
  d.n_t = n;
  set_grid(d, q, r);
  g.inv_h = d.inv_h;
  g.r2 = r * r;
  for (int c = 0; c < 3; ++c) {
    g.origin[c] = d.origin[c];
    g.cmax[c] = d.cmax[c];
    bits[c] = key_bits_for((uint64_t)d.cmax[c]);
  }
}

// The target index of one call under construction: per problem the descriptor with its offsets and hash grid, the
// block -> problem maps of both kernels' grids, and the running totals of source points, target points and buckets.
struct IcpIndex {
  std::vector<IcpDesc> desc;
  std::vector<int32_t> blk_prob, tblk_prob;
  int64_t s_off = 0, t_off = 0, b_off = 0;
};

// Appends problem b (n_s source points; the n_t points q[b] indexed for search radius r) with nblk blocks of the
// kernel that consumes the index; the caller fills in the descriptor's other fields.
inline IcpDesc& add_problem(IcpIndex& ix, int b, int32_t n_s, int32_t n_t, const double* const* q, double r, int32_t nblk) {
  ix.desc.emplace_back();
  IcpDesc& d = ix.desc.back();
  memset(&d, 0, sizeof(d));
  d.n_s = n_s;
  d.n_t = n_t;
  d.s_off = ix.s_off;
  d.t_off = ix.t_off;
  d.b_off = ix.b_off;
  d.blk_off = (int32_t)ix.blk_prob.size();
  d.nblk = nblk;
  d.tblk_off = (int32_t)ix.tblk_prob.size();
  d.r2 = r * r;
  if (n_t > 0) {
    set_grid(d, q[b], r);
    ix.b_off += d.tb_mask + 2;  // tb + 1 starts
  }
  for (int k = 0; k < nblk; ++k) ix.blk_prob.push_back(b);
  for (int k = 0; k < (n_t + 255) / 256; ++k) ix.tblk_prob.push_back(b);
  ix.s_off += n_s;
  ix.t_off += n_t;
  return d;
}

// The sizes of the buffers that hold a call's index: descriptors, both block maps, the points (B_Q), and per point and
// per bucket what launch_index fills; with `worklist` also B_MATCH as the self k-NN worklist (2 int32 per point).
// Counts below `least` (0 or 1) are sized as `least`.  The caller sets what is its own: B_STATE, B_X, B_PARTIALS, ...
inline void index_bytes(const IcpIndex& ix, int64_t least, bool worklist, size_t (&bytes)[B_COUNT]) {
  const size_t t = (size_t)std::max(ix.t_off, least), b = (size_t)std::max(ix.b_off, least);
  bytes[B_DESC] = sizeof(IcpDesc) * ix.desc.size();
  bytes[B_BLK] = sizeof(int32_t) * std::max<size_t>(ix.blk_prob.size(), (size_t)least);
  bytes[B_TBLK] = sizeof(int32_t) * std::max<size_t>(ix.tblk_prob.size(), (size_t)least);
  bytes[B_Q] = bytes[B_QS] = sizeof(double) * 3 * t;
  bytes[B_TBUCKET] = bytes[B_QJ] = sizeof(int32_t) * t;
  bytes[B_BCOUNT] = bytes[B_BSTART] = bytes[B_CURSOR] = sizeof(int32_t) * b;
  if (worklist) bytes[B_MATCH] = sizeof(int32_t) * 2 * (size_t)ix.t_off;
}

// Grows every buffer of the handle to its entry of `bytes`; `what`: the message of a failed allocation.
inline int32_t ensure_buffers(teaser_hip_icp* h, const size_t (&bytes)[B_COUNT], const char* what) {
  for (int k = 0; k < B_COUNT; ++k)
    if (!h->buf[k].ensure(bytes[k])) return fail(h, TEASER_HIP_ERR_OOM, what);
  return TEASER_HIP_OK;
}

// Packs the clouds q[b] (n[b] points each) one after the other -- the order of their descriptors' offsets -- into
// h->stage from its double `first` on, and enqueues their upload to B_Q; `what`: the message of a failed copy.
inline int32_t upload_points(teaser_hip_icp* h, int32_t batch, const double* const* q, const int32_t* n, size_t first,
                             const char* what) {
  size_t at = first;
  for (int b = 0; b < batch; ++b) {
    if (n[b]) memcpy(&h->stage[at], q[b], 24 * (size_t)n[b]);
    at += 3 * (size_t)n[b];
  }
  if (at > first)
    FCHK(h, hipMemcpyAsync(h->buf[B_Q].p, &h->stage[first], sizeof(double) * (at - first), hipMemcpyHostToDevice,
                           h->stream),
         what);
  return TEASER_HIP_OK;
}

// Packs the points into h->stage (sources, then targets; src may be NULL when no problem has any) and enqueues
// the uploads: descriptors, the per-problem `records` for B_STATE, both block maps, sources, targets (n_dst points
// per problem).
inline int32_t upload_inputs(teaser_hip_icp* h, const IcpIndex& ix, const double* const* src, const double* const* dst,
                             const int32_t* n_dst, const void* records, size_t record_bytes) {
  for (size_t b = 0; b < ix.desc.size(); ++b) {
    const IcpDesc& d = ix.desc[b];
    if (d.n_s) memcpy(&h->stage[(size_t)(3 * d.s_off)], src[b], 24 * (size_t)d.n_s);
  }
  DevBuf* B = h->buf;
  const struct {
    void* d;
    const void* hsrc;
    size_t n;
  } copies[] = {{B[B_DESC].p, ix.desc.data(), sizeof(IcpDesc) * ix.desc.size()},
                {B[B_STATE].p, records, record_bytes},
                {B[B_BLK].p, ix.blk_prob.data(), sizeof(int32_t) * ix.blk_prob.size()},
                {B[B_TBLK].p, ix.tblk_prob.data(), sizeof(int32_t) * ix.tblk_prob.size()},
                {B[B_X].p, h->stage.data(), sizeof(double) * 3 * ix.s_off}};
  for (const auto& c : copies)
    if (c.n) FCHK(h, hipMemcpyAsync(c.d, c.hsrc, c.n, hipMemcpyHostToDevice, h->stream), "hipMemcpyAsync (inputs)");
  return upload_points(h, (int32_t)ix.desc.size(), dst, n_dst, (size_t)(3 * ix.s_off),
                       "hipMemcpyAsync (inputs)");
}

// Clears the bucket counts and enqueues the kernels that build the index over the uploaded targets.
inline int32_t launch_index(teaser_hip_icp* h, const IcpIndex& ix) {
  DevBuf* B = h->buf;
  if (ix.b_off) FCHK(h, hipMemsetAsync(B[B_BCOUNT].p, 0, sizeof(int32_t) * ix.b_off, h->stream), "hipMemsetAsync");
  launch_icp_index(h->stream, B[B_DESC].as<IcpDesc>(), B[B_TBLK].as<int32_t>(), (int)ix.tblk_prob.size(),
                   (int)ix.desc.size(), B[B_Q].as<double>(), B[B_TBUCKET].as<int32_t>(), B[B_BCOUNT].as<int32_t>(),
                   B[B_BSTART].as<int32_t>(), B[B_CURSOR].as<int32_t>(), B[B_QS].as<double>(), B[B_QJ].as<int32_t>());
  return TEASER_HIP_OK;
}

// What the three calls check alike: n, the clouds and their coordinates.  *total = the number of points.
inline int32_t check_clouds(teaser_hip_icp* h, int32_t batch, const double* const* points, const int32_t* n, int64_t* total) {
  *total = 0;
  if (!n) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must not be NULL");
  for (int b = 0; b < batch; ++b) {
    if (n[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must be >= 0" + at(b));
    if (n[b] > 0 && (!points || !points[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "points is NULL" + at(b));
    if (n[b] > 0 && !finite_points(points[b], n[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "points has a non-finite coordinate" + at(b));
    *total += n[b];
  }
  if (*total >= INT32_MAX / 9) return fail(h, TEASER_HIP_ERR_BAD_ARG, "too many points in one call");
  return TEASER_HIP_OK;
}

// How a cloud call begins: the handle, its cleared error (and, for the calls that report it, fallback count), batch
// and check_clouds.  done: the entry point returns rc at once; else total = the number of points.
struct CallStart {
  int32_t rc;
  bool done;
  int64_t total;
};
inline CallStart begin_cloud_call(teaser_hip_icp* h, int32_t batch, const double* const* points, const int32_t* n,
                                  bool reset_fallbacks) {
  if (!h) return {TEASER_HIP_ERR_BAD_ARG, true, 0};
  h->err.clear();
  if (reset_fallbacks) h->knn_fallbacks = 0;
  if (batch < 0) return {fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0"), true, 0};
  if (batch == 0) return {TEASER_HIP_OK, true, 0};
  CallStart c = {TEASER_HIP_OK, false, 0};
  c.rc = check_clouds(h, batch, points, n, &c.total);
  c.done = c.rc != TEASER_HIP_OK;
  return c;
}

// The one copy back of a call (`bytes` of B_X from byte `off` -> h->back) and its synchronisation.  launch NULL: the
// caller has checked its launches already.
inline int32_t copy_back(teaser_hip_icp* h, size_t off, size_t bytes, const char* sync,
                         const char* launch = "kernel launch (k-NN / outlier removal)",
                         const char* copy = "hipMemcpyAsync (results)") {
  h->back.resize((bytes + 7) / 8);
  if (launch) FCHK(h, hipGetLastError(), launch);
  FCHK(h, hipMemcpyAsync(h->back.data(), h->buf[B_X].as<char>() + off, bytes, hipMemcpyDeviceToHost, h->stream), copy);
  FCHK(h, hipStreamSynchronize(h->stream), sync);
  return TEASER_HIP_OK;
}

// knn_fallbacks of the call: the worklist counter, at byte `off` of what copy_back brought.
inline void read_fallbacks(teaser_hip_icp* h, size_t off) {
  int32_t fallbacks = 0;
  memcpy(&fallbacks, (const char*)h->back.data() + off, sizeof(int32_t));
  h->knn_fallbacks = fallbacks;
}

// The cell edge h of the self k-NN grid of one cloud (n > 0 points, `want` = min(k, n) neighbours per query): the
// bounding box is cut into about n / c cells, c = max(2, want / 2) points per cell, counting only the axes along
// which the box is wider than a cell (a planar cloud gets a 2-D grid of square cells, a collinear one a 1-D grid),
// and never into more than 2^20 cells per axis.  A cloud of identical points gets h = 1 (one cell).  *rings_ok is
// cleared for an extent whose squares leave the normal range: such a cloud is served by the whole-cloud route.
inline double knn_edge(const double* q, int32_t n, int32_t want, bool* rings_ok) {
  double lo[3], hi[3], e[3];
  for (int c = 0; c < 3; ++c) lo[c] = hi[c] = q[c];
  for (int64_t j = 1; j < n; ++j)
    for (int c = 0; c < 3; ++c) {
      lo[c] = std::min(lo[c], q[3 * j + c]);
      hi[c] = std::max(hi[c], q[3 * j + c]);
    }
  for (int c = 0; c < 3; ++c) e[c] = hi[c] - lo[c];
  std::sort(e, e + 3);  // e[2] the largest
  const double E = e[2];
  *rings_ok = true;
  if (E == 0) return 1.0;
  if (!(E > 1e-140 && E < 1e140)) {
    *rings_ok = false;
    return 1.0;
  }
  const double cells = std::max(1.0, floor((double)n / (double)std::max(2, want / 2)));
  // the thin axes are found by comparing the extents themselves with the edge of the lower-dimensional grid, from
  // one dimension up, so that no product of two tiny ratios decides anything
  double hh = E / cells;                                   // a 1-D grid along the longest axis
  if (e[1] > hh) {
    hh = E * sqrt((e[1] / E) / cells);                     // a 2-D grid of square cells
    if (e[0] > hh) hh = E * cbrt((e[1] / E) * (e[0] / E) / cells);
  }
  return std::max(hh, E / 1048576.0);
}

// Where one self k-NN stage puts its outputs in B_X (byte offsets).  res_per_cloud is set by the caller: doubles per
// cloud, cleared with the worklist counter and lying right in front of it, so that one memset and one copy serve both
// (self k-NN only; the keypoints' resolutions).
struct KnnLayout {
  int res_per_cloud = 0;
  size_t d2 = 0, idx = 0, avg = 0, stats = 0, res = 0, ints = 0, counter = 0, keep = 0, bytes = 0;
  int64_t slots = 0;  // sum of n k (self k-NN)
};

// Index and self k-NN launches of one call (icp_outlier.hip).  k[b] neighbours per cloud; ratio NULL: self k-NN (idx /
// d2 outputs at L.idx / L.d2 of B_X), else statistical removal (avg at L.avg, the kept counts at L.ints); the worklist
// counter at L.counter.  B_PARTIALS holds a double per target block unless the call is
// plain self k-NN.  Leaves the descriptors in ix.
int32_t run_self_knn(teaser_hip_icp* h, int32_t batch, const double* const* points, const int32_t* n, const int32_t* k,
                     const double* ratio, IcpIndex& ix, KnnLayout& L);

// The descriptors of one normal-estimation pass over `batch` clouds; a cloud with n[b] = 0 has no blocks.
struct NormalsPlan {
  IcpIndex ix;
  std::vector<IcpKnnDesc> knn;
  std::vector<IcpNormalDesc> nd;
  std::vector<int32_t> blk;  // hybrid blocks, then k-NN blocks
  int n_hyb = 0, n_knn = 0;  // blocks of either kind
  int top_hyb = 0, top_knn = 0;
};

// What a call that estimates normals on the way (icp_fpfh.hip) needs of icp_normals.hip.  check_normal_search: one
// search record of the normals contract; `arg` names the argument in the message.  plan_normals_in_place: the plan of
// the clouds b with estimated[b] != 0 (record rec[b]) where ALL clouds of the call lie packed one after the other in the
// point array, the normals going to the same rows of d_nrm.  launch_normals_plan: uploads the plan (B_N*), builds the
// index over d_q and enqueues the search launches; the caller has sized the index buffers for P.ix (index_bytes with
// the worklist) and gives the worklist counter, one int32 on the device.
int32_t check_normal_search(teaser_hip_icp* h, const teaser_icp_normal_search_c& r, int b, const char* arg);
void plan_normals_in_place(teaser_hip_icp* h, NormalsPlan& P, int32_t batch, const double* const* points,
                           const int32_t* n, const teaser_icp_normal_search_c* rec, const char* estimated);
int32_t launch_normals_plan(teaser_hip_icp* h, const NormalsPlan& P, const double* d_q, double* d_nrm,
                            int32_t* d_counter);

// The neighbour lists of a call that walks every point's sorted list (icp_fpfh.hip, icp_boundary.hip), in pieces under
// the option "fpfh_list_bytes".  One pass: its pieces' blocks in B_FPFH_BLK from blk0 (n_hyb hybrid blocks, then n_knn
// k-NN blocks).
struct ListPass {
  int64_t blk0 = 0, slots = 0;
  int n_hyb = 0, n_knn = 0;
  std::vector<int32_t> hyb, knn;  // the pieces of either kind
};
// The plan of a call: the clouds with the grids of the search (ix), their pieces (an IcpDesc of n_s points from s_off,
// the cloud itself at t_off, and an IcpSearchDesc of max_nn slots per row from out_off of the list scratch), the passes
// and the block map of all passes.
struct ListPlan {
  IcpIndex ix;
  std::vector<IcpDesc> piece;
  std::vector<IcpSearchDesc> psd;
  std::vector<int32_t> cloud;  // the cloud of every piece
  std::vector<ListPass> passes;
  std::vector<int32_t> blk;
  int64_t max_slots = 1;  // the list scratch holds this many (d2, index) slots
  int top_hyb = 0, top_knn = 0;
};
// icp_fpfh.hip.  check_list_search: one search record of such a call (hybrid or k-NN, max_nn in [2, 100], not oriented;
// the argument is named "search").  plan_lists: the plan of the checked clouds.  list_bytes: the sizes of B_FPFH_*.
// upload_lists: enqueues the uploads of the plan (B_DESC, B_TBLK, B_FPFH_DESC / _SD / _BLK).  launch_lists: enqueues the
// search launches that fill the lists of one pass (d2 at B_FPFH_LIST, the indices max_slots doubles behind); counter:
// the worklist counter of the k-NN search, one int32 on the device.
int32_t check_list_search(teaser_hip_icp* h, const teaser_icp_normal_search_c& r, int b);
void plan_lists(teaser_hip_icp* h, ListPlan& L, int32_t batch, const double* const* points, const int32_t* n,
                const teaser_icp_normal_search_c* search);
void list_bytes(const ListPlan& L, size_t (&bytes)[B_COUNT]);
int32_t upload_lists(teaser_hip_icp* h, const ListPlan& L);
int32_t launch_lists(teaser_hip_icp* h, const ListPlan& L, const ListPass& P, int32_t* counter);

// Called by icp_run_batch between the uploads and the index build of the iterations: ix is the call's index, the
// targets lie in B_Q at its offsets.  Returns a status.
typedef int32_t (*IcpPreIndexHook)(teaser_hip_icp* h, void* ctx, const IcpIndex& ix);

// One iteration (a correspondence pass and its finalize) of a call that holds a Colored-ICP problem, enqueued on the
// handle's buffers; ctx is the hook's.  icp.hip reaches the mode-3 launcher through it and names no launcher of its own.
typedef void (*IcpIterateFn)(teaser_hip_icp* h, void* ctx, int n_blk, int batch);

// Every batched ICP entry point (icp.hip).  max_method: the largest estimation method the entry accepts.  nsearch: NULL,
// or per problem a record whose max_nn != 0 stands in for the dst_normals of a point-to-plane problem that gives none;
// `hook` then has to fill those rows of B_NORMALS.  iterate: what enqueues an iteration when the call holds a
// Colored-ICP problem (max_method = 3 needs it); the hook then has to fill B_COLOR_*.
int32_t icp_run_batch(teaser_hip_icp* h, int32_t batch, const double* const* src, const int32_t* n_src,
                      const double* const* dst, const int32_t* n_dst, const double* init,
                      const teaser_icp_params_c* params, teaser_icp_result_c* out, int32_t* const* corr,
                      const double* const* dst_normals, const teaser_icp_estimation_c* est,
                      const double* const* src_cov, const double* const* dst_cov, int max_method,
                      const teaser_icp_normal_search_c* nsearch, IcpPreIndexHook hook, void* ctx,
                      IcpIterateFn iterate = nullptr);

}  // namespace thip
