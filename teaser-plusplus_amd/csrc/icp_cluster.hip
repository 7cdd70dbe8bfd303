// icp_cluster.hip -- host side of DBSCAN clustering on the ICP handle (include/teaser_hip.h, "DBSCAN clustering").
// Kernels: kernels_cluster.hip on the device code of icp_dbscan_device.h; design and launch count in DESIGN.md
// section 26.
//
// One call is one stage over every cloud: per cloud the grid of eps (make_sorted_grid), the key layout, keys, one
// stable sort of n entries, the gather (the kernels of ISS keypoint detection with one grid per cloud), then count,
// union, flatten, one exclusive scan and label, and one copy back.  Neither the launches nor the synchronisations
// depend on the data.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_common.h"
#include "icp_dbscan_device.h"
#include "icp_host.h"
#include "icp_internal.h"
#include "teaser_hip.h"

using namespace thip;

static_assert(sizeof(teaser_icp_dbscan_params_c) == 16, "the header states the record's size");

extern "C" {

int32_t teaser_hip_icp_cluster_dbscan_batch(teaser_hip_icp* h, int32_t batch, const double* const* points,
                                            const int32_t* n, const teaser_icp_dbscan_params_c* params,
                                            int32_t* const* labels_out, int32_t* n_clusters_out,
                                            int32_t* const* count_out, int32_t* const* root_out) {
  const CallStart c = begin_cloud_call(h, batch, points, n, false);
  if (c.done) return c.rc;
  const int64_t total = c.total;
  int32_t rc = TEASER_HIP_OK;
  if (!params) return fail(h, TEASER_HIP_ERR_BAD_ARG, "params must not be NULL");
  if (!n_clusters_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_clusters_out must not be NULL");
  if (total >= INT32_MAX) return fail(h, TEASER_HIP_ERR_BAD_ARG, "too many points in one call");
  for (int b = 0; b < batch; ++b) {
    const teaser_icp_dbscan_params_c& p = params[b];
    if (!radius_ok(p.eps)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "eps must be >= 0 and finite like its square" + at(b));
    if (p.min_points < 1) return fail(h, TEASER_HIP_ERR_BAD_ARG, "min_points must be >= 1" + at(b));
    if (p.reserved != 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "reserved must be 0" + at(b));
    if (n[b] > 0 && (!labels_out || !labels_out[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "labels_out is NULL" + at(b));
  }

  // ---- descriptors, grids and the key layout ----
  std::vector<IssDesc> desc((size_t)batch);
  std::vector<int32_t> blk;
  std::vector<int> cbits(3 * (size_t)batch, 0);
  int key_bits = 0;
  bool any_active = false;
  int64_t off = 0;
  for (int b = 0; b < batch; ++b) {
    IssDesc& d = desc[(size_t)b];
    memset(&d, 0, sizeof(d));
    d.n = n[b];
    d.min_nb = params[b].min_points;
    d.off = off;
    d.blk_off = (int32_t)blk.size();
    const double eps = params[b].eps;
    d.active = n[b] > 0 && eps * eps > 0;
    if (d.active) {
      int bs[3];
      make_sorted_grid(d.gs, points[b], n[b], eps, bs);
      for (int k = 0; k < 3; ++k) cbits[3 * (size_t)b + k] = bs[k];
      key_bits = std::max(key_bits, bs[0] + bs[1] + bs[2]);
      any_active = true;
    }
    for (int k = 0; k < (n[b] + kIssBlock - 1) / kIssBlock; ++k) blk.push_back(b);
    off += n[b];
  }
  const int id_bits = key_bits_for((uint64_t)((int64_t)batch - 1));
  const int bits = key_bits + id_bits;
  if (bits > 63)
    for (int b = 0; b < batch; ++b)  // the cloud whose grid is the widest
      if (cbits[3 * (size_t)b] + cbits[3 * (size_t)b + 1] + cbits[3 * (size_t)b + 2] == key_bits)
        return fail(h, TEASER_HIP_ERR_BAD_ARG,
                    "eps is too small for the cloud's extent: the cell keys of the call need " + std::to_string(bits) +
                        " bits (at most 63)" + at(b));
  for (int b = 0; b < batch; ++b) {
    IssDesc& d = desc[(size_t)b];
    d.gs.base = d.off;
    d.gs.id = (uint64_t)b << key_bits;
    d.gs.shift[1] = cbits[3 * (size_t)b + 2];
    d.gs.shift[0] = cbits[3 * (size_t)b + 2] + cbits[3 * (size_t)b + 1];
  }

  // ---- outputs a call without device work gives ----
  for (int b = 0; b < batch; ++b) {
    n_clusters_out[b] = 0;
    if (n[b] == 0) continue;
    std::fill(labels_out[b], labels_out[b] + n[b], -1);
    if (count_out && count_out[b]) std::fill(count_out[b], count_out[b] + n[b], 0);
    if (root_out && root_out[b]) std::fill(root_out[b], root_out[b] + n[b], -1);
  }
  if (!any_active) return TEASER_HIP_OK;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");

  // ---- the one stage ----
  const int n_blk = (int)blk.size();
  const size_t T = (size_t)total;
  // B_X: labels, roots (both cleared to -1), counts, cluster counts (both cleared to 0)
  const size_t o_root = sizeof(int32_t) * T, o_cnt = 2 * o_root, o_ncl = 3 * o_root,
               out_bytes = o_ncl + sizeof(int32_t) * (size_t)batch;
  size_t bytes[B_COUNT] = {};
  bytes[B_X] = out_bytes;
  bytes[B_Q] = 24 * T;
  bytes[B_KDESC] = sizeof(IssDesc) * batch;
  bytes[B_KBLK] = sizeof(int32_t) * n_blk;
  bytes[B_KKEY] = bytes[B_KSKEY] = 8 * T;
  bytes[B_KIOTA] = bytes[B_KSIDX] = 4 * T;
  bytes[B_KSPTS] = 24 * T;
  bytes[B_KTEMP] = std::max(iss_sort_temp_bytes(total), dbscan_scan_temp_bytes(total + 1));
  bytes[B_DPARENT] = 4 * T;
  bytes[B_DFLAG] = bytes[B_DSCAN] = 4 * (T + 1);
  if ((rc = ensure_buffers(h, bytes, "hipMalloc failed (clustering buffers)")) != TEASER_HIP_OK) return rc;
  hipStream_t s = h->stream;
  DevBuf* B = h->buf;
  char* out = B[B_X].as<char>();
  h->stage.resize(3 * T);
  if ((rc = upload_points(h, batch, points, n, 0, "hipMemcpyAsync (points)")) != TEASER_HIP_OK) return rc;
  FCHK(h, hipMemcpyAsync(B[B_KDESC].p, desc.data(), bytes[B_KDESC], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (descriptors)");
  FCHK(h, hipMemcpyAsync(B[B_KBLK].p, blk.data(), bytes[B_KBLK], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (block map)");
  // the clouds without neighbours keep these: label -1, root -1, count 0, no cluster, no root flag
  FCHK(h, hipMemsetAsync(out, 0xFF, o_cnt, s), "hipMemsetAsync");
  FCHK(h, hipMemsetAsync(out + o_cnt, 0, out_bytes - o_cnt, s), "hipMemsetAsync");
  FCHK(h, hipMemsetAsync(B[B_DFLAG].p, 0, bytes[B_DFLAG], s), "hipMemsetAsync");
  const IssDesc* dd = B[B_KDESC].as<IssDesc>();
  const int32_t* dblk = B[B_KBLK].as<int32_t>();
  const uint64_t* skey = B[B_KSKEY].as<uint64_t>();
  const int32_t* sidx = B[B_KSIDX].as<int32_t>();
  const double* spts = B[B_KSPTS].as<double>();
  int32_t *d_label = (int32_t*)out, *d_root = (int32_t*)(out + o_root), *d_count = (int32_t*)(out + o_cnt),
          *d_ncl = (int32_t*)(out + o_ncl);
  launch_iss_keys_grids(s, dd, dblk, n_blk, B[B_Q].as<double>(), total, 1, B[B_KKEY].as<uint64_t>(),
                        B[B_KIOTA].as<int32_t>());
  FCHK(h, launch_iss_sort(s, B[B_KTEMP].p, bytes[B_KTEMP], total, std::max(bits, 1), B[B_KKEY].as<uint64_t>(),
                          B[B_KIOTA].as<int32_t>(), B[B_KSKEY].as<uint64_t>(), B[B_KSIDX].as<int32_t>()),
       "clustering sort");
  launch_iss_gather_entries(s, total, total, B[B_Q].as<double>(), sidx, B[B_KSPTS].as<double>());
  launch_dbscan_count(s, dd, dblk, n_blk, skey, sidx, spts, d_count, B[B_DPARENT].as<int32_t>());
  launch_dbscan_union(s, dd, dblk, n_blk, skey, sidx, spts, d_count, B[B_DPARENT].as<int32_t>());
  launch_dbscan_flatten(s, dd, dblk, n_blk, d_count, B[B_DPARENT].as<int32_t>(), d_root, B[B_DFLAG].as<int32_t>());
  FCHK(h, launch_dbscan_scan(s, B[B_KTEMP].p, bytes[B_KTEMP], total + 1, B[B_DFLAG].as<int32_t>(),
                             B[B_DSCAN].as<int32_t>()),
       "clustering scan");
  launch_dbscan_label(s, dd, dblk, n_blk, skey, sidx, spts, d_root, B[B_DSCAN].as<int32_t>(), d_label, d_ncl);
  if ((rc = copy_back(h, 0, out_bytes, "clustering", "kernel launch (clustering)")) != TEASER_HIP_OK) return rc;
  const char* back = (const char*)h->back.data();
  for (int b = 0; b < batch; ++b) {
    memcpy(&n_clusters_out[b], back + o_ncl + sizeof(int32_t) * b, sizeof(int32_t));
    if (n[b] == 0) continue;
    const size_t o = sizeof(int32_t) * (size_t)desc[(size_t)b].off, len = sizeof(int32_t) * (size_t)n[b];
    memcpy(labels_out[b], back + o, len);
    if (count_out && count_out[b]) memcpy(count_out[b], back + o_cnt + o, len);
    if (root_out && root_out[b]) memcpy(root_out[b], back + o_root + o, len);
  }
  return TEASER_HIP_OK;
}

}  // extern "C"
