// icp_keypoints.hip -- host side of ISS keypoint detection on the ICP handle (include/teaser_hip.h, "ISS keypoints").
// Kernels: kernels_keypoints.hip on the device code of icp_iss_device.h; design and launch count in DESIGN.md section 19.
//
// One call is at most two stages.  Stage A only when a cloud asks for automatic radii: the hash-grid index and the self
// k-NN launches of kernels_outlier.hip with k = 2 over THOSE clouds, the blocked sum of the nearest-neighbour
// distances, and one copy back of a double per cloud.  Stage B over every cloud: per cloud the grids of r_s and r_n
// (set_grid), the key layout, keys, one stable sort of 2 n entries, the gather, the saliency and the suppression
// kernels, and one copy back.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "host_common.h"
#include "icp_host.h"
#include "icp_internal.h"
#include "icp_iss_device.h"
#include "teaser_hip.h"

using namespace thip;

static_assert(sizeof(teaser_icp_iss_params_c) == 40, "the header states the record's size");

namespace {

bool auto_radii(const teaser_icp_iss_params_c& p) { return p.salient_radius == 0 || p.non_max_radius == 0; }

// Stage A: res[b] of the clouds with want[b] (n[b] >= 2), through self k-NN with k = 2 over those clouds alone.
int32_t resolutions(teaser_hip_icp* h, int32_t batch, const double* const* points, const int32_t* n,
                    const std::vector<char>& want, std::vector<double>& res) {
  std::vector<int32_t> nb((size_t)batch), k((size_t)batch, 2);
  for (int b = 0; b < batch; ++b) nb[(size_t)b] = want[(size_t)b] ? n[b] : 0;
  IcpIndex ix;
  KnnLayout L;
  L.res_per_cloud = 1;  // cleared and copied back together with the worklist counter behind them
  int32_t rc = run_self_knn(h, batch, points, nb.data(), k.data(), nullptr, ix, L);
  if (rc != TEASER_HIP_OK) return rc;
  DevBuf* B = h->buf;
  char* out = B[B_X].as<char>();
  launch_iss_resolution(h->stream, B[B_DESC].as<IcpDesc>(), B[B_STATE].as<IcpKnnDesc>(), B[B_TBLK].as<int32_t>(),
                        (int)ix.tblk_prob.size(), batch, (const double*)(out + L.d2), B[B_PARTIALS].as<double>(),
                        (double*)(out + L.res));
  if ((rc = copy_back(h, L.res, L.idx - L.res, "resolution", "kernel launch (resolution)",
                      "hipMemcpyAsync (resolution)")) != TEASER_HIP_OK)
    return rc;
  read_fallbacks(h, L.counter - L.res);
  for (int b = 0; b < batch; ++b)
    if (want[(size_t)b]) res[(size_t)b] = h->back[(size_t)b];
  return TEASER_HIP_OK;
}

}  // namespace

extern "C" {

int32_t teaser_hip_icp_iss_params_default(teaser_icp_iss_params_c* p) {
  if (!p) return TEASER_HIP_ERR_BAD_ARG;
  memset(p, 0, sizeof(*p));
  p->gamma_21 = p->gamma_32 = 0.975;
  p->min_neighbors = 5;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_icp_iss_keypoints_batch(teaser_hip_icp* h, int32_t batch, const double* const* points,
                                           const int32_t* n, const teaser_icp_iss_params_c* params,
                                           uint8_t* const* keep_out, int32_t* n_keypoints_out,
                                           double* const* saliency_out, int32_t* const* count_out, double* radii_out) {
  const CallStart c = begin_cloud_call(h, batch, points, n, true);
  if (c.done) return c.rc;
  const int64_t total = c.total;
  int32_t rc = TEASER_HIP_OK;
  if (!params) return fail(h, TEASER_HIP_ERR_BAD_ARG, "params must not be NULL");
  if (!n_keypoints_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_keypoints_out must not be NULL");
  if (2 * total >= INT32_MAX) return fail(h, TEASER_HIP_ERR_BAD_ARG, "too many points in one call");
  for (int b = 0; b < batch; ++b) {
    const teaser_icp_iss_params_c& p = params[b];
    if (!radius_ok(p.salient_radius))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "salient_radius must be >= 0 and finite like its square" + at(b));
    if (!radius_ok(p.non_max_radius))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "non_max_radius must be >= 0 and finite like its square" + at(b));
    if (!std::isfinite(p.gamma_21)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "gamma_21 must be finite" + at(b));
    if (!std::isfinite(p.gamma_32)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "gamma_32 must be finite" + at(b));
    if (p.min_neighbors < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "min_neighbors must be >= 0" + at(b));
    if (p.reserved != 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "reserved must be 0" + at(b));
    if (n[b] > 0 && (!keep_out || !keep_out[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "keep_out is NULL" + at(b));
  }
  const bool have_device_work = total > 0;
  if (have_device_work) FCHK(h, hipSetDevice(h->device), "hipSetDevice");

  // ---- radii: stage A for the clouds that ask for it ----
  const double kNaN = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> res((size_t)batch, kNaN), rs((size_t)batch), rn((size_t)batch);
  std::vector<char> want((size_t)batch, 0);
  bool any_auto = false;
  for (int b = 0; b < batch; ++b) {
    if (!auto_radii(params[b])) continue;
    res[(size_t)b] = 0.0;  // n < 2
    want[(size_t)b] = n[b] >= 2;
    any_auto |= n[b] >= 2;
  }
  if (any_auto && (rc = resolutions(h, batch, points, n, want, res)) != TEASER_HIP_OK) return rc;
  for (int b = 0; b < batch; ++b) {
    const bool a = auto_radii(params[b]);
    rs[(size_t)b] = a ? 6.0 * res[(size_t)b] : params[b].salient_radius;
    rn[(size_t)b] = a ? 4.0 * res[(size_t)b] : params[b].non_max_radius;
    if (!radius_ok(rs[(size_t)b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "salient_radius (automatic) is not finite like its square" + at(b));
    if (!radius_ok(rn[(size_t)b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "non_max_radius (automatic) is not finite like its square" + at(b));
  }

  // ---- descriptors, grids and the key layout ----
  std::vector<IssDesc> desc((size_t)batch);
  std::vector<int32_t> blk;
  std::vector<int> sbits(3 * (size_t)batch, 0), nbits(3 * (size_t)batch, 0);
  int key_bits = 0;
  bool any_active = false;
  int64_t off = 0;
  for (int b = 0; b < batch; ++b) {
    IssDesc& d = desc[(size_t)b];
    memset(&d, 0, sizeof(d));
    d.n = n[b];
    d.min_nb = params[b].min_neighbors;
    d.off = off;
    d.blk_off = (int32_t)blk.size();
    d.g21 = params[b].gamma_21;
    d.g32 = params[b].gamma_32;
    const double r_s = rs[(size_t)b], r_n = rn[(size_t)b];
    d.active = n[b] > 0 && r_s * r_s > 0 && r_n * r_n > 0;
    if (d.active) {
      int bs[3], bn[3];
      make_sorted_grid(d.gs, points[b], n[b], r_s, bs);
      make_sorted_grid(d.gn, points[b], n[b], r_n, bn);
      for (int c = 0; c < 3; ++c) sbits[3 * (size_t)b + c] = bs[c], nbits[3 * (size_t)b + c] = bn[c];
      key_bits = std::max(key_bits, std::max(bs[0] + bs[1] + bs[2], bn[0] + bn[1] + bn[2]));
      any_active = true;
    }
    for (int k = 0; k < (n[b] + kIssBlock - 1) / kIssBlock; ++k) blk.push_back(b);
    off += n[b];
  }
  const int id_bits = key_bits_for((uint64_t)(2 * (int64_t)batch - 1));
  const int bits = key_bits + id_bits;
  if (bits > 63)
    for (int b = 0; b < batch; ++b) {  // the cloud and the radius whose grid is the widest
      const int ws = sbits[3 * (size_t)b] + sbits[3 * (size_t)b + 1] + sbits[3 * (size_t)b + 2],
                wn = nbits[3 * (size_t)b] + nbits[3 * (size_t)b + 1] + nbits[3 * (size_t)b + 2];
      if (std::max(ws, wn) == key_bits)
        return fail(h, TEASER_HIP_ERR_BAD_ARG,
                    std::string(ws == key_bits ? "salient_radius" : "non_max_radius") +
                        " is too small for the cloud's extent: the cell keys of the call need " + std::to_string(bits) +
                        " bits (at most 63)" + at(b));
    }
  for (int b = 0; b < batch; ++b) {
    IssDesc& d = desc[(size_t)b];
    d.gs.base = d.off;
    d.gn.base = total + d.off;
    d.gs.id = (uint64_t)b << key_bits;
    d.gn.id = (uint64_t)(batch + b) << key_bits;
    d.gs.shift[1] = sbits[3 * (size_t)b + 2];
    d.gs.shift[0] = sbits[3 * (size_t)b + 2] + sbits[3 * (size_t)b + 1];
    d.gn.shift[1] = nbits[3 * (size_t)b + 2];
    d.gn.shift[0] = nbits[3 * (size_t)b + 2] + nbits[3 * (size_t)b + 1];
  }

  // ---- outputs a call without device work gives ----
  for (int b = 0; b < batch; ++b) {
    n_keypoints_out[b] = 0;
    if (radii_out) radii_out[3 * b] = res[(size_t)b], radii_out[3 * b + 1] = rs[(size_t)b], radii_out[3 * b + 2] = rn[(size_t)b];
    if (n[b] == 0) continue;
    memset(keep_out[b], 0, (size_t)n[b]);
    if (saliency_out && saliency_out[b]) memset(saliency_out[b], 0, sizeof(double) * (size_t)n[b]);
    if (count_out && count_out[b]) memset(count_out[b], 0, sizeof(int32_t) * 2 * (size_t)n[b]);
  }
  if (!any_active) return TEASER_HIP_OK;

  // ---- stage B ----
  const int n_blk = (int)blk.size();
  const size_t T = (size_t)total;
  // B_X: saliencies, counts (m, cnt), keypoint counts, mask bytes
  const size_t o_cnt = sizeof(double) * T, o_kept = o_cnt + sizeof(int32_t) * 2 * T,
               o_keep = o_kept + sizeof(int32_t) * batch, out_bytes = o_keep + T;
  size_t bytes[B_COUNT] = {};
  bytes[B_X] = out_bytes;
  bytes[B_Q] = 24 * T;
  bytes[B_KDESC] = sizeof(IssDesc) * batch;
  bytes[B_KBLK] = sizeof(int32_t) * n_blk;
  bytes[B_KKEY] = bytes[B_KSKEY] = 8 * 2 * T;
  bytes[B_KIOTA] = bytes[B_KSIDX] = 4 * 2 * T;
  bytes[B_KSPTS] = 24 * 2 * T;
  bytes[B_KTEMP] = iss_sort_temp_bytes(2 * total);
  if ((rc = ensure_buffers(h, bytes, "hipMalloc failed (keypoint buffers)")) != TEASER_HIP_OK) return rc;
  hipStream_t s = h->stream;
  DevBuf* B = h->buf;
  char* out = B[B_X].as<char>();
  h->stage.resize(3 * T);
  if ((rc = upload_points(h, batch, points, n, 0, "hipMemcpyAsync (points)")) != TEASER_HIP_OK) return rc;
  FCHK(h, hipMemcpyAsync(B[B_KDESC].p, desc.data(), bytes[B_KDESC], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (descriptors)");
  FCHK(h, hipMemcpyAsync(B[B_KBLK].p, blk.data(), bytes[B_KBLK], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (block map)");
  FCHK(h, hipMemsetAsync(out, 0, out_bytes, s), "hipMemsetAsync");  // the clouds without neighbours keep their zeros
  const IssDesc* dd = B[B_KDESC].as<IssDesc>();
  const int32_t* dblk = B[B_KBLK].as<int32_t>();
  launch_iss_keys(s, dd, dblk, n_blk, B[B_Q].as<double>(), total, B[B_KKEY].as<uint64_t>(), B[B_KIOTA].as<int32_t>());
  FCHK(h, launch_iss_sort(s, B[B_KTEMP].p, bytes[B_KTEMP], 2 * total, std::max(bits, 1), B[B_KKEY].as<uint64_t>(),
                          B[B_KIOTA].as<int32_t>(), B[B_KSKEY].as<uint64_t>(), B[B_KSIDX].as<int32_t>()),
       "keypoint sort");
  launch_iss_gather(s, total, B[B_Q].as<double>(), B[B_KSIDX].as<int32_t>(), B[B_KSPTS].as<double>());
  launch_iss_saliency(s, dd, dblk, n_blk, B[B_KSKEY].as<uint64_t>(), B[B_KSIDX].as<int32_t>(),
                      B[B_KSPTS].as<double>(), (double*)out, (int32_t*)(out + o_cnt));
  launch_iss_suppress(s, dd, dblk, n_blk, total, B[B_KSKEY].as<uint64_t>(), B[B_KSIDX].as<int32_t>(),
                      B[B_KSPTS].as<double>(), (const double*)out, (int32_t*)(out + o_cnt), (uint8_t*)(out + o_keep),
                      (int32_t*)(out + o_kept));
  if ((rc = copy_back(h, 0, out_bytes, "keypoint detection", "kernel launch (keypoints)")) != TEASER_HIP_OK) return rc;
  const char* back = (const char*)h->back.data();
  for (int b = 0; b < batch; ++b) {
    if (n[b] == 0) continue;
    const size_t o = (size_t)desc[(size_t)b].off;
    memcpy(keep_out[b], back + o_keep + o, (size_t)n[b]);
    memcpy(&n_keypoints_out[b], back + o_kept + sizeof(int32_t) * b, sizeof(int32_t));
    if (saliency_out && saliency_out[b]) memcpy(saliency_out[b], back + sizeof(double) * o, sizeof(double) * (size_t)n[b]);
    if (count_out && count_out[b])
      memcpy(count_out[b], back + o_cnt + sizeof(int32_t) * 2 * o, sizeof(int32_t) * 2 * (size_t)n[b]);
  }
  return TEASER_HIP_OK;
}

}  // extern "C"
