// icp_fps.hip -- host side of farthest-point down-sampling on the ICP handle (include/teaser_hip.h, "Farthest-point
// down-sampling").  Kernels: kernels_fps.hip on the device code of icp_fps_device.h; design and launch count in
// DESIGN.md section 27.
//
// One call: the clouds of n <= "fps_resident_max" points go into ONE launch of the resident kernel, the others into one
// launch per round, max K of them; everything on the handle's stream, one upload, one copy back, one synchronisation.
// The launch count is a function of (n, K, the option) only.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_common.h"
#include "icp_fps_device.h"
#include "icp_host.h"
#include "icp_internal.h"
#include "teaser_hip.h"

using namespace thip;

static_assert(sizeof(teaser_icp_fps_params_c) == 8, "the header states the record's size");

extern "C" {

int32_t teaser_hip_icp_farthest_point_down_sample_batch(teaser_hip_icp* h, int32_t batch, const double* const* points,
                                                        const int32_t* n, const teaser_icp_fps_params_c* params,
                                                        int32_t* const* index_out, double* const* sel_dist_out,
                                                        double* const* final_dist_out) {
  const CallStart c = begin_cloud_call(h, batch, points, n, false);
  if (c.done) return c.rc;
  const int64_t total = c.total;
  int32_t rc = TEASER_HIP_OK;
  if (!params) return fail(h, TEASER_HIP_ERR_BAD_ARG, "params must not be NULL");
  if (total >= INT32_MAX) return fail(h, TEASER_HIP_ERR_BAD_ARG, "too many points in one call");
  for (int b = 0; b < batch; ++b) {
    const teaser_icp_fps_params_c& p = params[b];
    if (p.num_samples < 0 || p.num_samples > n[b])
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "num_samples must lie in [0, n]" + at(b));
    if (p.num_samples == 0) continue;
    if (p.start_index < 0 || p.start_index >= n[b])
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "start_index must lie in [0, n)" + at(b));
    if (!index_out || !index_out[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "index_out is NULL" + at(b));
  }

  // ---- descriptors and the route split ----
  std::vector<FpsDesc> desc((size_t)batch);
  std::vector<int32_t> map_res, map_blk;  // block -> cloud of the resident launch and of a round's launch
  int64_t off = 0, samples = 0;
  int32_t rounds = 0;
  bool want_fin = false;
  for (int b = 0; b < batch; ++b) {
    FpsDesc& d = desc[(size_t)b];
    memset(&d, 0, sizeof(d));
    d.n = n[b];
    d.k = params[b].num_samples;
    d.start = params[b].start_index;
    d.off = off;
    d.out_off = samples;
    off += n[b];
    samples += d.k;
    if (d.k == 0) continue;  // nothing is written for the cloud
    want_fin = want_fin || (final_dist_out && final_dist_out[b]);
    if (d.n <= h->fps_resident_max) {
      map_res.push_back(b);
    } else {
      d.nblk = (d.n + kFpsBlockPoints - 1) / kFpsBlockPoints;
      d.blk_off = (int32_t)map_blk.size();
      map_blk.insert(map_blk.end(), (size_t)d.nblk, b);
      rounds = std::max(rounds, d.k);
    }
  }
  if (samples == 0) return TEASER_HIP_OK;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");

  // ---- the launches ----
  const int n_res = (int)map_res.size(), n_blk = (int)map_blk.size();
  const size_t T = (size_t)total, S = (size_t)samples;
  // B_X: sel_dist, index (padded to a double), final_dist; the last is the streamed route's d and is copied back only
  // when a cloud asks for it
  const size_t o_idx = sizeof(double) * S, o_fin = o_idx + 8 * ((sizeof(int32_t) * S + 7) / 8),
               out_bytes = o_fin + sizeof(double) * T;
  size_t bytes[B_COUNT] = {};
  bytes[B_X] = out_bytes;
  bytes[B_Q] = 24 * T;
  bytes[B_KDESC] = sizeof(FpsDesc) * batch;
  bytes[B_KBLK] = sizeof(int32_t) * (size_t)(n_res + n_blk);
  bytes[B_PARTIALS] = sizeof(FpsBest) * 2 * (size_t)n_blk;
  if ((rc = ensure_buffers(h, bytes, "hipMalloc failed (farthest-point buffers)")) != TEASER_HIP_OK) return rc;
  hipStream_t s = h->stream;
  DevBuf* B = h->buf;
  char* out = B[B_X].as<char>();
  h->stage.resize(3 * T);
  if ((rc = upload_points(h, batch, points, n, 0, "hipMemcpyAsync (points)")) != TEASER_HIP_OK) return rc;
  map_res.insert(map_res.end(), map_blk.begin(), map_blk.end());
  FCHK(h, hipMemcpyAsync(B[B_KDESC].p, desc.data(), bytes[B_KDESC], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (descriptors)");
  FCHK(h, hipMemcpyAsync(B[B_KBLK].p, map_res.data(), bytes[B_KBLK], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (block maps)");
  const FpsDesc* dd = B[B_KDESC].as<FpsDesc>();
  const int32_t* dmap = B[B_KBLK].as<int32_t>();
  const double* pts = B[B_Q].as<double>();
  double *d_sel = (double*)out, *d_fin = (double*)(out + o_fin);
  int32_t* d_idx = (int32_t*)(out + o_idx);
  launch_fps_resident(s, dd, dmap, n_res, pts, d_idx, d_sel, want_fin ? d_fin : nullptr);
  for (int r = 0; r < rounds; ++r)
    launch_fps_round(s, dd, dmap + n_res, n_blk, r, pts, d_idx, d_sel, d_fin, B[B_PARTIALS].as<FpsBest>());
  if ((rc = copy_back(h, 0, want_fin ? out_bytes : o_fin, "farthest-point down-sampling",
                      "kernel launch (farthest-point down-sampling)")) != TEASER_HIP_OK)
    return rc;
  const char* back = (const char*)h->back.data();
  for (int b = 0; b < batch; ++b) {
    const FpsDesc& d = desc[(size_t)b];
    if (d.k == 0) continue;
    memcpy(index_out[b], back + o_idx + sizeof(int32_t) * (size_t)d.out_off, sizeof(int32_t) * (size_t)d.k);
    if (sel_dist_out && sel_dist_out[b])
      memcpy(sel_dist_out[b], back + sizeof(double) * (size_t)d.out_off, sizeof(double) * (size_t)d.k);
    if (final_dist_out && final_dist_out[b])
      memcpy(final_dist_out[b], back + o_fin + sizeof(double) * (size_t)d.off, sizeof(double) * (size_t)d.n);
  }
  return TEASER_HIP_OK;
}

}  // extern "C"
