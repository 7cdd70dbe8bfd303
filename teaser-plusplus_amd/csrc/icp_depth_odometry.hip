// icp_depth_odometry.hip -- host side of depth odometry on the ICP handle (include/teaser_hip.h, "Depth odometry"):
// teaser_hip_icp_depth_odometry_pairs and the preprocessing stage alone, teaser_hip_icp_depth_odometry_pyramid_pairs.
// Kernels: kernels_depth_odometry.hip; device code: icp_depth_odometry_device.h; design, bytes moved, launch counts and
// the resource report: DESIGN.md section 40.
//
// The two depth images of every pair go up one copy each, from where they lie when their rows are not padded (a padded
// image has its rows packed into the staging array first), beside the descriptors, the initial states and the block map.
// Then the launches: preprocessing, per level its iterations (two launches each), the information matrices.  Which
// launches run follows from the options and the image sizes alone; a pair that fails or converges carries a flag on the
// device.  Result records and trace come back in the one copy of B_X (the pyramid call: the image pool), with the call's
// one synchronisation.  Every word a kernel reads has been written inside the call: the planes by the preprocessing, the
// block partials by the sums launch in front of the finishing launch that reads them, the records by the memset.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_common.h"
#include "icp_depth_odometry_device.h"
#include "icp_host.h"
#include "teaser_hip.h"

using namespace thip;

namespace {

inline size_t round_up16(size_t v) { return (v + 15) / 16 * 16; }
inline std::string pair_at(int b) { return " (pair " + std::to_string(b) + ")"; }

// What a call has on the host between its checks and its launches.
struct DodoPlan {
  std::vector<DodoDesc> desc;
  std::vector<DodoState> state;
  std::vector<int32_t> blk_pair;
  int level_blk0[kOdoMaxLevels] = {}, level_nblk[kOdoMaxLevels] = {};
  int64_t pixels = 0, img_floats = 0, blocks0 = 0, records = 0;
  size_t in_bytes = 0;
  int levels = 0, n_iter = 0;
};

int32_t check_option(teaser_hip_icp* h, const teaser_icp_depth_odometry_option_c* o) {
  if (!o) return fail(h, TEASER_HIP_ERR_BAD_ARG, "option must not be NULL");
  if (o->n_levels < 1 || o->n_levels > kOdoMaxLevels) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_levels must lie in [1, 8]");
  for (int k = 0; k < o->n_levels; ++k)
    if (o->iterations[k] < 0)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "iterations must be >= 0 (level entry " + std::to_string(k) + ")");
  if (o->reserved[0] != 0 || o->reserved[1] != 0 || o->reserved[2] != 0 || o->reserved2[0] != 0.0 || o->reserved2[1] != 0.0)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "reserved must be 0 (option)");
  if (!std::isfinite(o->depth_outlier_trunc) || !(o->depth_outlier_trunc > 0.0))
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_outlier_trunc must be finite and > 0");
  if (!std::isfinite(o->depth_huber_delta) || !(o->depth_huber_delta > 0.0))
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_huber_delta must be finite and > 0");
  if (!std::isfinite(o->depth_min) || o->depth_min < 0.0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_min must be finite and >= 0");
  if (!std::isfinite(o->depth_max)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_max must be finite");
  if (!std::isfinite(o->relative_rmse)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "relative_rmse must be finite");
  if (!std::isfinite(o->relative_fitness)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "relative_fitness must be finite");
  return TEASER_HIP_OK;
}

// The checks of a call and its plan; trace: NULL or per pair NULL or the room for its records.
int32_t make_plan(teaser_hip_icp* h, int32_t batch, const teaser_icp_depth_odometry_pair_c* pairs,
                  const teaser_icp_depth_odometry_option_c* o, const void* const* img[2],
                  teaser_icp_depth_odometry_trace_c* const* trace, DodoPlan& P) {
  static const char* const kNames[2] = {"source_depth", "target_depth"};
  if (!pairs) return fail(h, TEASER_HIP_ERR_BAD_ARG, "pairs must not be NULL");
  int32_t rc = check_option(h, o);
  if (rc != TEASER_HIP_OK) return rc;
  for (int k = 0; k < 2; ++k)
    if (!img[k]) return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string(kNames[k]) + " must not be NULL");
  const int L = o->n_levels;
  P.levels = L;
  for (int k = 0; k < L; ++k) P.n_iter += o->iterations[k];
  P.desc.resize((size_t)batch);
  P.state.resize((size_t)batch);
  std::vector<int32_t> nblk((size_t)batch * kOdoMaxLevels, 0);
  for (int b = 0; b < batch; ++b) {
    const teaser_icp_depth_odometry_pair_c& p = pairs[b];
    if (p.depth_format < 0 || p.depth_format > 1)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_format must be 0 (uint16) or 1 (float32)" + pair_at(b));
    if (p.reserved != 0 || p.reserved2 != 0.0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "reserved must be 0" + pair_at(b));
    if (p.width > kRgbdMaxSide || p.height > kRgbdMaxSide || (p.width >> (L - 1)) < 1 || (p.height >> (L - 1)) < 1)
      return fail(h, TEASER_HIP_ERR_BAD_ARG,
                  "width and height must lie in [2^(n_levels - 1), 16384]: every level needs a pixel" + pair_at(b));
    if (!std::isfinite(p.fx) || !std::isfinite(p.fy) || !(p.fx > 0.0) || !(p.fy > 0.0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "fx and fy must be finite and > 0" + pair_at(b));
    if (!std::isfinite(p.cx) || !std::isfinite(p.cy)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "cx and cy must be finite" + pair_at(b));
    for (int k = 0; k < 16; ++k)
      if (!std::isfinite(p.init[k])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "init has a non-finite entry" + pair_at(b));
    if (!std::isfinite(p.depth_scale) || !(p.depth_scale > 0.0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "depth_scale must be finite and > 0" + pair_at(b));
    const int64_t row = (int64_t)p.width * (p.depth_format == 0 ? 2 : 4);
    const int64_t given[2] = {p.source_depth_row_bytes, p.target_depth_row_bytes};
    DodoDesc& d = P.desc[(size_t)b];
    memset(&d, 0, sizeof(d));
    for (int k = 0; k < 2; ++k) {
      if (given[k] < row)
        return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string(kNames[k]) + "_row_bytes is smaller than a row" + pair_at(b));
      if (!img[k][b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string(kNames[k]) + " is NULL" + pair_at(b));
      d.in_off[k] = (int64_t)P.in_bytes;
      P.in_bytes = round_up16(P.in_bytes + (size_t)(row * p.height));
    }
    d.width = p.width, d.height = p.height, d.levels = L, d.depth_format = p.depth_format;
    d.img_off = P.img_floats, d.part_off = P.blocks0;
    d.trace_off = -1;
    if (trace && trace[b] && P.n_iter > 0) {
      d.trace_off = P.records;
      P.records += P.n_iter;
    }
    d.fx = p.fx, d.fy = p.fy, d.cx = p.cx, d.cy = p.cy;
    d.trunc = o->depth_outlier_trunc, d.delta = o->depth_huber_delta, d.depth_min = o->depth_min, d.depth_max = o->depth_max;
    d.rel_rmse = o->relative_rmse, d.rel_fitness = o->relative_fitness;
    d.depth_scale = (float)p.depth_scale;
    d.thr = (float)(2.0 * o->depth_outlier_trunc);
    for (int l = 0; l < L; ++l) nblk[(size_t)b * kOdoMaxLevels + l] = (int32_t)dodo_blocks(d, l);
    P.pixels += dodo_n(d, 0);
    P.img_floats += kDodoPlanes * odo_pyramid_pixels(d.width, d.height, L);
    P.blocks0 += dodo_blocks(d, 0);
    if (P.pixels > INT32_MAX) return fail(h, TEASER_HIP_ERR_BAD_ARG, "more than 2^31 - 1 pixels in one call");
    DodoState& st = P.state[(size_t)b];
    memset(&st, 0, sizeof(st));
    memcpy(st.T, p.init, sizeof(st.T));
    st.T[12] = st.T[13] = st.T[14] = 0.0, st.T[15] = 1.0;  // row 3 is not read
  }
  for (int l = 0; l < L; ++l) {  // the blocks of level 0 of all pairs, then level 1, ...
    P.level_blk0[l] = (int)P.blk_pair.size();
    for (int b = 0; b < batch; ++b) {
      P.desc[(size_t)b].blk_off[l] = (int32_t)P.blk_pair.size() - P.level_blk0[l];
      P.blk_pair.insert(P.blk_pair.end(), (size_t)nblk[(size_t)b * kOdoMaxLevels + l], b);
    }
    P.level_nblk[l] = (int)P.blk_pair.size() - P.level_blk0[l];
  }
  return TEASER_HIP_OK;
}

// Buffers, uploads and the preprocessing launches; `out_bytes` of B_X are cleared.  Fills `a`.
int32_t start_call(teaser_hip_icp* h, int32_t batch, const teaser_icp_depth_odometry_pair_c* pairs, const void* const* img[2],
                   const DodoPlan& P, size_t out_bytes, DodoArgs& a) {
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  size_t bytes[B_COUNT] = {};
  bytes[B_RGBD_DESC] = sizeof(DodoDesc) * (size_t)batch;
  bytes[B_STATE] = sizeof(DodoState) * (size_t)batch;
  bytes[B_BLK] = sizeof(int32_t) * P.blk_pair.size();
  bytes[B_RGBD_IN] = P.in_bytes;
  bytes[B_ODO_IMG] = sizeof(float) * (size_t)P.img_floats;
  bytes[B_PARTIALS] = sizeof(double) * kOdoSums * (size_t)P.blocks0;
  bytes[B_X] = std::max<size_t>(out_bytes, 8);
  int32_t rc = ensure_buffers(h, bytes, "hipMalloc failed (depth odometry buffers)");
  if (rc != TEASER_HIP_OK) return rc;
  DevBuf* B = h->buf;
  hipStream_t s = h->stream;
  FCHK(h, hipMemcpyAsync(B[B_RGBD_DESC].p, P.desc.data(), bytes[B_RGBD_DESC], hipMemcpyHostToDevice, s), "hipMemcpyAsync (inputs)");
  FCHK(h, hipMemcpyAsync(B[B_STATE].p, P.state.data(), bytes[B_STATE], hipMemcpyHostToDevice, s), "hipMemcpyAsync (inputs)");
  FCHK(h, hipMemcpyAsync(B[B_BLK].p, P.blk_pair.data(), bytes[B_BLK], hipMemcpyHostToDevice, s), "hipMemcpyAsync (inputs)");
  // an image without row padding goes up from where it lies; a padded one has its rows packed into the staging array first
  size_t staged = 0;
  for (int b = 0; b < batch; ++b) {
    const teaser_icp_depth_odometry_pair_c& p = pairs[b];
    const int64_t row = (int64_t)p.width * (p.depth_format == 0 ? 2 : 4);
    const int64_t given[2] = {p.source_depth_row_bytes, p.target_depth_row_bytes};
    for (int k = 0; k < 2; ++k)
      if (given[k] != row) staged += round_up16((size_t)(row * p.height));
  }
  h->stage.resize((staged + 7) / 8);
  unsigned char* stage = (unsigned char*)h->stage.data();
  size_t at = 0;
  for (int b = 0; b < batch; ++b) {
    const teaser_icp_depth_odometry_pair_c& p = pairs[b];
    const DodoDesc& d = P.desc[(size_t)b];
    const int64_t row = (int64_t)p.width * (p.depth_format == 0 ? 2 : 4);
    const int64_t given[2] = {p.source_depth_row_bytes, p.target_depth_row_bytes};
    for (int k = 0; k < 2; ++k) {
      const void* from = img[k][b];
      if (given[k] != row) {
        for (int64_t r = 0; r < d.height; ++r) memcpy(stage + at + r * row, (const unsigned char*)img[k][b] + r * given[k], (size_t)row);
        from = stage + at;
        at += round_up16((size_t)(row * d.height));
      }
      FCHK(h, hipMemcpyAsync(B[B_RGBD_IN].as<unsigned char>() + d.in_off[k], from, (size_t)(row * d.height), hipMemcpyHostToDevice, s),
           "hipMemcpyAsync (images)");
    }
  }
  if (out_bytes) FCHK(h, hipMemsetAsync(B[B_X].p, 0, out_bytes, s), "hipMemsetAsync (results)");
  memset(&a, 0, sizeof(a));
  a.desc = B[B_RGBD_DESC].as<DodoDesc>(), a.state = B[B_STATE].as<DodoState>(), a.blk_pair = B[B_BLK].as<int32_t>();
  a.in = B[B_RGBD_IN].as<unsigned char>(), a.img = B[B_ODO_IMG].as<float>(), a.part = B[B_PARTIALS].as<double>();
  a.results = (teaser_icp_depth_odometry_result_c*)B[B_X].p;
  a.trace = (teaser_icp_depth_odometry_trace_c*)(B[B_X].as<char>() + sizeof(teaser_icp_depth_odometry_result_c) * (size_t)batch);
  a.batch = batch, a.levels = P.levels;
  memcpy(a.level_blk0, P.level_blk0, sizeof(a.level_blk0));
  memcpy(a.level_nblk, P.level_nblk, sizeof(a.level_nblk));
  launch_dodo_preprocess(s, a);
  return TEASER_HIP_OK;
}

}  // namespace

extern "C" {

int32_t teaser_hip_icp_depth_odometry_option_default(teaser_icp_depth_odometry_option_c* o) {
  if (!o) return TEASER_HIP_ERR_BAD_ARG;
  memset(o, 0, sizeof(*o));
  o->n_levels = 3;
  o->iterations[0] = 10, o->iterations[1] = 5, o->iterations[2] = 3;
  o->depth_outlier_trunc = 0.07;
  o->depth_huber_delta = 0.05;
  o->depth_min = 0.0;
  o->depth_max = 3.0;
  o->relative_rmse = 1e-6;
  o->relative_fitness = 1e-6;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_icp_depth_odometry_pairs(teaser_hip_icp* h, int32_t batch, const teaser_icp_depth_odometry_pair_c* pairs,
                                            const teaser_icp_depth_odometry_option_c* option, const void* const* source_depth,
                                            const void* const* target_depth, teaser_icp_depth_odometry_result_c* results,
                                            teaser_icp_depth_odometry_trace_c* const* trace_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (batch < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0");
  if (batch == 0) return TEASER_HIP_OK;
  if (!results) return fail(h, TEASER_HIP_ERR_BAD_ARG, "results must not be NULL");
  const void* const* img[2] = {source_depth, target_depth};
  DodoPlan P;
  int32_t rc = make_plan(h, batch, pairs, option, img, trace_out, P);
  if (rc != TEASER_HIP_OK) return rc;
  const size_t o_trace = sizeof(teaser_icp_depth_odometry_result_c) * (size_t)batch;
  const size_t o_end = o_trace + sizeof(teaser_icp_depth_odometry_trace_c) * (size_t)P.records;
  DodoArgs a;
  if ((rc = start_call(h, batch, pairs, img, P, o_end, a)) != TEASER_HIP_OK) return rc;
  int iter = 0;
  for (int l = P.levels - 1; l >= 0; --l) {
    const int n = option->iterations[P.levels - 1 - l];
    for (int k = 0; k < n; ++k) launch_dodo_iteration(h->stream, a, l, iter++, k == 0, k == n - 1);
  }
  launch_dodo_information(h->stream, a);
  if ((rc = copy_back(h, 0, o_end, "depth odometry", "kernel launch (depth odometry)")) != TEASER_HIP_OK) return rc;
  const char* back = (const char*)h->back.data();
  memcpy(results, back, o_trace);
  for (int b = 0; b < batch; ++b)
    if (P.desc[(size_t)b].trace_off >= 0)
      memcpy(trace_out[b], back + o_trace + sizeof(teaser_icp_depth_odometry_trace_c) * (size_t)P.desc[(size_t)b].trace_off,
             sizeof(teaser_icp_depth_odometry_trace_c) * (size_t)P.n_iter);
  return TEASER_HIP_OK;
}

int32_t teaser_hip_icp_depth_odometry_pyramid_pairs(teaser_hip_icp* h, int32_t batch,
                                                    const teaser_icp_depth_odometry_pair_c* pairs,
                                                    const teaser_icp_depth_odometry_option_c* option,
                                                    const void* const* source_depth, const void* const* target_depth,
                                                    float* const* images_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (batch < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0");
  if (batch == 0) return TEASER_HIP_OK;
  if (!images_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "images_out must not be NULL");
  for (int b = 0; b < batch; ++b)
    if (!images_out[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "images_out is NULL" + pair_at(b));
  const void* const* img[2] = {source_depth, target_depth};
  DodoPlan P;
  int32_t rc = make_plan(h, batch, pairs, option, img, nullptr, P);
  if (rc != TEASER_HIP_OK) return rc;
  DodoArgs a;
  if ((rc = start_call(h, batch, pairs, img, P, 0, a)) != TEASER_HIP_OK) return rc;
  const size_t bytes = sizeof(float) * (size_t)P.img_floats;
  h->back.resize((bytes + 7) / 8);
  FCHK(h, hipGetLastError(), "kernel launch (depth odometry pyramid)");
  FCHK(h, hipMemcpyAsync(h->back.data(), h->buf[B_ODO_IMG].p, bytes, hipMemcpyDeviceToHost, h->stream), "hipMemcpyAsync (results)");
  FCHK(h, hipStreamSynchronize(h->stream), "depth odometry pyramid");
  for (int b = 0; b < batch; ++b) {
    const DodoDesc& d = P.desc[(size_t)b];
    memcpy(images_out[b], (const float*)h->back.data() + d.img_off,
           sizeof(float) * kDodoPlanes * (size_t)odo_pyramid_pixels(d.width, d.height, d.levels));
  }
  return TEASER_HIP_OK;
}

}  // extern "C"
