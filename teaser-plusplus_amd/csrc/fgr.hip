// fgr.hip -- host side of Fast Global Registration on correspondences (include/teaser_hip.h, "Fast Global Registration
// on correspondences"): the handle, the entry checks, ONE upload (descriptors, route lists, both clouds, the pairs), the
// launches of the normalisation, of the resident route (one launch) and of the streamed route (two launches an
// iteration, enqueued back to back), ONE download of the per-problem state and ONE synchronisation.  The stage call
// runs the same launches with a log buffer and downloads the log and the records as well.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fgr_device.h"
#include "packed_call.h"
#include "teaser_hip.h"

using namespace thip;

struct teaser_hip_fgr : HandleBase {
  DevBuf in, pairs, work, state, log;
  HostBuf stage, back;  // page-locked: the upload and the download stay asynchronous until the one synchronisation
  int64_t resident_max_corr = FGR_RES_DEFAULT;
};

namespace thip {

// The route of a problem: 0 none (not optimised), 1 resident, 2 streamed.
inline int fgr_route(int32_t ncorr, int64_t resident_max_corr) {
  if (ncorr < FGR_MIN_CORR) return 0;
  return ncorr <= resident_max_corr ? 1 : 2;
}

}  // namespace thip

namespace {

const Knob<teaser_hip_fgr> kKnobs[] = {{"resident_max_corr", 0, FGR_RES_BOUND, &teaser_hip_fgr::resident_max_corr}};

void params_default(teaser_fgr_params_c* p) {
  memset(p, 0, sizeof(*p));
  p->division_factor = 1.4;
  p->maximum_correspondence_distance = 0.025;
  p->use_absolute_scale = 0;
  p->decrease_mu = 1;
  p->iteration_number = 64;
}

struct Stage {  // the stage call's outputs; all NULL in the full call
  int32_t n = -1;
  double *mu = nullptr, *A = nullptr, *g = nullptr, *xi = nullptr, *trans = nullptr, *p_out = nullptr, *q_out = nullptr;
  int32_t* flag = nullptr;
};

int32_t run(teaser_hip_fgr* h, int32_t batch, const double* const* src, const int32_t* n_src, const double* const* dst,
            const int32_t* n_dst, const int32_t* const* corr, const int32_t* n_corr, const teaser_fgr_params_c* params,
            teaser_fgr_result_c* out, const Stage& sg) {
  const int32_t r0 = begin_call(h, batch);
  if (r0 != TEASER_HIP_OK) return r0;
  const bool staged = sg.n >= 0;
  if (batch == 0) return TEASER_HIP_OK;
  if (!staged && !out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "out must not be NULL");
  if (!n_src) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src must not be NULL");
  if (!n_dst) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_dst must not be NULL");
  if (!n_corr) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_corr must not be NULL");
  if (!params) return fail(h, TEASER_HIP_ERR_BAD_ARG, "params must not be NULL");
  std::vector<FgrDesc> desc((size_t)batch);
  std::vector<int32_t> res_idx, str_idx;
  int64_t ns = 0, nt = 0, nc = 0, cblk = 0, pblk = 0;
  int max_cloud_blk = 0, max_pair_blk = 0, max_res_blk = 0, max_str_blk = 0, max_str_iter = 0;
  for (int b = 0; b < batch; ++b) {
    const teaser_fgr_params_c& q = params[b];
    if (!(std::isfinite(q.division_factor) && q.division_factor > 1))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "division_factor must be finite and > 1" + at(b));
    if (!(std::isfinite(q.maximum_correspondence_distance) && q.maximum_correspondence_distance > 0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "maximum_correspondence_distance must be finite and > 0" + at(b));
    if (q.iteration_number < 0 || q.iteration_number > FGR_MAX_ITER)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "iteration_number must be in 0 .. 1024" + at(b));
    if (q.use_absolute_scale != 0 && q.use_absolute_scale != 1)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "use_absolute_scale must be 0 or 1" + at(b));
    if (q.decrease_mu != 0 && q.decrease_mu != 1)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "decrease_mu must be 0 or 1" + at(b));
    if (staged && sg.n > q.iteration_number)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must be in 0 .. iteration_number" + at(b));
    if (n_src[b] <= 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src must be > 0: the source is empty" + at(b));
    if (n_dst[b] <= 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_dst must be > 0: the target is empty" + at(b));
    if (n_corr[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_corr must be >= 0" + at(b));
    if (!src || !src[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "src is NULL" + at(b));
    if (!dst || !dst[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst is NULL" + at(b));
    if (n_corr[b] > 0 && (!corr || !corr[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "corr is NULL" + at(b));
    if (!finite_points(src[b], n_src[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "src has non-finite points" + at(b));
    if (!finite_points(dst[b], n_dst[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst has non-finite points" + at(b));
    if (n_corr[b] > 0 && check_pairs(h, b, corr[b], n_corr[b], n_src[b], n_dst[b]) != TEASER_HIP_OK)
      return TEASER_HIP_ERR_BAD_ARG;  // the message is check_pairs's
    FgrDesc& d = desc[(size_t)b];
    memset(&d, 0, sizeof(d));
    d.src_off = ns;
    d.dst_off = nt;
    d.corr_off = nc;
    const int sb = (n_src[b] + FGR_BLOCK - 1) / FGR_BLOCK, tb = (n_dst[b] + FGR_BLOCK - 1) / FGR_BLOCK,
              pb = (n_corr[b] + FGR_BLOCK - 1) / FGR_BLOCK;
    d.sblk_off = cblk;
    d.tblk_off = cblk + sb;
    d.pblk_off = pblk;
    d.div = q.division_factor;
    d.maxd = q.maximum_correspondence_distance;
    d.n_s = n_src[b];
    d.n_t = n_dst[b];
    d.ncorr = n_corr[b];
    d.n_iter = staged ? sg.n : q.iteration_number;
    d.abs_scale = q.use_absolute_scale;
    d.decrease_mu = q.decrease_mu;
    const int route = fgr_route(n_corr[b], h->resident_max_corr);
    d.run = route != 0;
    if (route == 1) {
      res_idx.push_back(b);
      max_res_blk = std::max(max_res_blk, pb);
    } else if (route == 2) {
      str_idx.push_back(b);
      max_str_blk = std::max(max_str_blk, pb);
      max_str_iter = std::max(max_str_iter, (int)d.n_iter);
    }
    max_cloud_blk = std::max(max_cloud_blk, std::max(sb, tb));
    max_pair_blk = std::max(max_pair_blk, pb);
    ns += n_src[b];
    nt += n_dst[b];
    nc += n_corr[b];
    cblk += sb + tb;
    pblk += pb;
  }
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  hipStream_t s = h->stream;
  // ---- one upload: descriptors, the route lists, both clouds, the pairs ----
  Pack pin;
  const size_t i_desc = pin.add(sizeof(FgrDesc) * batch), i_res = pin.add(sizeof(int32_t) * batch),
               i_str = pin.add(sizeof(int32_t) * batch), i_src = pin.add(sizeof(double) * 3 * (size_t)ns),
               i_dst = pin.add(sizeof(double) * 3 * (size_t)nt),
               i_corr = pin.add(sizeof(int32_t) * 2 * (size_t)std::max<int64_t>(nc, 1));
  Pack pw;
  const size_t w_sum = pw.add(sizeof(double) * 3 * (size_t)cblk), w_max = pw.add(sizeof(double) * (size_t)cblk),
               w_part = pw.add(sizeof(double) * FGR_SUMS * (size_t)std::max<int64_t>(pblk, 1));
  const size_t log_bytes = staged ? sizeof(FgrLog) * (size_t)batch * (size_t)std::max(sg.n, 1) : 0;
  const size_t state_bytes = sizeof(FgrState) * (size_t)batch;
  if (!h->in.ensure(pin.bytes) || !h->pairs.ensure(sizeof(double) * 6 * (size_t)std::max<int64_t>(nc, 1)) ||
      !h->work.ensure(pw.bytes) || !h->state.ensure(state_bytes) || (staged && !h->log.ensure(log_bytes)))
    return fail(h, TEASER_HIP_ERR_HIP, "hipMalloc failed (FGR buffers)");
  if (!h->stage.ensure(pin.bytes) || !h->back.ensure(state_bytes))
    return fail(h, TEASER_HIP_ERR_HIP, "hipHostMalloc failed (FGR staging)");
  char* stage = h->stage.as<char>();
  memcpy(stage + i_desc, desc.data(), sizeof(FgrDesc) * batch);
  if (!res_idx.empty()) memcpy(stage + i_res, res_idx.data(), sizeof(int32_t) * res_idx.size());
  if (!str_idx.empty()) memcpy(stage + i_str, str_idx.data(), sizeof(int32_t) * str_idx.size());
  pack_rows(stage + i_src, batch, src, n_src, sizeof(double) * 3);
  pack_rows(stage + i_dst, batch, dst, n_dst, sizeof(double) * 3);
  pack_rows(stage + i_corr, batch, corr, n_corr, sizeof(int32_t) * 2);
  FCHK(h, hipMemcpyAsync(h->in.p, stage, pin.bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync (FGR inputs)");
  void* din = h->in.p;
  void* dw = h->work.p;
  FgrBufs B;
  B.desc = Pack::at<const FgrDesc>(din, i_desc);
  B.state = h->state.as<FgrState>();
  B.src = Pack::at<const double>(din, i_src);
  B.dst = Pack::at<const double>(din, i_dst);
  B.corr = Pack::at<const int32_t>(din, i_corr);
  B.pairs = h->pairs.as<double>();
  B.cloud_sum = Pack::at<double>(dw, w_sum);
  B.cloud_max = Pack::at<double>(dw, w_max);
  B.partials = Pack::at<double>(dw, w_part);
  B.log = staged && sg.n > 0 ? h->log.as<FgrLog>() : nullptr;
  B.log_stride = staged ? sg.n : 0;
  const int32_t* d_res = Pack::at<const int32_t>(din, i_res);
  const int32_t* d_str = Pack::at<const int32_t>(din, i_str);
  if (B.log) FCHK(h, hipMemsetAsync(B.log, 0, log_bytes, s), "hipMemsetAsync (FGR log)");
  launch_fgr_normalise(s, batch, max_cloud_blk, max_pair_blk, B);
  FCHK(h, launch_fgr_resident(s, (int)res_idx.size(), d_res, max_res_blk, B, staged ? 1 : 0), "FGR resident launch");
  for (int itr = 0; itr < max_str_iter; ++itr)  // no host synchronisation in between
    launch_fgr_streamed_step(s, (int)str_idx.size(), d_str, max_str_blk, B, itr);
  if (staged) launch_fgr_streamed_move(s, (int)str_idx.size(), d_str, max_str_blk, B);
  launch_fgr_finish(s, batch, B);
  FCHK(h, hipGetLastError(), "FGR kernel launch");
  // ---- one download, one synchronisation ----
  FCHK(h, hipMemcpyAsync(h->back.p, h->state.p, state_bytes, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (FGR state)");
  std::vector<FgrLog> logs;
  std::vector<double> recs;
  if (B.log) {
    logs.resize((size_t)batch * (size_t)sg.n);
    FCHK(h, hipMemcpyAsync(logs.data(), B.log, log_bytes, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (FGR log)");
  }
  if (staged && (sg.p_out || sg.q_out) && nc > 0) {
    recs.resize(6 * (size_t)nc);
    FCHK(h, hipMemcpyAsync(recs.data(), B.pairs, sizeof(double) * 6 * (size_t)nc, hipMemcpyDeviceToHost, s),
         "hipMemcpyAsync (FGR records)");
  }
  FCHK(h, hipStreamSynchronize(s), "FGR solve");
  const FgrState* st = h->back.as<FgrState>();
  for (int b = 0; b < batch && out; ++b) {
    teaser_fgr_result_c& r = out[b];
    memset(&r, 0, sizeof(r));
    memcpy(r.transformation, st[b].T, sizeof(r.transformation));
    memcpy(r.optimised, st[b].trans, sizeof(r.optimised));
    r.scale_global = st[b].scale_global;
    r.scale_start = st[b].scale_start;
    r.final_mu = st[b].mu;
    r.iterations = st[b].iterations;
    r.n_corr = n_corr[b];
    r.failed_solves = st[b].failed;
    r.flags = st[b].flags;
  }
  for (size_t q = 0; q < logs.size(); ++q) {
    const FgrLog& L = logs[q];
    if (sg.mu) sg.mu[q] = L.mu;
    if (sg.A) memcpy(sg.A + 36 * q, L.A, sizeof(L.A));
    if (sg.g) memcpy(sg.g + 6 * q, L.g, sizeof(L.g));
    if (sg.xi) memcpy(sg.xi + 6 * q, L.xi, sizeof(L.xi));
    if (sg.trans) memcpy(sg.trans + 16 * q, L.trans, sizeof(L.trans));
    if (sg.flag) sg.flag[q] = L.flag;
  }
  for (size_t c = 0; c < recs.size() / 6; ++c)
    for (int k = 0; k < 3; ++k) {
      if (sg.p_out) sg.p_out[3 * c + k] = recs[6 * c + k];
      if (sg.q_out) sg.q_out[3 * c + k] = recs[6 * c + 3 + k];
    }
  return TEASER_HIP_OK;
}

}  // namespace

extern "C" {

int32_t teaser_hip_fgr_create(int32_t device, teaser_hip_fgr** out) { return open_handle(device, out); }
int32_t teaser_hip_fgr_destroy(teaser_hip_fgr* h) { return close_handle(h); }
const char* teaser_hip_fgr_last_error(const teaser_hip_fgr* h) { return h ? h->err.c_str() : ""; }

int32_t teaser_hip_fgr_fill_scratch(teaser_hip_fgr* h, int32_t byte, int64_t* bytes_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  const ScratchSpan spans[] = {span_of(h->in),  span_of(h->pairs), span_of(h->work), span_of(h->state),
                               span_of(h->log), span_of(h->stage), span_of(h->back)};
  return fill_scratch(h, byte, spans, 7, bytes_out);
}

int32_t teaser_hip_fgr_params_default(teaser_fgr_params_c* params) {
  if (!params) return TEASER_HIP_ERR_BAD_ARG;
  params_default(params);
  return TEASER_HIP_OK;
}

int32_t teaser_hip_fgr_correspondence_batch(teaser_hip_fgr* h, int32_t batch, const double* const* src,
                                            const int32_t* n_src, const double* const* dst, const int32_t* n_dst,
                                            const int32_t* const* corr, const int32_t* n_corr,
                                            const teaser_fgr_params_c* params, teaser_fgr_result_c* out) {
  return run(h, batch, src, n_src, dst, n_dst, corr, n_corr, params, out, Stage());
}

int32_t teaser_hip_fgr_correspondence(teaser_hip_fgr* h, const double* src, int32_t n_src, const double* dst,
                                      int32_t n_dst, const int32_t* corr, int32_t n_corr,
                                      const teaser_fgr_params_c* params, teaser_fgr_result_c* out) {
  return run(h, 1, &src, &n_src, &dst, &n_dst, &corr, &n_corr, params, out, Stage());
}

int32_t teaser_hip_fgr_set_option(teaser_hip_fgr* h, const char* name, int64_t value) {
  return set_knob(h, kKnobs, name, value);
}
int32_t teaser_hip_fgr_get_option(const teaser_hip_fgr* h, const char* name, int64_t* value) {
  return get_knob(h, kKnobs, name, value);
}

int32_t teaser_hip_fgr_iterations_batch(teaser_hip_fgr* h, int32_t batch, const double* const* src,
                                        const int32_t* n_src, const double* const* dst, const int32_t* n_dst,
                                        const int32_t* const* corr, const int32_t* n_corr,
                                        const teaser_fgr_params_c* params, int32_t n, teaser_fgr_result_c* out,
                                        double* mu, double* A, double* g, double* xi, int32_t* solve_flag,
                                        double* trans, double* p_records, double* q_records) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  if (n < 0) {
    h->err.clear();
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must be in 0 .. iteration_number");
  }
  Stage sg;
  sg.n = n;
  sg.mu = mu;
  sg.A = A;
  sg.g = g;
  sg.xi = xi;
  sg.flag = solve_flag;
  sg.trans = trans;
  sg.p_out = p_records;
  sg.q_out = q_records;
  return run(h, batch, src, n_src, dst, n_dst, corr, n_corr, params, out, sg);
}

}  // extern "C"
