// ransac.hip -- host side of RANSAC registration on correspondences (include/teaser_hip.h, "RANSAC registration on
// correspondences"): the handle, the entry checks, ONE upload of the clouds and pairs and the pack launch, then the
// loop.  The trials of a problem are cut into chunks of chunk_trials; a GROUP of chunks is enqueued (hypothesis, score
// and prefix kernel each) before the host looks, with one small upload (the plan and the best carried in) and one small
// download (per chunk and problem: survivors, number of strict improvements and the first RS_LIST_CAP of them).  The
// host walks those lists with log, pow and ceil; what lies past a problem's stopping trial is dropped unread.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "packed_call.h"
#include "ransac_device.h"
#include "teaser_hip.h"

using namespace thip;

struct teaser_hip_ransac : HandleBase {
  DevBuf in, pairs, work, ctl;
  int64_t chunk_trials = 4096;
};

namespace thip {

constexpr int RS_MAX_GROUP = 4;               // chunks enqueued before the host looks
constexpr int64_t RS_GROUP_RECORDS = 1 << 21;  // ... as long as their per-trial records stay below this many

// The chunks of a group: how many, given the chunk size and the batch.
inline int rs_group_chunks(int64_t chunk, int batch) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(RS_MAX_GROUP, RS_GROUP_RECORDS / (chunk * std::max(batch, 1))));
}

// The stop rule's state of one problem and its walk over the strict improvements (the contract's loop).
struct RsWalk {
  int64_t max_iteration = 0, limit = 0;  // limit: the loop indices the loop visits, as known so far
  double est_k = 0, confidence = 0;
  int32_t ncorr = 0, ransac_n = 0;
  RsBest best{0.0, 0, 0};
  int64_t best_trial = -1, valid = 0;
  double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, sum = 0;
  bool done = false;
  void start(const teaser_ransac_params_c& p, int32_t nc, bool run) {
    max_iteration = p.max_iteration;
    limit = run ? max_iteration : 0;
    est_k = (double)max_iteration;
    confidence = p.confidence;
    ncorr = nc;
    ransac_n = p.ransac_n;
    done = limit == 0;
  }
  // The improvement at `e` if the loop reaches it; false when the loop has ended before it.
  bool take(const RsEntry& e) {
    if (e.trial >= limit) return false;
    best.count = e.count;
    best.rmse = rs_rmse(e.count, e.sum);
    best_trial = e.trial;
    sum = e.sum;
    memcpy(T, e.T, sizeof(T));
    const double k = log(1.0 - confidence) / log(1.0 - pow((double)e.count / (double)ncorr, (double)ransac_n));
    if (k < est_k) est_k = ceil(k);
    const double lim = std::max(std::min((double)max_iteration, est_k), (double)(e.trial + 1));
    limit = (int64_t)lim;
    return true;
  }
};

}  // namespace thip

namespace {

const Knob<teaser_hip_ransac> kKnobs[] = {{"chunk_trials", 64, 65536, &teaser_hip_ransac::chunk_trials}};

void params_default(teaser_ransac_params_c* p) {
  memset(p, 0, sizeof(*p));
  p->ransac_n = 3;
  p->max_iteration = 100000;
  p->confidence = 0.999;
}

struct Prep {  // what the entry checks and the upload leave for the loop
  std::vector<RsDesc> desc;
  int64_t total_corr = 0;
  int max_corr = 0;
  const RsDesc* d_desc = nullptr;
  const double* d_pairs = nullptr;
};

int32_t prepare(teaser_hip_ransac* h, int32_t batch, const double* const* src, const int32_t* n_src,
                const double* const* dst, const int32_t* n_dst, const int32_t* const* corr, const int32_t* n_corr,
                const teaser_ransac_params_c* params, Prep& p) {
  if (!n_src) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src must not be NULL");
  if (!n_dst) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_dst must not be NULL");
  if (!n_corr) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_corr must not be NULL");
  if (!params) return fail(h, TEASER_HIP_ERR_BAD_ARG, "params must not be NULL");
  uint64_t clock_seed = 0;
  p.desc.resize((size_t)batch);
  int64_t ns = 0, nt = 0;
  for (int b = 0; b < batch; ++b) {
    const teaser_ransac_params_c& q = params[b];
    if (!(std::isfinite(q.max_correspondence_distance) && q.max_correspondence_distance > 0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "max_correspondence_distance must be finite and > 0" + at(b));
    if (q.ransac_n < 3 || q.ransac_n > RS_MAX_N)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "ransac_n must be in 3 .. 8" + at(b));
    if (q.max_iteration < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "max_iteration must be >= 0" + at(b));
    if (!(q.confidence >= 0 && q.confidence <= 1))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "confidence must be in [0, 1]" + at(b));
    if (!(q.edge_length_threshold >= 0 && q.edge_length_threshold <= 1))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "edge_length_threshold must be 0 (off) or in (0, 1]" + at(b));
    if (!(std::isfinite(q.distance_threshold) && q.distance_threshold >= 0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "distance_threshold must be 0 (off) or finite and > 0" + at(b));
    if (q.with_scaling) return fail(h, TEASER_HIP_ERR_BAD_ARG, "with_scaling is not offered" + at(b));
    if (q.estimation)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "estimation: point-to-plane inside RANSAC is not offered" + at(b));
    if (q.normal_checker)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "normal_checker: the normal-angle checker is not offered" + at(b));
    if (n_src[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src must be >= 0" + at(b));
    if (n_dst[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_dst must be >= 0" + at(b));
    if (n_corr[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_corr must be >= 0" + at(b));
    if (n_src[b] > 0 && (!src || !src[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "src is NULL" + at(b));
    if (n_dst[b] > 0 && (!dst || !dst[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst is NULL" + at(b));
    if (n_corr[b] > 0 && (!corr || !corr[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "corr is NULL" + at(b));
    if (n_src[b] > 0 && !finite_points(src[b], n_src[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "src has non-finite points" + at(b));
    if (n_dst[b] > 0 && !finite_points(dst[b], n_dst[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst has non-finite points" + at(b));
    if (n_corr[b] > 0 && check_pairs(h, b, corr[b], n_corr[b], n_src[b], n_dst[b]) != TEASER_HIP_OK)
      return TEASER_HIP_ERR_BAD_ARG;  // the message is check_pairs's
    RsDesc& d = p.desc[(size_t)b];
    memset(&d, 0, sizeof(d));
    d.pair_off = d.corr_off = p.total_corr;
    d.src_off = ns;
    d.dst_off = nt;
    d.seed = call_seed(q.seed, clock_seed);
    d.r2 = q.max_correspondence_distance * q.max_correspondence_distance;
    d.s = q.edge_length_threshold;
    d.d = q.distance_threshold;
    d.ncorr = n_corr[b];
    d.ransac_n = q.ransac_n;
    d.run = n_corr[b] >= q.ransac_n ? 1 : 0;
    ns += n_src[b];
    nt += n_dst[b];
    p.total_corr += n_corr[b];
    p.max_corr = std::max(p.max_corr, (int)n_corr[b]);
  }
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  // ---- one upload: descriptors, both clouds, the pairs; then the pack launch ----
  Pack pin;
  const size_t i_desc = pin.add(sizeof(RsDesc) * batch), i_src = pin.add(sizeof(double) * 3 * (size_t)std::max<int64_t>(ns, 1)),
               i_dst = pin.add(sizeof(double) * 3 * (size_t)std::max<int64_t>(nt, 1)),
               i_corr = pin.add(sizeof(int32_t) * 2 * (size_t)std::max<int64_t>(p.total_corr, 1));
  if (!h->in.ensure(pin.bytes) || !h->pairs.ensure(sizeof(double) * 6 * (size_t)std::max<int64_t>(p.total_corr, 1)))
    return fail(h, TEASER_HIP_ERR_HIP, "hipMalloc failed (RANSAC inputs)");
  std::vector<char> stage(pin.bytes, 0);
  memcpy(stage.data() + i_desc, p.desc.data(), sizeof(RsDesc) * batch);
  pack_rows(stage.data() + i_src, batch, src, n_src, sizeof(double) * 3);
  pack_rows(stage.data() + i_dst, batch, dst, n_dst, sizeof(double) * 3);
  pack_rows(stage.data() + i_corr, batch, corr, n_corr, sizeof(int32_t) * 2);
  FCHK(h, hipMemcpyAsync(h->in.p, stage.data(), pin.bytes, hipMemcpyHostToDevice, h->stream), "hipMemcpyAsync (RANSAC inputs)");
  FCHK(h, hipStreamSynchronize(h->stream), "RANSAC upload");  // `stage` goes out of scope with this function
  void* din = h->in.p;
  p.d_desc = Pack::at<const RsDesc>(din, i_desc);
  p.d_pairs = h->pairs.as<double>();
  launch_ransac_pack(h->stream, batch, p.max_corr, p.d_desc, Pack::at<const double>(din, i_src),
                     Pack::at<const double>(din, i_dst), Pack::at<const int32_t>(din, i_corr), h->pairs.as<double>());
  FCHK(h, hipGetLastError(), "RANSAC pack launch");
  return TEASER_HIP_OK;
}

// The per-trial arrays of `slots` chunks in h->work and their control records in h->ctl.
struct Layout {
  size_t w_slot = 0, w_T = 0, w_flags = 0, w_count = 0, w_sum = 0, w_surv = 0, w_samples = 0;
  size_t c_n = 0, c_best = 0, c_nsurv = 0, c_nimp = 0, c_entries = 0, c_bytes = 0;
  int batch = 0, slots = 0;
  int64_t chunk = 0;
  bool samples = false;
  int32_t make(teaser_hip_ransac* h, int batch_, int slots_, int64_t chunk_, bool samples_) {
    batch = batch_;
    slots = slots_;
    chunk = chunk_;
    samples = samples_;
    const size_t per = (size_t)batch * (size_t)chunk;
    Pack w;
    w_T = w.add(sizeof(double) * 12 * per);
    w_flags = w.add(per);
    w_count = w.add(sizeof(int32_t) * per);
    w_sum = w.add(sizeof(double) * per);
    w_surv = w.add(sizeof(int32_t) * per);
    w_samples = w.add(samples ? sizeof(int32_t) * RS_MAX_N * per : 0);
    w_slot = w.bytes;
    Pack c;
    c_n = c.add(sizeof(int32_t) * batch * slots);
    c_best = c.add(sizeof(RsBest) * batch * (slots + 1));
    c_nsurv = c.add(sizeof(int32_t) * batch * slots);
    c_nimp = c.add(sizeof(int32_t) * batch * slots);
    c_entries = c.add(sizeof(RsEntry) * batch * slots * RS_LIST_CAP);
    c_bytes = c.bytes;
    if (!h->work.ensure(w_slot * slots) || !h->ctl.ensure(c_bytes))
      return fail(h, TEASER_HIP_ERR_HIP, "hipMalloc failed (RANSAC work buffers)");
    return TEASER_HIP_OK;
  }
  RsSlot slot(teaser_hip_ransac* h, int g) const {
    void* w = h->work.as<char>() + w_slot * g;
    void* c = h->ctl.p;
    RsSlot s;
    s.T = Pack::at<double>(w, w_T);
    s.flags = Pack::at<uint8_t>(w, w_flags);
    s.count = Pack::at<int32_t>(w, w_count);
    s.sum = Pack::at<double>(w, w_sum);
    s.surv = Pack::at<int32_t>(w, w_surv);
    s.samples = samples ? Pack::at<int32_t>(w, w_samples) : nullptr;
    s.n = Pack::at<const int32_t>(c, c_n) + (size_t)batch * g;
    s.best_in = Pack::at<const RsBest>(c, c_best) + (size_t)batch * g;
    s.best_out = Pack::at<RsBest>(c, c_best) + (size_t)batch * (g + 1);
    s.nsurv = Pack::at<int32_t>(c, c_nsurv) + (size_t)batch * g;
    s.n_imp = Pack::at<int32_t>(c, c_nimp) + (size_t)batch * g;
    s.entries = Pack::at<RsEntry>(c, c_entries) + (size_t)batch * g * RS_LIST_CAP;
    return s;
  }
};

void default_result(teaser_ransac_result_c* r) {
  memset(r, 0, sizeof(*r));
  r->transformation[0] = r->transformation[5] = r->transformation[10] = r->transformation[15] = 1.0;
  r->best_trial = -1;
}

int32_t run_full(teaser_hip_ransac* h, int32_t batch, const double* const* src, const int32_t* n_src,
                 const double* const* dst, const int32_t* n_dst, const int32_t* const* corr, const int32_t* n_corr,
                 const teaser_ransac_params_c* params, teaser_ransac_result_c* out, int32_t* const* inliers) {
  const int32_t r0 = begin_call(h, batch);
  if (r0 != TEASER_HIP_OK) return r0;
  if (batch == 0) return TEASER_HIP_OK;
  if (!out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "out must not be NULL");
  Prep p;
  const int32_t rc = prepare(h, batch, src, n_src, dst, n_dst, corr, n_corr, params, p);
  if (rc != TEASER_HIP_OK) return rc;
  hipStream_t s = h->stream;
  const int64_t chunk = h->chunk_trials;
  const int G = rs_group_chunks(chunk, batch);
  Layout L;
  const int32_t rl = L.make(h, batch, G, chunk, false);
  if (rl != TEASER_HIP_OK) return rl;
  std::vector<RsWalk> walk((size_t)batch);
  bool any = false;
  for (int b = 0; b < batch; ++b) {
    walk[(size_t)b].start(params[b], n_corr[b], p.desc[(size_t)b].run != 0);
    any = any || !walk[(size_t)b].done;
  }
  char* ctl = h->ctl.as<char>();
  const size_t up_bytes = L.c_best + sizeof(RsBest) * batch;  // the plan of every chunk and the best carried in
  std::vector<char> up(up_bytes), down(L.c_bytes - L.c_nsurv);
  std::vector<uint8_t> fl;
  for (int64_t first0 = 0; any; first0 += (int64_t)G * chunk) {
    // ---- plan the group ----
    memset(up.data(), 0, up_bytes);
    int32_t* plan = Pack::at<int32_t>(up.data(), L.c_n);
    RsBest* carry = Pack::at<RsBest>(up.data(), L.c_best);
    int used = 0;
    std::vector<int> max_n((size_t)G, 0);
    for (int g = 0; g < G; ++g) {
      const int64_t first = first0 + g * chunk;
      for (int b = 0; b < batch; ++b) {
        const RsWalk& w = walk[(size_t)b];
        const int64_t n = w.done ? 0 : std::max<int64_t>(0, std::min<int64_t>(chunk, w.limit - first));
        plan[(size_t)g * batch + b] = (int32_t)n;
        max_n[(size_t)g] = std::max(max_n[(size_t)g], (int)n);
      }
      if (max_n[(size_t)g] > 0) used = g + 1;
    }
    for (int b = 0; b < batch; ++b) carry[b] = walk[(size_t)b].best;
    FCHK(h, hipMemcpyAsync(ctl, up.data(), up_bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync (RANSAC plan)");
    FCHK(h, hipMemsetAsync(ctl + L.c_nsurv, 0, sizeof(int32_t) * batch * G, s), "hipMemsetAsync (RANSAC survivors)");
    for (int g = 0; g < used; ++g) {
      const RsSlot slot = L.slot(h, g);
      launch_ransac_chunk(s, batch, (int)chunk, max_n[(size_t)g], p.d_desc, p.d_pairs, slot, first0 + g * chunk);
      launch_ransac_prefix(s, batch, (int)chunk, slot, first0 + g * chunk, 0);
    }
    FCHK(h, hipGetLastError(), "RANSAC kernel launch");
    FCHK(h, hipMemcpyAsync(down.data(), ctl + L.c_nsurv, down.size(), hipMemcpyDeviceToHost, s),
         "hipMemcpyAsync (RANSAC lists)");
    FCHK(h, hipStreamSynchronize(s), "RANSAC trials");
    const int32_t* nsurv = Pack::at<const int32_t>(down.data(), 0);
    const int32_t* nimp = Pack::at<const int32_t>(down.data(), L.c_nimp - L.c_nsurv);
    const RsEntry* entries = Pack::at<const RsEntry>(down.data(), L.c_entries - L.c_nsurv);
    // ---- walk the lists ----
    any = false;
    for (int b = 0; b < batch; ++b) {
      RsWalk& w = walk[(size_t)b];
      for (int g = 0; g < used && !w.done; ++g) {
        const int64_t first = first0 + g * chunk;
        const int64_t n = plan[(size_t)g * batch + b];
        const int total = nimp[(size_t)g * batch + b];
        std::vector<RsEntry> window(entries + ((size_t)g * batch + b) * RS_LIST_CAP,
                                    entries + ((size_t)g * batch + b + 1) * RS_LIST_CAP);
        int skip = 0;
        for (int q = 0; q < total; ++q) {
          if (q >= skip + RS_LIST_CAP) {  // a longer list than one launch hands over: ask for its next part
            skip += RS_LIST_CAP;
            const RsSlot slot = L.slot(h, g);
            launch_ransac_prefix(s, batch, (int)chunk, slot, first, skip);
            FCHK(h, hipGetLastError(), "RANSAC prefix launch");
            FCHK(h, hipMemcpyAsync(window.data(), slot.entries + (size_t)b * RS_LIST_CAP, sizeof(RsEntry) * RS_LIST_CAP,
                                   hipMemcpyDeviceToHost, s),
                 "hipMemcpyAsync (RANSAC list)");
            FCHK(h, hipStreamSynchronize(s), "RANSAC prefix");
          }
          if (!w.take(window[(size_t)(q - skip)])) break;
        }
        if (w.limit > first + n) {  // the loop goes on past this chunk
          w.valid += nsurv[(size_t)g * batch + b];
          continue;
        }
        const int64_t m = w.limit - first;  // it ends inside this chunk, after m of its trials
        if (m == n) {
          w.valid += nsurv[(size_t)g * batch + b];
        } else {
          fl.resize((size_t)m);
          FCHK(h, hipMemcpyAsync(fl.data(), L.slot(h, g).flags + (size_t)b * chunk, (size_t)m, hipMemcpyDeviceToHost, s),
               "hipMemcpyAsync (RANSAC flags)");
          FCHK(h, hipStreamSynchronize(s), "RANSAC flags");
          for (int64_t t = 0; t < m; ++t) w.valid += (fl[(size_t)t] & RS_FLAG_SCORED) ? 1 : 0;
        }
        w.done = true;
      }
      any = any || !w.done;
    }
  }
  // ---- results ----
  for (int b = 0; b < batch; ++b) {
    const RsWalk& w = walk[(size_t)b];
    teaser_ransac_result_c& r = out[b];
    default_result(&r);
    r.trials = w.limit;
    r.valid_trials = w.valid;
    r.best_trial = w.best_trial;
    if (w.best_trial < 0) continue;
    memcpy(r.transformation, w.T, sizeof(w.T));
    r.n_correspondences = w.best.count;
    r.fitness = (double)w.best.count / (double)n_corr[b];
    r.inlier_rmse = w.best.rmse;
    if (inliers && inliers[b]) {  // the winner's inliers, by the score's own expression
      int32_t k = 0;
      for (int c = 0; c < n_corr[b]; ++c) {
        const int32_t i = corr[b][2 * c], j = corr[b][2 * c + 1];
        const double rec[6] = {src[b][3 * i], src[b][3 * i + 1], src[b][3 * i + 2],
                               dst[b][3 * j], dst[b][3 * j + 1], dst[b][3 * j + 2]};
        if (rs_pair_d2(w.T, rec) < p.desc[(size_t)b].r2) {
          inliers[b][2 * k] = i;
          inliers[b][2 * k + 1] = j;
          ++k;
        }
      }
      if (k != w.best.count) return fail(h, TEASER_HIP_ERR_HIP, "RANSAC: the host's inlier count differs from the device's" + at(b));
    }
  }
  return TEASER_HIP_OK;
}

int32_t run_trials(teaser_hip_ransac* h, int32_t batch, const double* const* src, const int32_t* n_src,
                   const double* const* dst, const int32_t* n_dst, const int32_t* const* corr, const int32_t* n_corr,
                   const teaser_ransac_params_c* params, int64_t first, int32_t n, int32_t* samples, uint8_t* flags,
                   double* T, int32_t* count, double* sum) {
  const int32_t r0 = begin_call(h, batch);
  if (r0 != TEASER_HIP_OK) return r0;
  if (first < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "first must be >= 0");
  if (n < 0 || n > 65536) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must be in 0 .. 65536");
  if (batch == 0) return TEASER_HIP_OK;
  Prep p;
  const int32_t rc = prepare(h, batch, src, n_src, dst, n_dst, corr, n_corr, params, p);
  if (rc != TEASER_HIP_OK) return rc;
  if (n == 0) return TEASER_HIP_OK;
  hipStream_t s = h->stream;
  Layout L;
  const int32_t rl = L.make(h, batch, 1, n, true);
  if (rl != TEASER_HIP_OK) return rl;
  char* ctl = h->ctl.as<char>();
  std::vector<int32_t> plan((size_t)batch, n);
  FCHK(h, hipMemcpyAsync(ctl + L.c_n, plan.data(), sizeof(int32_t) * batch, hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (RANSAC plan)");
  FCHK(h, hipMemsetAsync(ctl + L.c_nsurv, 0, sizeof(int32_t) * batch, s), "hipMemsetAsync (RANSAC survivors)");
  const RsSlot slot = L.slot(h, 0);
  launch_ransac_chunk(s, batch, n, n, p.d_desc, p.d_pairs, slot, first);
  FCHK(h, hipGetLastError(), "RANSAC kernel launch");
  const size_t per = (size_t)batch * (size_t)n;
  std::vector<double> T12(T ? 12 * per : 0);
  if (T) FCHK(h, hipMemcpyAsync(T12.data(), slot.T, sizeof(double) * 12 * per, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (T)");
  if (flags) FCHK(h, hipMemcpyAsync(flags, slot.flags, per, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (flags)");
  if (count) FCHK(h, hipMemcpyAsync(count, slot.count, sizeof(int32_t) * per, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (count)");
  if (sum) FCHK(h, hipMemcpyAsync(sum, slot.sum, sizeof(double) * per, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (sum_d2)");
  if (samples)
    FCHK(h, hipMemcpyAsync(samples, slot.samples, sizeof(int32_t) * RS_MAX_N * per, hipMemcpyDeviceToHost, s),
         "hipMemcpyAsync (samples)");
  FCHK(h, hipStreamSynchronize(s), "RANSAC trials");
  for (size_t q = 0; T && q < per; ++q) {
    memcpy(T + 16 * q, T12.data() + 12 * q, sizeof(double) * 12);
    T[16 * q + 12] = T[16 * q + 13] = T[16 * q + 14] = 0.0;
    T[16 * q + 15] = 1.0;
  }
  return TEASER_HIP_OK;
}

}  // namespace

extern "C" {

int32_t teaser_hip_ransac_create(int32_t device, teaser_hip_ransac** out) { return open_handle(device, out); }
int32_t teaser_hip_ransac_destroy(teaser_hip_ransac* h) { return close_handle(h); }
const char* teaser_hip_ransac_last_error(const teaser_hip_ransac* h) { return h ? h->err.c_str() : ""; }

int32_t teaser_hip_ransac_fill_scratch(teaser_hip_ransac* h, int32_t byte, int64_t* bytes_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  const ScratchSpan spans[] = {span_of(h->in), span_of(h->pairs), span_of(h->work), span_of(h->ctl)};
  return fill_scratch(h, byte, spans, 4, bytes_out);
}

int32_t teaser_hip_ransac_params_default(teaser_ransac_params_c* params) {
  if (!params) return TEASER_HIP_ERR_BAD_ARG;
  params_default(params);
  return TEASER_HIP_OK;
}

int32_t teaser_hip_ransac_correspondence_batch(teaser_hip_ransac* h, int32_t batch, const double* const* src,
                                               const int32_t* n_src, const double* const* dst, const int32_t* n_dst,
                                               const int32_t* const* corr, const int32_t* n_corr,
                                               const teaser_ransac_params_c* params, teaser_ransac_result_c* out,
                                               int32_t* const* inliers) {
  return run_full(h, batch, src, n_src, dst, n_dst, corr, n_corr, params, out, inliers);
}

int32_t teaser_hip_ransac_correspondence(teaser_hip_ransac* h, const double* src, int32_t n_src, const double* dst,
                                         int32_t n_dst, const int32_t* corr, int32_t n_corr,
                                         const teaser_ransac_params_c* params, teaser_ransac_result_c* out,
                                         int32_t* inliers) {
  return run_full(h, 1, &src, &n_src, &dst, &n_dst, &corr, &n_corr, params, out, inliers ? &inliers : nullptr);
}

int32_t teaser_hip_ransac_set_option(teaser_hip_ransac* h, const char* name, int64_t value) {
  return set_knob(h, kKnobs, name, value);
}
int32_t teaser_hip_ransac_get_option(const teaser_hip_ransac* h, const char* name, int64_t* value) {
  return get_knob(h, kKnobs, name, value);
}

int32_t teaser_hip_ransac_trials_batch(teaser_hip_ransac* h, int32_t batch, const double* const* src,
                                       const int32_t* n_src, const double* const* dst, const int32_t* n_dst,
                                       const int32_t* const* corr, const int32_t* n_corr,
                                       const teaser_ransac_params_c* params, int64_t first, int32_t n, int32_t* samples,
                                       uint8_t* flags, double* transformations, int32_t* count, double* sum_d2) {
  return run_trials(h, batch, src, n_src, dst, n_dst, corr, n_corr, params, first, n, samples, flags, transformations,
                    count, sum_d2);
}

}  // extern "C"
