// plane.hip -- host side of RANSAC plane segmentation (include/teaser_hip.h, "Plane segmentation"): the handle, the
// entry checks, ONE upload of the clouds, then the loop.  The trials of a problem are cut into chunks of chunk_trials and
// its points into waves of W groups, W from the partial-array budget; a ROUND of chunks (1, then 2, then 4) is enqueued
// before the host looks, with one small upload (the plan) and one download per chunk (flag, count and E of every
// trial: 13 bytes each).  The host walks those records with sqrt, log and pow exactly as the contract's loop does; what
// lies past a problem's stopping trial is dropped unread.  The finish recomputes the winner's plane from (seed, trial).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "packed_call.h"
#include "plane_device.h"
#include "teaser_hip.h"

using namespace thip;

struct teaser_hip_plane : HandleBase {
  DevBuf in, work, part, fin;
  HostBuf stage;  // page-locked: the upload is one DMA copy at bus speed
  int64_t chunk_trials = 256;
  int64_t partial_bytes = 64ll << 20;
};

namespace thip {

constexpr int PL_MAX_ROUND = 4;  // chunks enqueued before the host looks, at the most
constexpr int64_t PL_MIN_CHUNK = 64, PL_MAX_CHUNK = 4096;
constexpr int64_t PL_MIN_PARTIAL = 1 << 16, PL_MAX_PARTIAL = 1ll << 34;
constexpr int64_t PL_GROUP_BYTES = (PL_GROUP + 1) * 12;  // per trial of the chunk: 64 block records and the group's

// The groups of points one wave covers: the largest halving of the longest problem's groups whose partials, over the
// whole batch, stay within the budget; one group per problem at the least.
inline int pl_wave_groups(const std::vector<PlDesc>& desc, int64_t chunk, int64_t budget) {
  int64_t W = 1;
  for (const PlDesc& d : desc) W = std::max(W, pl_groups(d.n));
  const int64_t fit = budget / (chunk * PL_GROUP_BYTES);
  for (; W > 1; W = (W + 1) / 2) {
    int64_t total = 0;
    for (const PlDesc& d : desc) total += std::min(W, pl_groups(d.n));
    if (total <= fit) break;
  }
  return (int)W;
}

// The contract's loop over the records of one problem, trial by trial.
struct PlWalk {
  int64_t num_iterations = 0, trials = 0, counted = 0, best_trial = -1;
  double k = std::numeric_limits<double>::infinity(), probability = 0, best_rmse = 0;
  int32_t n = 0, ransac_n = 0, best_count = 0;
  bool done = false;
  void start(const teaser_plane_params_c& p, int32_t n_, bool run) {
    num_iterations = p.num_iterations;
    probability = p.probability;
    ransac_n = p.ransac_n;
    n = n_;
    done = !run || num_iterations == 0;
  }
  // Trial `trial` with its record; false when the loop has stopped before it.
  bool visit(int64_t trial, uint8_t flag, int32_t count, double E) {
    if ((double)counted > k) {
      done = true;
      return false;
    }
    trials = trial + 1;
    if (trials == num_iterations) done = true;
    if (!(flag & PL_FLAG_VALID)) return true;
    const double rmse = pl_rmse(count, E);
    if (count > best_count || (count == best_count && rmse < best_rmse)) {
      best_count = count;
      best_rmse = rmse;
      best_trial = trial;
      if (count == n) {
        k = 0.0;
      } else {
        const double fitness = (double)count / (double)n;
        const double q = log(1.0 - probability) / log(1.0 - pow(fitness, (double)ransac_n));
        const double cap = (double)num_iterations;
        k = q < cap ? q : cap;
      }
    }
    ++counted;
    return true;
  }
};

}  // namespace thip

namespace {

const Knob<teaser_hip_plane> kKnobs[] = {{"chunk_trials", PL_MIN_CHUNK, PL_MAX_CHUNK, &teaser_hip_plane::chunk_trials},
                                         {"partial_bytes", PL_MIN_PARTIAL, PL_MAX_PARTIAL, &teaser_hip_plane::partial_bytes}};

void params_default(teaser_plane_params_c* p) {
  memset(p, 0, sizeof(*p));
  p->ransac_n = 3;
  p->num_iterations = 100;
  p->probability = 0.99999999;
}

struct Prep {  // what the entry checks and the upload leave for the loop
  std::vector<PlDesc> desc;
  int64_t total_points = 0, total_blocks = 0, total_groups = 0, part_groups = 0;
  int max_points = 0, W = 1;
  const PlDesc* d_desc = nullptr;
  const double* d_pts = nullptr;
};

int32_t prepare(teaser_hip_plane* h, int32_t batch, const double* const* points, const int32_t* n,
                const teaser_plane_params_c* params, Prep& p) {
  if (!n) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must not be NULL");
  if (!params) return fail(h, TEASER_HIP_ERR_BAD_ARG, "params must not be NULL");
  uint64_t clock_seed = 0;
  p.desc.resize((size_t)batch);
  for (int b = 0; b < batch; ++b) {
    const teaser_plane_params_c& q = params[b];
    if (!(std::isfinite(q.distance_threshold) && q.distance_threshold > 0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "distance_threshold must be finite and > 0" + at(b));
    if (q.ransac_n < 3 || q.ransac_n > PL_MAX_N)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "ransac_n must be in 3 .. 8" + at(b));
    if (q.num_iterations < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "num_iterations must be >= 0" + at(b));
    if (!(q.probability > 0 && q.probability <= 1))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "probability must be in (0, 1]" + at(b));
    if (n[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must be >= 0" + at(b));
    if (n[b] > 0 && (!points || !points[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "points is NULL" + at(b));
    if (n[b] > 0 && !finite_points(points[b], n[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "points has non-finite points" + at(b));
    PlDesc& d = p.desc[(size_t)b];
    memset(&d, 0, sizeof(d));
    d.pt_off = p.total_points;
    d.blk_off = p.total_blocks;
    d.grp_off = p.total_groups;
    d.seed = call_seed(q.seed, clock_seed);
    d.d = q.distance_threshold;
    d.n = n[b];
    d.ransac_n = q.ransac_n;
    d.run = n[b] >= q.ransac_n ? 1 : 0;
    p.total_points += n[b];
    p.total_blocks += pl_blocks(n[b]);
    p.total_groups += pl_groups(n[b]);
    p.max_points = std::max(p.max_points, (int)n[b]);
  }
  p.W = pl_wave_groups(p.desc, h->chunk_trials, h->partial_bytes);
  for (int b = 0; b < batch; ++b) {
    p.desc[(size_t)b].part_grp = p.part_groups;
    p.part_groups += std::min<int64_t>(p.W, pl_groups(n[b]));
  }
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  // ---- one upload: descriptors and clouds ----
  Pack pin;
  const size_t i_desc = pin.add(sizeof(PlDesc) * batch),
               i_pts = pin.add(sizeof(double) * 3 * (size_t)std::max<int64_t>(p.total_points, 1));
  if (!h->in.ensure(pin.bytes) || !h->stage.ensure(pin.bytes))
    return fail(h, TEASER_HIP_ERR_HIP, "hipMalloc failed (plane inputs)");
  char* stage = h->stage.as<char>();
  memcpy(stage + i_desc, p.desc.data(), sizeof(PlDesc) * batch);
  pack_rows(stage + i_pts, batch, points, n, sizeof(double) * 3);
  FCHK(h, hipMemcpyAsync(h->in.p, stage, pin.bytes, hipMemcpyHostToDevice, h->stream), "hipMemcpyAsync (plane inputs)");
  FCHK(h, hipStreamSynchronize(h->stream), "plane upload");  // the staging buffer is free for the next call
  p.d_desc = Pack::at<const PlDesc>(h->in.p, i_desc);
  p.d_pts = Pack::at<const double>(h->in.p, i_pts);
  return TEASER_HIP_OK;
}

// The per-trial arrays of `slots` chunks in h->work (each slot: plan, E, count, flags -- what the host reads -- then the
// models and the samples) and the partials of one point wave in h->part.
struct Layout {
  size_t w_n = 0, w_E = 0, w_count = 0, w_flags = 0, w_read = 0, w_model = 0, w_samples = 0, w_slot = 0;
  size_t p_bcnt = 0, p_bsum = 0, p_gcnt = 0, p_gsum = 0;
  int batch = 0, slots = 0;
  int64_t chunk = 0;
  bool samples = false;
  int32_t make(teaser_hip_plane* h, const Prep& p, int batch_, int slots_, int64_t chunk_, bool samples_) {
    batch = batch_;
    slots = slots_;
    chunk = chunk_;
    samples = samples_;
    const size_t per = (size_t)batch * (size_t)chunk;
    Pack w;
    w_n = w.add(sizeof(int32_t) * batch);
    w_E = w.add(sizeof(double) * per);
    w_count = w.add(sizeof(int32_t) * per);
    w_flags = w.add(per);
    w_read = w.bytes;
    w_model = w.add(sizeof(double) * 4 * per);
    w_samples = w.add(samples ? sizeof(int32_t) * PL_MAX_N * per : 0);
    w_slot = w.bytes;
    const size_t groups = (size_t)std::max<int64_t>(p.part_groups, 1);
    Pack q;
    p_bcnt = q.add(sizeof(int32_t) * groups * PL_GROUP * (size_t)chunk);
    p_bsum = q.add(sizeof(double) * groups * PL_GROUP * (size_t)chunk);
    p_gcnt = q.add(sizeof(int32_t) * groups * (size_t)chunk);
    p_gsum = q.add(sizeof(double) * groups * (size_t)chunk);
    if (!h->work.ensure(w_slot * slots) || !h->part.ensure(q.bytes))
      return fail(h, TEASER_HIP_ERR_HIP, "hipMalloc failed (plane work buffers)");
    return TEASER_HIP_OK;
  }
  char* base(teaser_hip_plane* h, int g) const { return h->work.as<char>() + w_slot * g; }
  PlSlot slot(teaser_hip_plane* h, int g) const {
    void* w = base(h, g);
    PlSlot s;
    s.n = Pack::at<const int32_t>(w, w_n);
    s.E = Pack::at<double>(w, w_E);
    s.count = Pack::at<int32_t>(w, w_count);
    s.flags = Pack::at<uint8_t>(w, w_flags);
    s.model = Pack::at<double>(w, w_model);
    s.samples = samples ? Pack::at<int32_t>(w, w_samples) : nullptr;
    return s;
  }
  PlPart partials(teaser_hip_plane* h) const {
    void* q = h->part.p;
    PlPart s;
    s.bcnt = Pack::at<int32_t>(q, p_bcnt);
    s.bsum = Pack::at<double>(q, p_bsum);
    s.gcnt = Pack::at<int32_t>(q, p_gcnt);
    s.gsum = Pack::at<double>(q, p_gsum);
    return s;
  }
};

// Models, then the score of every point wave, for one chunk.
void enqueue_chunk(teaser_hip_plane* h, const Prep& p, const Layout& L, int batch, int g, int max_n, int64_t first) {
  const PlSlot slot = L.slot(h, g);
  launch_plane_models(h->stream, batch, (int)L.chunk, max_n, p.d_desc, p.d_pts, slot, first);
  const int ng = (int)pl_groups(p.max_points);
  for (int g0 = 0; g0 < ng; g0 += p.W)
    launch_plane_score(h->stream, batch, (int)L.chunk, max_n, p.d_desc, p.d_pts, slot, L.partials(h), g0, p.W);
}

void default_result(teaser_plane_result_c* r) {
  memset(r, 0, sizeof(*r));
  r->best_trial = -1;
}

int32_t run_full(teaser_hip_plane* h, int32_t batch, const double* const* points, const int32_t* n,
                 const teaser_plane_params_c* params, teaser_plane_result_c* out, int32_t* const* inliers,
                 uint8_t* const* mask) {
  const int32_t r0 = begin_call(h, batch);
  if (r0 != TEASER_HIP_OK) return r0;
  if (batch == 0) return TEASER_HIP_OK;
  if (!out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "out must not be NULL");
  Prep p;
  const int32_t rc = prepare(h, batch, points, n, params, p);
  if (rc != TEASER_HIP_OK) return rc;
  hipStream_t s = h->stream;
  const int64_t chunk = h->chunk_trials;
  Layout L;
  const int32_t rl = L.make(h, p, batch, PL_MAX_ROUND, chunk, false);
  if (rl != TEASER_HIP_OK) return rl;
  std::vector<PlWalk> walk((size_t)batch);
  bool any = false;
  for (int b = 0; b < batch; ++b) {
    walk[(size_t)b].start(params[b], n[b], p.desc[(size_t)b].run != 0);
    any = any || !walk[(size_t)b].done;
  }
  std::vector<int32_t> plan((size_t)PL_MAX_ROUND * batch);
  std::vector<char> down(L.w_read * PL_MAX_ROUND);
  int G = 1;
  for (int64_t first0 = 0; any; first0 += (int64_t)G * chunk, G = std::min(PL_MAX_ROUND, 2 * G)) {
    // ---- plan and enqueue the round ----
    int used = 0;
    for (int g = 0; g < G; ++g) {
      const int64_t first = first0 + g * chunk;
      int max_n = 0;
      for (int b = 0; b < batch; ++b) {
        const PlWalk& w = walk[(size_t)b];
        const int64_t m = w.done ? 0 : std::max<int64_t>(0, std::min<int64_t>(chunk, w.num_iterations - first));
        plan[(size_t)g * batch + b] = (int32_t)m;
        max_n = std::max(max_n, (int)m);
      }
      if (max_n == 0) break;
      used = g + 1;
      FCHK(h, hipMemcpyAsync(L.base(h, g) + L.w_n, plan.data() + (size_t)g * batch, sizeof(int32_t) * batch,
                             hipMemcpyHostToDevice, s),
           "hipMemcpyAsync (plane plan)");
      enqueue_chunk(h, p, L, batch, g, max_n, first);
      FCHK(h, hipGetLastError(), "plane kernel launch");
      FCHK(h, hipMemcpyAsync(down.data() + L.w_read * g, L.base(h, g), L.w_read, hipMemcpyDeviceToHost, s),
           "hipMemcpyAsync (plane records)");
    }
    FCHK(h, hipStreamSynchronize(s), "plane trials");
    // ---- walk the records ----
    any = false;
    for (int b = 0; b < batch; ++b) {
      PlWalk& w = walk[(size_t)b];
      for (int g = 0; g < used && !w.done; ++g) {
        const char* rec = down.data() + L.w_read * g;
        const double* E = Pack::at<const double>(rec, L.w_E) + (size_t)b * chunk;
        const int32_t* count = Pack::at<const int32_t>(rec, L.w_count) + (size_t)b * chunk;
        const uint8_t* flags = Pack::at<const uint8_t>(rec, L.w_flags) + (size_t)b * chunk;
        const int64_t first = first0 + g * chunk;
        const int m = plan[(size_t)g * batch + b];
        for (int t = 0; t < m && !w.done; ++t)
          if (!w.visit(first + t, flags[t], count[t], E[t])) break;
      }
      any = any || !w.done;
    }
  }
  // ---- finish: the mask under the winner, the refit ----
  Pack f;
  const size_t f_best = f.add(sizeof(int64_t) * batch), f_win = f.add(sizeof(double) * 4 * batch),
               f_cen = f.add(sizeof(double) * 3 * batch), f_out = f.add(sizeof(double) * 4 * batch),
               f_m = f.add(sizeof(int32_t) * batch), f_mask = f.add((size_t)std::max<int64_t>(p.total_points, 1)),
               f_bsum = f.add(sizeof(double) * 6 * (size_t)std::max<int64_t>(p.total_blocks, 1)),
               f_bcnt = f.add(sizeof(int32_t) * (size_t)std::max<int64_t>(p.total_blocks, 1)),
               f_gsum = f.add(sizeof(double) * 6 * (size_t)std::max<int64_t>(p.total_groups, 1)),
               f_gcnt = f.add(sizeof(int32_t) * (size_t)std::max<int64_t>(p.total_groups, 1));
  if (!h->fin.ensure(f.bytes)) return fail(h, TEASER_HIP_ERR_HIP, "hipMalloc failed (plane finish buffers)");
  char* df = h->fin.as<char>();
  PlFin fin;
  fin.best = Pack::at<const int64_t>(df, f_best);
  fin.win = Pack::at<double>(df, f_win);
  fin.centroid = Pack::at<double>(df, f_cen);
  fin.plane = Pack::at<double>(df, f_out);
  fin.m = Pack::at<int32_t>(df, f_m);
  fin.mask = Pack::at<uint8_t>(df, f_mask);
  fin.bsum = Pack::at<double>(df, f_bsum);
  fin.bcnt = Pack::at<int32_t>(df, f_bcnt);
  fin.gsum = Pack::at<double>(df, f_gsum);
  fin.gcnt = Pack::at<int32_t>(df, f_gcnt);
  std::vector<int64_t> best((size_t)batch);
  for (int b = 0; b < batch; ++b) best[(size_t)b] = walk[(size_t)b].best_trial;
  FCHK(h, hipMemcpyAsync(df + f_best, best.data(), sizeof(int64_t) * batch, hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (plane winners)");
  launch_plane_finish(s, batch, p.max_points, p.d_desc, p.d_pts, fin);
  FCHK(h, hipGetLastError(), "plane finish launch");
  std::vector<double> planes((size_t)4 * batch);
  std::vector<int32_t> m((size_t)batch);
  bool want_mask = false;
  for (int b = 0; b < batch; ++b) want_mask = want_mask || (inliers && inliers[b]) || (mask && mask[b]);
  std::vector<uint8_t> hmask(want_mask ? (size_t)p.total_points : 0);
  FCHK(h, hipMemcpyAsync(planes.data(), fin.plane, sizeof(double) * 4 * batch, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (planes)");
  FCHK(h, hipMemcpyAsync(m.data(), fin.m, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (plane counts)");
  if (!hmask.empty())
    FCHK(h, hipMemcpyAsync(hmask.data(), fin.mask, hmask.size(), hipMemcpyDeviceToHost, s), "hipMemcpyAsync (plane mask)");
  FCHK(h, hipStreamSynchronize(s), "plane finish");
  for (int b = 0; b < batch; ++b) {
    const PlWalk& w = walk[(size_t)b];
    teaser_plane_result_c& r = out[b];
    default_result(&r);
    r.trials = w.trials;
    r.valid_trials = w.counted;
    r.best_trial = w.best_trial;
    if (mask && mask[b] && n[b] > 0) memcpy(mask[b], hmask.data() + p.desc[(size_t)b].pt_off, (size_t)n[b]);
    if (w.best_trial < 0) continue;
    if (m[(size_t)b] != w.best_count)
      return fail(h, TEASER_HIP_ERR_HIP, "plane: the finish's inlier count differs from the score's" + at(b));
    memcpy(r.plane, planes.data() + 4 * (size_t)b, sizeof(double) * 4);
    r.n_inliers = w.best_count;
    r.fitness = (double)w.best_count / (double)n[b];
    r.inlier_rmse = w.best_rmse;
    if (inliers && inliers[b]) {  // ascending, from the mask
      const uint8_t* mk = hmask.data() + p.desc[(size_t)b].pt_off;
      int32_t k = 0;
      for (int32_t i = 0; i < n[b]; ++i)
        if (mk[i]) inliers[b][k++] = i;
    }
  }
  return TEASER_HIP_OK;
}

int32_t run_trials(teaser_hip_plane* h, int32_t batch, const double* const* points, const int32_t* n,
                   const teaser_plane_params_c* params, int64_t first, int32_t cnt, int32_t* samples, uint8_t* flags,
                   double* planes, int32_t* count, double* E) {
  const int32_t r0 = begin_call(h, batch);
  if (r0 != TEASER_HIP_OK) return r0;
  if (first < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "first must be >= 0");
  if (cnt < 0 || cnt > 65536) return fail(h, TEASER_HIP_ERR_BAD_ARG, "cnt must be in 0 .. 65536");
  if (batch == 0) return TEASER_HIP_OK;
  Prep p;
  const int32_t rc = prepare(h, batch, points, n, params, p);
  if (rc != TEASER_HIP_OK) return rc;
  if (cnt == 0) return TEASER_HIP_OK;
  hipStream_t s = h->stream;
  const int64_t chunk = h->chunk_trials;
  Layout L;
  const int32_t rl = L.make(h, p, batch, 1, chunk, true);
  if (rl != TEASER_HIP_OK) return rl;
  const PlSlot slot = L.slot(h, 0);
  std::vector<int32_t> plan((size_t)batch);
  for (int64_t c0 = 0; c0 < cnt; c0 += chunk) {  // the chunks of the full call, one at a time
    const int m = (int)std::min<int64_t>(chunk, cnt - c0);
    std::fill(plan.begin(), plan.end(), m);
    FCHK(h, hipMemcpyAsync(L.base(h, 0) + L.w_n, plan.data(), sizeof(int32_t) * batch, hipMemcpyHostToDevice, s),
         "hipMemcpyAsync (plane plan)");
    enqueue_chunk(h, p, L, batch, 0, m, first + c0);
    FCHK(h, hipGetLastError(), "plane kernel launch");
    for (int b = 0; b < batch; ++b) {
      const size_t from = (size_t)b * chunk, to = (size_t)b * cnt + (size_t)c0;
      if (samples)
        FCHK(h, hipMemcpyAsync(samples + PL_MAX_N * to, slot.samples + PL_MAX_N * from, sizeof(int32_t) * PL_MAX_N * m,
                               hipMemcpyDeviceToHost, s), "hipMemcpyAsync (samples)");
      if (flags) FCHK(h, hipMemcpyAsync(flags + to, slot.flags + from, (size_t)m, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (flags)");
      if (planes)
        FCHK(h, hipMemcpyAsync(planes + 4 * to, slot.model + 4 * from, sizeof(double) * 4 * m, hipMemcpyDeviceToHost, s),
             "hipMemcpyAsync (planes)");
      if (count) FCHK(h, hipMemcpyAsync(count + to, slot.count + from, sizeof(int32_t) * m, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (count)");
      if (E) FCHK(h, hipMemcpyAsync(E + to, slot.E + from, sizeof(double) * m, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (E)");
    }
    FCHK(h, hipStreamSynchronize(s), "plane trials");
  }
  return TEASER_HIP_OK;
}

}  // namespace

extern "C" {

int32_t teaser_hip_plane_create(int32_t device, teaser_hip_plane** out) { return open_handle(device, out); }
int32_t teaser_hip_plane_destroy(teaser_hip_plane* h) { return close_handle(h); }
const char* teaser_hip_plane_last_error(const teaser_hip_plane* h) { return h ? h->err.c_str() : ""; }

int32_t teaser_hip_plane_fill_scratch(teaser_hip_plane* h, int32_t byte, int64_t* bytes_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  const ScratchSpan spans[] = {span_of(h->in), span_of(h->work), span_of(h->part), span_of(h->fin), span_of(h->stage)};
  return fill_scratch(h, byte, spans, 5, bytes_out);
}

int32_t teaser_hip_plane_params_default(teaser_plane_params_c* params) {
  if (!params) return TEASER_HIP_ERR_BAD_ARG;
  params_default(params);
  return TEASER_HIP_OK;
}

int32_t teaser_hip_plane_segment_batch(teaser_hip_plane* h, int32_t batch, const double* const* points, const int32_t* n,
                                       const teaser_plane_params_c* params, teaser_plane_result_c* out,
                                       int32_t* const* inliers, uint8_t* const* mask) {
  return run_full(h, batch, points, n, params, out, inliers, mask);
}

int32_t teaser_hip_plane_segment(teaser_hip_plane* h, const double* points, int32_t n,
                                 const teaser_plane_params_c* params, teaser_plane_result_c* out, int32_t* inliers,
                                 uint8_t* mask) {
  return run_full(h, 1, &points, &n, params, out, inliers ? &inliers : nullptr, mask ? &mask : nullptr);
}

int32_t teaser_hip_plane_set_option(teaser_hip_plane* h, const char* name, int64_t value) {
  return set_knob(h, kKnobs, name, value);
}
int32_t teaser_hip_plane_get_option(const teaser_hip_plane* h, const char* name, int64_t* value) {
  return get_knob(h, kKnobs, name, value);
}

int32_t teaser_hip_plane_trials_batch(teaser_hip_plane* h, int32_t batch, const double* const* points, const int32_t* n,
                                      const teaser_plane_params_c* params, int64_t first, int32_t cnt, int32_t* samples,
                                      uint8_t* flags, double* planes, int32_t* count, double* E) {
  return run_trials(h, batch, points, n, params, first, cnt, samples, flags, planes, count, E);
}

}  // extern "C"
