// posegraph.hip -- host side of pose-graph optimisation (include/teaser_hip.h, "Pose-graph optimisation"): the handle,
// the entry checks, the per-graph index the kernel assembles from (a CSR of incident edges per node and the sorted
// list of distinct node pairs with their edges, both ascending in edge index), ONE upload of everything packed, ONE
// launch of kernels_posegraph.hip (a workgroup per graph), ONE download and one synchronisation.  The caller's
// arrays are written only after the synchronisation, so a refusal or a HIP error leaves them untouched.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "packed_call.h"
#include "posegraph_device.h"
#include "teaser_hip.h"

using namespace thip;

struct teaser_hip_posegraph : HandleBase {
  DevBuf in, work, dense, out;
};

namespace thip {

// The index of a call: descriptors, CSR and pair lists.  Built by pg_build_index; tests/posegraph_host_driver.cpp
// checks it against brute force.
struct PgIndex {
  std::vector<PgDesc> desc;
  std::vector<int32_t> node_ptr, inc_edge, pair_u, pair_v, pair_ptr, pair_edge;
  int64_t nodes = 0, edges = 0, pairs = 0, dense = 0, free_unknowns = 0, trace_rows = 0;
};

inline void pg_build_index(PgIndex& ix, int batch, const int32_t* n_nodes, const int32_t* n_edges, const int32_t* src,
                           const int32_t* tgt, const teaser_posegraph_option_c* opts, const int32_t* trace_cap,
                           int mode) {
  ix.desc.resize((size_t)batch);
  for (int b = 0; b < batch; ++b) {
    PgDesc& d = ix.desc[(size_t)b];
    memset(&d, 0, sizeof(d));
    const int n = n_nodes[b], m = n_edges[b];
    d.n = n;
    d.m = m;
    d.opt = opts[b];
    d.ref = d.opt.reference_node < 0 ? 0 : d.opt.reference_node;
    d.N = n > 1 ? 6 * (n - 1) : 0;
    d.trivial = mode == PG_MODE_OPTIMIZE ? (n <= 1 || m == 0) : n == 0;
    d.trace_cap = trace_cap ? trace_cap[b] : 0;
    d.node_off = ix.nodes;
    d.edge_off = ix.edges;
    d.nodeptr_off = ix.nodes + b;
    d.inc_off = 2 * ix.edges;
    d.pair_off = ix.pairs;
    d.pairptr_off = ix.pairs + b;
    d.h_off = ix.dense;
    d.g_off = ix.free_unknowns;
    d.trace_off = ix.trace_rows;
    const int32_t* s = src + ix.edges;
    const int32_t* t = tgt + ix.edges;
    // CSR: node -> incident edges, ascending (an edge is in its source's and in its target's row)
    std::vector<int32_t> ptr((size_t)n + 1, 0);
    for (int k = 0; k < m; ++k) {
      ++ptr[(size_t)s[k] + 1];
      ++ptr[(size_t)t[k] + 1];
    }
    for (int i = 0; i < n; ++i) ptr[(size_t)i + 1] += ptr[(size_t)i];
    std::vector<int32_t> inc((size_t)2 * m), fill(ptr.begin(), ptr.end() - 1);
    for (int k = 0; k < m; ++k) {
      inc[(size_t)fill[(size_t)s[k]]++] = k;
      inc[(size_t)fill[(size_t)t[k]]++] = k;
    }
    ix.node_ptr.insert(ix.node_ptr.end(), ptr.begin(), ptr.end());
    ix.inc_edge.insert(ix.inc_edge.end(), inc.begin(), inc.end());
    // distinct unordered pairs, sorted, with their edges ascending
    std::vector<int64_t> key((size_t)m);
    for (int k = 0; k < m; ++k) {
      const int64_t u = std::min(s[k], t[k]), v = std::max(s[k], t[k]);
      key[(size_t)k] = ((u * (int64_t)(TEASER_HIP_POSEGRAPH_MAX_NODES + 1) + v) << 20) | k;  // m <= 2^14
    }
    std::sort(key.begin(), key.end());
    int np = 0;
    ix.pair_ptr.push_back(0);
    for (int q = 0; q < m; ++q) {
      const int64_t uv = key[(size_t)q] >> 20;
      if (q == 0 || uv != (key[(size_t)q - 1] >> 20)) {
        if (q > 0) ix.pair_ptr.push_back(q);
        ix.pair_u.push_back((int32_t)(uv / (TEASER_HIP_POSEGRAPH_MAX_NODES + 1)));
        ix.pair_v.push_back((int32_t)(uv % (TEASER_HIP_POSEGRAPH_MAX_NODES + 1)));
        ++np;
      }
      ix.pair_edge.push_back((int32_t)(key[(size_t)q] & ((1 << 20) - 1)));
    }
    if (m > 0) ix.pair_ptr.push_back(m);
    d.n_pairs = np;
    ix.nodes += n;
    ix.edges += m;
    ix.pairs += np;
    ix.dense += (int64_t)d.N * d.N;
    ix.free_unknowns += d.N;
    ix.trace_rows += d.trace_cap;
  }
}

}  // namespace thip

namespace {

void option_default(teaser_posegraph_option_c* o) {
  memset(o, 0, sizeof(*o));
  o->max_iteration = 100;
  o->max_iteration_lm = 20;
  o->min_relative_increment = 1e-6;
  o->min_relative_residual_increment = 1e-6;
  o->min_right_term = 1e-6;
  o->min_residual = 1e-6;
  o->upper_scale_factor = 2.0 / 3.0;
  o->lower_scale_factor = 1.0 / 3.0;
  o->max_correspondence_distance = 0.03;
  o->edge_prune_threshold = 0.25;
  o->preference_loop_closure = 1.0;
  o->reference_node = -1;
}

struct PgOutputs {  // the caller's arrays; which ones exist depends on the entry
  double *poses_out = nullptr, *confidence = nullptr;
  uint8_t* pruned = nullptr;
  teaser_posegraph_result_c* results = nullptr;
  teaser_posegraph_trace_c* trace = nullptr;
  double *e = nullptr, *r = nullptr, *l = nullptr, *mu = nullptr, *F = nullptr, *H = nullptr, *g = nullptr;
};

int32_t run(teaser_hip_posegraph* h, int mode, int32_t batch, const int32_t* n_nodes, const double* poses,
            const int32_t* n_edges, const int32_t* src, const int32_t* tgt, const double* X, const double* L,
            const uint8_t* unc, const teaser_posegraph_option_c* options, const int32_t* trace_cap,
            const PgOutputs& o) {
  const int32_t r0 = begin_call(h, batch, false);  // a workgroup per graph along x: no grid limit
  if (r0 != TEASER_HIP_OK) return r0;
  if (batch == 0) return TEASER_HIP_OK;
  if (!n_nodes) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_nodes must not be NULL");
  if (!n_edges) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_edges must not be NULL");
  if (o.trace && !trace_cap) return fail(h, TEASER_HIP_ERR_BAD_ARG, "trace_cap must not be NULL with a trace");
  // ---- the entry checks ----
  std::vector<teaser_posegraph_option_c> opts((size_t)batch);
  int64_t nodes = 0, edges = 0;
  for (int b = 0; b < batch; ++b) {
    const int n = n_nodes[b], m = n_edges[b];
    if (n < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_nodes must be >= 0" + at(b));
    if (m < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_edges must be >= 0" + at(b));
    if (n > TEASER_HIP_POSEGRAPH_MAX_NODES)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_nodes exceeds TEASER_HIP_POSEGRAPH_MAX_NODES" + at(b));
    if (m > TEASER_HIP_POSEGRAPH_MAX_EDGES)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_edges exceeds TEASER_HIP_POSEGRAPH_MAX_EDGES" + at(b));
    if (o.trace && trace_cap[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "trace_cap must be >= 0" + at(b));
    teaser_posegraph_option_c& op = opts[(size_t)b];
    if (options)
      op = options[b];
    else
      option_default(&op);
    const double* fields[9] = {&op.min_relative_increment, &op.min_relative_residual_increment, &op.min_right_term,
                               &op.min_residual, &op.upper_scale_factor, &op.lower_scale_factor,
                               &op.max_correspondence_distance, &op.edge_prune_threshold, &op.preference_loop_closure};
    static const char* names[9] = {"min_relative_increment", "min_relative_residual_increment", "min_right_term",
                                   "min_residual", "upper_scale_factor", "lower_scale_factor",
                                   "max_correspondence_distance", "edge_prune_threshold", "preference_loop_closure"};
    for (int k = 0; k < 9; ++k)
      if (!std::isfinite(*fields[k]))
        return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string("options.") + names[k] + " is not finite" + at(b));
    if (op.max_iteration < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "options.max_iteration must be >= 0" + at(b));
    if (op.max_iteration_lm < 0)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "options.max_iteration_lm must be >= 0" + at(b));
    if (op.max_iteration > TEASER_HIP_POSEGRAPH_MAX_ITERATION)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "options.max_iteration exceeds TEASER_HIP_POSEGRAPH_MAX_ITERATION" + at(b));
    if (op.max_iteration_lm > TEASER_HIP_POSEGRAPH_MAX_ITERATION_LM)
      return fail(h, TEASER_HIP_ERR_BAD_ARG,
                  "options.max_iteration_lm exceeds TEASER_HIP_POSEGRAPH_MAX_ITERATION_LM" + at(b));
    if (op.reference_node >= 0 && op.reference_node >= n)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "options.reference_node must be < n_nodes" + at(b));
    if (n > 0 && !poses) return fail(h, TEASER_HIP_ERR_BAD_ARG, "poses is NULL" + at(b));
    if (m > 0 && (!src || !tgt)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "edge_source / edge_target is NULL" + at(b));
    if (m > 0 && !X) return fail(h, TEASER_HIP_ERR_BAD_ARG, "edge_transformation is NULL" + at(b));
    if (m > 0 && !L) return fail(h, TEASER_HIP_ERR_BAD_ARG, "edge_information is NULL" + at(b));
    if (m > 0 && !unc) return fail(h, TEASER_HIP_ERR_BAD_ARG, "edge_uncertain is NULL" + at(b));
    if (n > 0 && mode == PG_MODE_OPTIMIZE && !o.poses_out)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "poses_out is NULL" + at(b));
    for (int i = 0; i < n; ++i) {
      const double* T = poses + 16 * (nodes + i);
      if (!finite_all(T, 16))
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "poses: node " + std::to_string(i) + " is not finite" + at(b));
      if (T[12] != 0 || T[13] != 0 || T[14] != 0 || T[15] != 1)
        return fail(h, TEASER_HIP_ERR_BAD_ARG,
                    "poses: last row of node " + std::to_string(i) + " must be 0 0 0 1" + at(b));
    }
    for (int k = 0; k < m; ++k) {
      const int64_t K = edges + k;
      const std::string ek = "edge " + std::to_string(k);
      if (src[K] < 0 || src[K] >= n)
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "edge_source: " + ek + " is out of range" + at(b));
      if (tgt[K] < 0 || tgt[K] >= n)
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "edge_target: " + ek + " is out of range" + at(b));
      if (src[K] == tgt[K])
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "edge_source == edge_target at " + ek + at(b));
      if (!finite_all(X + 16 * K, 16))
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "edge_transformation: " + ek + " is not finite" + at(b));
      const double* T = X + 16 * K;
      if (T[12] != 0 || T[13] != 0 || T[14] != 0 || T[15] != 1)
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "edge_transformation: last row of " + ek + " must be 0 0 0 1" + at(b));
      for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j)
          if (!std::isfinite(L[36 * K + 6 * i + j]))
            return fail(h, TEASER_HIP_ERR_BAD_ARG, "edge_information: " + ek + " is not finite" + at(b));
    }
    nodes += n;
    edges += m;
  }
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");

  // ---- index and packing ----
  PgIndex ix;
  pg_build_index(ix, batch, n_nodes, n_edges, src, tgt, opts.data(), o.trace ? trace_cap : nullptr, mode);
  Pack pin, pwork, pout;
  const size_t N1 = (size_t)std::max<int64_t>(nodes, 1), M1 = (size_t)std::max<int64_t>(edges, 1);
  const size_t i_desc = pin.add(sizeof(PgDesc) * batch), i_poses = pin.add(sizeof(double) * 16 * N1),
               i_src = pin.add(4 * M1), i_tgt = pin.add(4 * M1), i_X = pin.add(sizeof(double) * 16 * M1),
               i_L = pin.add(sizeof(double) * 36 * M1), i_unc = pin.add(M1),
               i_nptr = pin.add(4 * (ix.node_ptr.size() + 1)), i_inc = pin.add(4 * (ix.inc_edge.size() + 1)),
               i_pu = pin.add(4 * (ix.pair_u.size() + 1)), i_pv = pin.add(4 * (ix.pair_v.size() + 1)),
               i_pptr = pin.add(4 * (ix.pair_ptr.size() + 1)), i_pe = pin.add(4 * (ix.pair_edge.size() + 1));
  const size_t w_cur = pwork.add(sizeof(double) * 12 * N1), w_cand = pwork.add(sizeof(double) * 12 * N1),
               w_A = pwork.add(sizeof(double) * 36 * M1), w_b = pwork.add(sizeof(double) * 6 * M1);
  const size_t G1 = (size_t)std::max<int64_t>(ix.free_unknowns, 1), R1 = (size_t)std::max<int64_t>(ix.trace_rows, 1);
  const size_t o_poses = pout.add(sizeof(double) * 16 * N1), o_conf = pout.add(sizeof(double) * M1),
               o_pruned = pout.add(M1), o_res = pout.add(sizeof(teaser_posegraph_result_c) * batch),
               o_trace = pout.add(sizeof(teaser_posegraph_trace_c) * R1), o_e = pout.add(sizeof(double) * 6 * M1),
               o_r = pout.add(sizeof(double) * M1), o_l = pout.add(sizeof(double) * M1),
               o_g = pout.add(sizeof(double) * G1);
  const size_t dense1 = (size_t)std::max<int64_t>(ix.dense, 1);
  if (!h->in.ensure(pin.bytes) || !h->work.ensure(pwork.bytes) || !h->out.ensure(pout.bytes) ||
      !h->dense.ensure(sizeof(double) * 2 * dense1))
    return fail(h, TEASER_HIP_ERR_HIP, "hipMalloc failed (pose-graph buffers)");
  std::vector<char> stage(pin.bytes, 0);
  auto put = [&](size_t at_, const void* p, size_t n) {
    if (n) memcpy(stage.data() + at_, p, n);
  };
  put(i_desc, ix.desc.data(), sizeof(PgDesc) * batch);
  put(i_poses, poses, sizeof(double) * 16 * (size_t)nodes);
  put(i_src, src, 4 * (size_t)edges);
  put(i_tgt, tgt, 4 * (size_t)edges);
  put(i_X, X, sizeof(double) * 16 * (size_t)edges);
  put(i_L, L, sizeof(double) * 36 * (size_t)edges);
  put(i_unc, unc, (size_t)edges);
  put(i_nptr, ix.node_ptr.data(), 4 * ix.node_ptr.size());
  put(i_inc, ix.inc_edge.data(), 4 * ix.inc_edge.size());
  put(i_pu, ix.pair_u.data(), 4 * ix.pair_u.size());
  put(i_pv, ix.pair_v.data(), 4 * ix.pair_v.size());
  put(i_pptr, ix.pair_ptr.data(), 4 * ix.pair_ptr.size());
  put(i_pe, ix.pair_edge.data(), 4 * ix.pair_edge.size());
  hipStream_t s = h->stream;
  FCHK(h, hipMemcpyAsync(h->in.p, stage.data(), pin.bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync (pose graphs)");

  void* din = h->in.p;
  void* dw = h->work.p;
  void* dout = h->out.p;
  PgArgs a;
  memset(&a, 0, sizeof(a));
  a.desc = Pack::at<const PgDesc>(din, i_desc);
  a.poses_in = Pack::at<const double>(din, i_poses);
  a.src = Pack::at<const int32_t>(din, i_src);
  a.tgt = Pack::at<const int32_t>(din, i_tgt);
  a.X = Pack::at<const double>(din, i_X);
  a.L = Pack::at<const double>(din, i_L);
  a.unc = Pack::at<const uint8_t>(din, i_unc);
  a.node_ptr = Pack::at<const int32_t>(din, i_nptr);
  a.inc_edge = Pack::at<const int32_t>(din, i_inc);
  a.pair_u = Pack::at<const int32_t>(din, i_pu);
  a.pair_v = Pack::at<const int32_t>(din, i_pv);
  a.pair_ptr = Pack::at<const int32_t>(din, i_pptr);
  a.pair_edge = Pack::at<const int32_t>(din, i_pe);
  a.pose_cur = Pack::at<double>(dw, w_cur);
  a.pose_cand = Pack::at<double>(dw, w_cand);
  a.A = Pack::at<double>(dw, w_A);
  a.bv = Pack::at<double>(dw, w_b);
  a.H = h->dense.as<double>();
  a.M = h->dense.as<double>() + dense1;
  a.poses_out = Pack::at<double>(dout, o_poses);
  a.conf = Pack::at<double>(dout, o_conf);
  a.pruned = Pack::at<uint8_t>(dout, o_pruned);
  a.res = Pack::at<teaser_posegraph_result_c>(dout, o_res);
  a.trace = o.trace ? Pack::at<teaser_posegraph_trace_c>(dout, o_trace) : nullptr;
  a.e = Pack::at<double>(dout, o_e);
  a.r = Pack::at<double>(dout, o_r);
  a.l = Pack::at<double>(dout, o_l);
  a.g = Pack::at<double>(dout, o_g);
  a.mode = mode;
  launch_posegraph(s, batch, a);
  FCHK(h, hipGetLastError(), "pose-graph kernel launch");

  // ---- results: one download, one synchronisation ----
  std::vector<char> back(pout.bytes);
  FCHK(h, hipMemcpyAsync(back.data(), h->out.p, pout.bytes, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (results)");
  std::vector<double> Hfree;
  if (mode == PG_MODE_LINEARIZE && o.H) {
    Hfree.resize(dense1);
    FCHK(h, hipMemcpyAsync(Hfree.data(), h->dense.p, sizeof(double) * dense1, hipMemcpyDeviceToHost, s),
         "hipMemcpyAsync (H)");
  }
  FCHK(h, hipStreamSynchronize(s), "pose-graph optimisation");
  const teaser_posegraph_result_c* res = Pack::at<const teaser_posegraph_result_c>(back.data(), o_res);
  auto get = [&](void* dst, size_t at_, size_t n) {
    if (dst && n) memcpy(dst, back.data() + at_, n);
  };
  if (mode == PG_MODE_OPTIMIZE) {
    get(o.poses_out, o_poses, sizeof(double) * 16 * (size_t)nodes);
    get(o.confidence, o_conf, sizeof(double) * (size_t)edges);
    get(o.pruned, o_pruned, (size_t)edges);
    get(o.results, o_res, sizeof(teaser_posegraph_result_c) * batch);
    if (o.trace)
      for (int b = 0; b < batch; ++b) {
        const PgDesc& d = ix.desc[(size_t)b];
        const int rows = std::min(res[b].n_trace, d.trace_cap);
        get(o.trace + d.trace_off, o_trace + sizeof(teaser_posegraph_trace_c) * (size_t)d.trace_off,
            sizeof(teaser_posegraph_trace_c) * (size_t)rows);
      }
    return TEASER_HIP_OK;
  }
  get(o.e, o_e, sizeof(double) * 6 * (size_t)edges);
  get(o.r, o_r, sizeof(double) * (size_t)edges);
  get(o.l, o_l, sizeof(double) * (size_t)edges);
  const double* gfree = Pack::at<const double>(back.data(), o_g);
  int64_t h_at = 0;
  for (int b = 0; b < batch; ++b) {
    const PgDesc& d = ix.desc[(size_t)b];
    if (o.mu) o.mu[b] = res[b].mu[0];
    if (o.F) o.F[b] = res[b].F0;
    const int64_t W = 6 * (int64_t)d.n;
    double* Hb = o.H ? o.H + h_at : nullptr;
    double* gb = o.g ? o.g + 6 * d.node_off : nullptr;
    if (Hb) std::fill(Hb, Hb + W * W, 0.0);
    if (gb) std::fill(gb, gb + W, 0.0);
    for (int i = 0; i < d.n; ++i) {  // the free unknowns back at their nodes; the reference node's stay zero
      if (i == d.ref) continue;
      const int fi = 6 * pg_free(i, d.ref);
      for (int a_ = 0; a_ < 6; ++a_) {
        if (gb) gb[6 * i + a_] = gfree[d.g_off + fi + a_];
        if (!Hb) continue;
        for (int j = 0; j < d.n; ++j) {
          if (j == d.ref) continue;
          const int fj = 6 * pg_free(j, d.ref);
          for (int c = 0; c < 6; ++c)
            Hb[(6 * i + a_) * W + 6 * j + c] = Hfree[(size_t)(d.h_off + (int64_t)(fi + a_) * d.N + fj + c)];
        }
      }
    }
    h_at += W * W;
  }
  return TEASER_HIP_OK;
}

}  // namespace

extern "C" {

int32_t teaser_hip_posegraph_create(int32_t device, teaser_hip_posegraph** out) { return open_handle(device, out); }
int32_t teaser_hip_posegraph_destroy(teaser_hip_posegraph* h) { return close_handle(h); }
const char* teaser_hip_posegraph_last_error(const teaser_hip_posegraph* h) { return h ? h->err.c_str() : ""; }

int32_t teaser_hip_posegraph_fill_scratch(teaser_hip_posegraph* h, int32_t byte, int64_t* bytes_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  const ScratchSpan spans[] = {span_of(h->in), span_of(h->work), span_of(h->dense), span_of(h->out)};
  return fill_scratch(h, byte, spans, 4, bytes_out);
}

int32_t teaser_hip_posegraph_option_default(teaser_posegraph_option_c* out) {
  if (!out) return TEASER_HIP_ERR_BAD_ARG;
  option_default(out);
  return TEASER_HIP_OK;
}

int32_t teaser_hip_posegraph_optimize_batch(teaser_hip_posegraph* h, int32_t batch, const int32_t* n_nodes,
                                            const double* poses, const int32_t* n_edges, const int32_t* edge_source,
                                            const int32_t* edge_target, const double* edge_transformation,
                                            const double* edge_information, const uint8_t* edge_uncertain,
                                            const teaser_posegraph_option_c* options, double* poses_out,
                                            double* confidence, uint8_t* pruned, teaser_posegraph_result_c* results,
                                            teaser_posegraph_trace_c* trace, const int32_t* trace_cap) {
  PgOutputs o;
  o.poses_out = poses_out;
  o.confidence = confidence;
  o.pruned = pruned;
  o.results = results;
  o.trace = trace;
  return run(h, PG_MODE_OPTIMIZE, batch, n_nodes, poses, n_edges, edge_source, edge_target, edge_transformation,
             edge_information, edge_uncertain, options, trace_cap, o);
}

int32_t teaser_hip_posegraph_optimize(teaser_hip_posegraph* h, int32_t n_nodes, const double* poses, int32_t n_edges,
                                      const int32_t* edge_source, const int32_t* edge_target,
                                      const double* edge_transformation, const double* edge_information,
                                      const uint8_t* edge_uncertain, const teaser_posegraph_option_c* option,
                                      double* poses_out, double* confidence, uint8_t* pruned,
                                      teaser_posegraph_result_c* result, teaser_posegraph_trace_c* trace,
                                      int32_t trace_cap) {
  return teaser_hip_posegraph_optimize_batch(h, 1, &n_nodes, poses, &n_edges, edge_source, edge_target,
                                             edge_transformation, edge_information, edge_uncertain, option, poses_out,
                                             confidence, pruned, result, trace, &trace_cap);
}

int32_t teaser_hip_posegraph_linearize_batch(teaser_hip_posegraph* h, int32_t batch, const int32_t* n_nodes,
                                             const double* poses, const int32_t* n_edges, const int32_t* edge_source,
                                             const int32_t* edge_target, const double* edge_transformation,
                                             const double* edge_information, const uint8_t* edge_uncertain,
                                             const teaser_posegraph_option_c* options, double* e, double* r, double* l,
                                             double* mu, double* F, double* H, double* g) {
  PgOutputs o;
  o.e = e;
  o.r = r;
  o.l = l;
  o.mu = mu;
  o.F = F;
  o.H = H;
  o.g = g;
  return run(h, PG_MODE_LINEARIZE, batch, n_nodes, poses, n_edges, edge_source, edge_target, edge_transformation,
             edge_information, edge_uncertain, options, nullptr, o);
}

int32_t teaser_hip_posegraph_linearize(teaser_hip_posegraph* h, int32_t n_nodes, const double* poses, int32_t n_edges,
                                       const int32_t* edge_source, const int32_t* edge_target,
                                       const double* edge_transformation, const double* edge_information,
                                       const uint8_t* edge_uncertain, const teaser_posegraph_option_c* option,
                                       double* e, double* r, double* l, double* mu, double* F, double* H, double* g) {
  return teaser_hip_posegraph_linearize_batch(h, 1, &n_nodes, poses, &n_edges, edge_source, edge_target,
                                              edge_transformation, edge_information, edge_uncertain, option, e, r, l,
                                              mu, F, H, g);
}

}  // extern "C"
