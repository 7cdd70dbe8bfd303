// Host-only check of csrc/posegraph.hip (tests/test_posegraph_host.py): compiled by g++ against the HIP stand-in header
// (tests/hip_stub) with -fsanitize=address,undefined as a stand-alone program.  The launcher is a stand-in that checks
// the CSR of incident edges and the pair lists of every graph against brute force, reads every input element and
// writes every element of every work, scratch and output array the kernel may touch (a buffer sized or packed at a
// wrong offset is an AddressSanitizer report or a wrong value here), and leaves recognisable values.  Then the entry
// checks: every refusal names its argument and the problem, and leaves the outputs alone.
//   posegraph_host_driver    exit code 0 and "mismatches 0": every expectation met
// TEST INFRASTRUCTURE ONLY.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <limits>
#include <set>
#include <utility>

#include "../teaser-plusplus_amd/csrc/posegraph.hip"

static int g_bad = 0, g_launches = 0, g_last_batch = -1;
#define EXPECT(c)                                          \
  do {                                                     \
    if (!(c)) {                                            \
      ++g_bad;                                             \
      printf("line %d: expectation failed: %s\n", __LINE__, #c); \
    }                                                      \
  } while (0)

namespace thip {

void launch_posegraph(hipStream_t, int batch, const PgArgs& a) {
  ++g_launches;
  g_last_batch = batch;
  for (int b = 0; b < batch; ++b) {
    const PgDesc& D = a.desc[b];
    const int32_t* s = a.src + D.edge_off;
    const int32_t* t = a.tgt + D.edge_off;
    EXPECT(D.N == (D.n > 1 ? 6 * (D.n - 1) : 0));
    EXPECT(D.ref == (D.opt.reference_node < 0 ? 0 : D.opt.reference_node));
    // the CSR against brute force: node i's row lists exactly the edges that touch it, ascending
    const int32_t* nptr = a.node_ptr + D.nodeptr_off;
    EXPECT(nptr[0] == 0 && nptr[D.n] == 2 * D.m);
    for (int i = 0; i < D.n; ++i) {
      int q = nptr[i];
      for (int k = 0; k < D.m; ++k)
        if (s[k] == i || t[k] == i) {
          EXPECT(q < nptr[i + 1] && a.inc_edge[D.inc_off + q] == k);
          ++q;
        }
      EXPECT(q == nptr[i + 1]);
    }
    // the pair lists against brute force: the distinct unordered pairs in ascending order, each with its edges
    // (either direction) ascending
    std::set<std::pair<int, int>> want;
    for (int k = 0; k < D.m; ++k) want.insert({std::min(s[k], t[k]), std::max(s[k], t[k])});
    EXPECT((int)want.size() == D.n_pairs);
    const int32_t* pptr = a.pair_ptr + D.pairptr_off;
    EXPECT(pptr[0] == 0 && pptr[D.n_pairs] == D.m);
    int p = 0;
    for (const auto& uv : want) {
      EXPECT(a.pair_u[D.pair_off + p] == uv.first && a.pair_v[D.pair_off + p] == uv.second);
      int q = pptr[p];
      for (int k = 0; k < D.m; ++k)
        if (std::min(s[k], t[k]) == uv.first && std::max(s[k], t[k]) == uv.second) {
          EXPECT(q < pptr[p + 1] && a.pair_edge[D.edge_off + q] == k);
          ++q;
        }
      EXPECT(q == pptr[p + 1]);
      ++p;
    }
    // every element the kernel reads or writes
    double sum = 0.0;
    for (int i = 0; i < 16 * D.n; ++i) sum += a.poses_in[16 * D.node_off + i];
    for (int k = 0; k < D.m; ++k) {
      for (int i = 0; i < 16; ++i) sum += a.X[16 * (D.edge_off + k) + i];
      for (int i = 0; i < 36; ++i) sum += a.L[36 * (D.edge_off + k) + i];
      sum += a.unc[D.edge_off + k];
      for (int i = 0; i < 36; ++i) a.A[36 * (D.edge_off + k) + i] = 1.0;
      for (int i = 0; i < 6; ++i) a.bv[6 * (D.edge_off + k) + i] = a.e[6 * (D.edge_off + k) + i] = 100.0 * b + k + 0.1 * i;
      a.r[D.edge_off + k] = 200.0 * b + k;
      a.l[D.edge_off + k] = 300.0 * b + k;
      a.conf[D.edge_off + k] = 400.0 * b + k;
      a.pruned[D.edge_off + k] = (uint8_t)(k % 2);
    }
    EXPECT(sum == sum || true);  // the lower triangles hold NaN here: read, never used
    for (int i = 0; i < 12 * D.n; ++i) a.pose_cur[12 * D.node_off + i] = a.pose_cand[12 * D.node_off + i] = 0.0;
    for (int i = 0; i < 16 * D.n; ++i) a.poses_out[16 * D.node_off + i] = a.poses_in[16 * D.node_off + i] + 1000.0;
    for (int64_t i = 0; i < (int64_t)D.N * D.N; ++i) {
      a.H[D.h_off + i] = 1000.0 * b + (double)i;  // entry (i / N, i % N) of the free system
      a.M[D.h_off + i] = 0.0;
    }
    for (int i = 0; i < D.N; ++i) a.g[D.g_off + i] = 500.0 * b + i;
    teaser_posegraph_result_c& res = a.res[b];
    res.F0 = 10.0 + b;
    res.F = 20.0 + b;
    res.mu[0] = 30.0 + b;
    res.mu[1] = 40.0 + b;
    res.iterations[0] = res.iterations[1] = res.trials[0] = res.trials[1] = b;
    res.status = a.mode == PG_MODE_OPTIMIZE ? (D.trivial ? TEASER_HIP_PG_TRIVIAL : TEASER_HIP_PG_RESIDUAL) : -1;
    res.n_trace = a.trace ? D.trace_cap + 3 : 0;  // more rows than fit: the count is still reported
    for (int q = 0; a.trace && q < D.trace_cap; ++q) {
      teaser_posegraph_trace_c& row = a.trace[D.trace_off + q];
      row.lam = 1000.0 * b + q;
      row.rho = row.F_new = 0.5;
      row.pass = 0;
      row.accepted = row.factorised = 1;
      row.reserved = 0;
    }
  }
}

}  // namespace thip

namespace {

struct Batch {
  std::vector<int32_t> n, m, src, tgt;
  std::vector<double> poses, X, L;
  std::vector<uint8_t> unc;
  std::vector<teaser_posegraph_option_c> opt;
  void add(int nodes, std::vector<std::pair<int, int>> edges, int ref) {
    const int b = (int)n.size();
    n.push_back(nodes);
    m.push_back((int)edges.size());
    for (int i = 0; i < nodes; ++i)
      for (int k = 0; k < 16; ++k) poses.push_back(k == 15 ? 1.0 : k >= 12 ? 0.0 : b + 0.01 * i + 0.001 * k);
    for (size_t k = 0; k < edges.size(); ++k) {
      src.push_back(edges[k].first);
      tgt.push_back(edges[k].second);
      for (int q = 0; q < 16; ++q) X.push_back(q == 15 ? 1.0 : q >= 12 ? 0.0 : 0.5 * q);
      for (int q = 0; q < 36; ++q) L.push_back(q / 6 > q % 6 ? std::numeric_limits<double>::quiet_NaN() : 1.0 + q);
      unc.push_back((uint8_t)(k % 3 == 0));
    }
    teaser_posegraph_option_c o;
    teaser_hip_posegraph_option_default(&o);
    o.reference_node = ref;
    opt.push_back(o);
  }
};

struct Outputs {
  std::vector<double> poses_out, conf;
  std::vector<uint8_t> pruned;
  std::vector<teaser_posegraph_result_c> res;
  std::vector<teaser_posegraph_trace_c> trace;
  std::vector<int32_t> cap;
  explicit Outputs(const Batch& B) {
    poses_out.assign(B.poses.size() + 1, -7.0);
    conf.assign(B.src.size() + 1, -7.0);
    pruned.assign(B.src.size() + 1, 77);
    res.resize(B.n.size() + 1);
    for (auto& r : res) r.status = -77;
    for (size_t b = 0; b < B.n.size(); ++b) cap.push_back((int32_t)(b % 3));
    trace.resize(3 * B.n.size() + 1);
    for (auto& r : trace) r.pass = -77;
  }
  bool untouched() const {
    for (double v : poses_out)
      if (v != -7.0) return false;
    for (double v : conf)
      if (v != -7.0) return false;
    for (uint8_t v : pruned)
      if (v != 77) return false;
    for (const auto& r : res)
      if (r.status != -77) return false;
    for (const auto& r : trace)
      if (r.pass != -77) return false;
    return true;
  }
};

int32_t optimize(teaser_hip_posegraph* h, const Batch& B, Outputs& O) {
  return teaser_hip_posegraph_optimize_batch(h, (int32_t)B.n.size(), B.n.data(), B.poses.data(), B.m.data(),
                                             B.src.data(), B.tgt.data(), B.X.data(), B.L.data(), B.unc.data(),
                                             B.opt.data(), O.poses_out.data(), O.conf.data(), O.pruned.data(),
                                             O.res.data(), O.trace.data(), O.cap.data());
}

Batch good() {
  Batch B;
  // duplicate pair (2, 1) twice, its reverse, a node (4) without an edge, the reference in the middle
  B.add(5, {{1, 0}, {2, 1}, {2, 1}, {1, 2}, {3, 2}, {0, 3}, {3, 0}}, 2);
  B.add(1, {}, -1);                          // trivial
  B.add(3, {{2, 0}, {0, 1}}, 2);             // reference = n - 1
  B.add(0, {}, -1);                          // empty
  B.add(4, {}, 0);                           // no edge: trivial
  B.add(2, {{1, 0}}, -1);
  return B;
}

// a refusal: BAD_ARG, the message holds `what` (and the problem index when given), outputs untouched, no launch
void refuse(teaser_hip_posegraph* h, const Batch& B, const char* what, int problem) {
  Outputs O(B);
  const int before = g_launches;
  const int32_t rc = optimize(h, B, O);
  const std::string msg = teaser_hip_posegraph_last_error(h);
  const bool ok = rc == TEASER_HIP_ERR_BAD_ARG && msg.find(what) != std::string::npos &&
                  (problem < 0 || msg.find("(problem " + std::to_string(problem) + ")") != std::string::npos) &&
                  O.untouched() && g_launches == before;
  if (!ok) {
    ++g_bad;
    printf("refusal '%s': rc %d message '%s' untouched %d launches %d\n", what, rc, msg.c_str(), (int)O.untouched(),
           g_launches - before);
  }
}

}  // namespace

int main() {
  teaser_hip_posegraph* h = nullptr;
  EXPECT(teaser_hip_posegraph_create(-1, &h) == TEASER_HIP_OK && h);
  teaser_posegraph_option_c def;
  EXPECT(teaser_hip_posegraph_option_default(&def) == TEASER_HIP_OK && def.max_iteration == 100 &&
         def.max_iteration_lm == 20 && def.upper_scale_factor == 2.0 / 3.0 && def.lower_scale_factor == 1.0 / 3.0 &&
         def.max_correspondence_distance == 0.03 && def.edge_prune_threshold == 0.25 && def.reference_node == -1 &&
         def.preference_loop_closure == 1.0 && def.min_residual == 1e-6);
  EXPECT(teaser_hip_posegraph_option_default(nullptr) == TEASER_HIP_ERR_BAD_ARG);

  // ---- a good batch, twice (the second call reuses the buffers), then a smaller and a larger one ----
  const Batch B = good();
  for (int rep = 0; rep < 2; ++rep) {
    Outputs O(B);
    EXPECT(optimize(h, B, O) == TEASER_HIP_OK);
    EXPECT(g_last_batch == (int)B.n.size());
    size_t no = 0, mo = 0, to = 0;
    for (size_t b = 0; b < B.n.size(); ++b) {
      for (int i = 0; i < 16 * B.n[b]; ++i) EXPECT(O.poses_out[16 * no + i] == B.poses[16 * no + i] + 1000.0);
      for (int k = 0; k < B.m[b]; ++k) {
        EXPECT(O.conf[mo + k] == 400.0 * b + k && O.pruned[mo + k] == k % 2);
      }
      EXPECT(O.res[b].F0 == 10.0 + b && O.res[b].mu[1] == 40.0 + b && O.res[b].iterations[1] == (int)b);
      EXPECT(O.res[b].status == (B.n[b] <= 1 || B.m[b] == 0 ? TEASER_HIP_PG_TRIVIAL : TEASER_HIP_PG_RESIDUAL));
      EXPECT(O.res[b].n_trace == O.cap[b] + 3);
      for (int q = 0; q < O.cap[b]; ++q) EXPECT(O.trace[to + q].lam == 1000.0 * b + q && O.trace[to + q].pass == 0);
      no += B.n[b];
      mo += B.m[b];
      to += O.cap[b];
    }
    EXPECT(O.poses_out.back() == -7.0 && O.conf.back() == -7.0 && O.pruned.back() == 77 && O.res.back().status == -77);
    for (size_t q = to; q < O.trace.size(); ++q) EXPECT(O.trace[q].pass == -77);  // rows beyond the capacities
  }
  {
    Outputs O(B);  // optional outputs NULL
    EXPECT(teaser_hip_posegraph_optimize_batch(h, (int32_t)B.n.size(), B.n.data(), B.poses.data(), B.m.data(),
                                               B.src.data(), B.tgt.data(), B.X.data(), B.L.data(), B.unc.data(), nullptr,
                                               O.poses_out.data(), nullptr, nullptr, nullptr, nullptr, nullptr) ==
           TEASER_HIP_OK);
    EXPECT(O.poses_out[0] == B.poses[0] + 1000.0 && O.conf[0] == -7.0);
    EXPECT(teaser_hip_posegraph_optimize_batch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr) == TEASER_HIP_OK);
  }
  {  // the largest graph the limits admit, beside a small one: the dense scratch holds both slices
    Batch Big;
    std::vector<std::pair<int, int>> ring;
    for (int i = 0; i < TEASER_HIP_POSEGRAPH_MAX_NODES; ++i) ring.push_back({(i + 1) % TEASER_HIP_POSEGRAPH_MAX_NODES, i});
    Big.add(2, {{0, 1}}, -1);
    Big.add(TEASER_HIP_POSEGRAPH_MAX_NODES, ring, 5);
    Outputs O(Big);
    EXPECT(optimize(h, Big, O) == TEASER_HIP_OK && O.res[1].status == TEASER_HIP_PG_RESIDUAL);
    // the stage call: H comes back with the free unknowns at their nodes and zero reference rows and columns
    const int n = TEASER_HIP_POSEGRAPH_MAX_NODES, W = 6 * n, N = 6 * (n - 1);
    std::vector<double> e(6 * (ring.size() + 1) + 1, -7.0), r(ring.size() + 2, -7.0), l(ring.size() + 2, -7.0), mu(3, -7.0),
        F(3, -7.0), H(144 + (size_t)W * W + 1, -7.0), g(12 + W + 1, -7.0);
    EXPECT(teaser_hip_posegraph_linearize_batch(h, 2, Big.n.data(), Big.poses.data(), Big.m.data(), Big.src.data(),
                                                Big.tgt.data(), Big.X.data(), Big.L.data(), Big.unc.data(),
                                                Big.opt.data(), e.data(), r.data(), l.data(), mu.data(), F.data(),
                                                H.data(), g.data()) == TEASER_HIP_OK);
    EXPECT(e[6 * 1 + 2] == 100.0 + 0 + 0.2 && e.back() == -7.0 && r[1] == 200.0 && l[2] == 301.0 && r.back() == -7.0);
    EXPECT(mu[0] == 30.0 && mu[1] == 31.0 && F[1] == 11.0 && mu[2] == -7.0 && H.back() == -7.0 && g.back() == -7.0);
    const double* Hb = H.data() + 144;
    const double* gb = g.data() + 12;
    int bad = 0;
    for (int i = 0; i < W; ++i)
      for (int j = 0; j < W; ++j) {
        const int ni = i / 6, nj = j / 6;
        double want = 0.0;
        if (ni != 5 && nj != 5) {
          const int fi = 6 * (ni < 5 ? ni : ni - 1) + i % 6, fj = 6 * (nj < 5 ? nj : nj - 1) + j % 6;
          want = 1000.0 + (double)((int64_t)fi * N + fj);
        }
        bad += Hb[(size_t)i * W + j] != want;
      }
    EXPECT(bad == 0);
    for (int i = 0; i < W; ++i) {
      const int ni = i / 6;
      bad += gb[i] != (ni == 5 ? 0.0 : 500.0 + 6 * (ni < 5 ? ni : ni - 1) + i % 6);
    }
    EXPECT(bad == 0);
    EXPECT(H[0] == 0.0 && H[6 * 12 + 6] == 0.0 + 0.0 && g[6] == 0.0);  // graph 0: reference node 0, free block from h_off 0
    EXPECT(H[(size_t)7 * 12 + 8] == 1.0 * 6 + 2);
  }

  // ---- refusals ----
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  {
    Outputs O(B);
    EXPECT(teaser_hip_posegraph_optimize_batch(h, -1, B.n.data(), B.poses.data(), B.m.data(), B.src.data(), B.tgt.data(),
                                               B.X.data(), B.L.data(), B.unc.data(), B.opt.data(), O.poses_out.data(),
                                               nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG);
    EXPECT(std::string(teaser_hip_posegraph_last_error(h)) == "batch must be >= 0" && O.untouched());
    // the empty batch is answered before any argument is looked at and clears the message; no handle, no message
    EXPECT(teaser_hip_posegraph_optimize_batch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK);
    EXPECT(std::string(teaser_hip_posegraph_last_error(h)).empty());
    EXPECT(teaser_hip_posegraph_optimize_batch(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr) == TEASER_HIP_ERR_BAD_ARG);
    EXPECT(teaser_hip_posegraph_optimize_batch(h, 6, nullptr, B.poses.data(), B.m.data(), B.src.data(), B.tgt.data(),
                                               B.X.data(), B.L.data(), B.unc.data(), B.opt.data(), O.poses_out.data(),
                                               nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG);
    EXPECT(std::string(teaser_hip_posegraph_last_error(h)).find("n_nodes") != std::string::npos);
    EXPECT(teaser_hip_posegraph_optimize_batch(h, 6, B.n.data(), nullptr, B.m.data(), B.src.data(), B.tgt.data(),
                                               B.X.data(), B.L.data(), B.unc.data(), B.opt.data(), O.poses_out.data(),
                                               nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG);
    EXPECT(std::string(teaser_hip_posegraph_last_error(h)).find("poses is NULL (problem 0)") != std::string::npos);
    EXPECT(teaser_hip_posegraph_optimize_batch(h, 6, B.n.data(), B.poses.data(), B.m.data(), B.src.data(), B.tgt.data(),
                                               B.X.data(), nullptr, B.unc.data(), B.opt.data(), O.poses_out.data(),
                                               nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG);
    EXPECT(std::string(teaser_hip_posegraph_last_error(h)).find("edge_information is NULL") != std::string::npos);
    EXPECT(teaser_hip_posegraph_optimize_batch(h, 6, B.n.data(), B.poses.data(), B.m.data(), B.src.data(), B.tgt.data(),
                                               B.X.data(), B.L.data(), B.unc.data(), B.opt.data(), nullptr, nullptr,
                                               nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG);
    EXPECT(std::string(teaser_hip_posegraph_last_error(h)).find("poses_out is NULL") != std::string::npos);
    EXPECT(teaser_hip_posegraph_optimize_batch(h, 6, B.n.data(), B.poses.data(), B.m.data(), B.src.data(), B.tgt.data(),
                                               B.X.data(), B.L.data(), B.unc.data(), B.opt.data(), O.poses_out.data(),
                                               nullptr, nullptr, nullptr, O.trace.data(), nullptr) ==
           TEASER_HIP_ERR_BAD_ARG);
    EXPECT(std::string(teaser_hip_posegraph_last_error(h)).find("trace_cap") != std::string::npos && O.untouched());
  }
  Batch C = good();
  C.poses[16 * 5 + 3] = nan;  // node 0 of problem 1
  refuse(h, C, "poses: node 0 is not finite", 1);
  C = good();
  C.poses[16 * 6 + 13] = 0.5;  // node 0 of problem 2
  refuse(h, C, "poses: last row of node 0 must be 0 0 0 1", 2);
  C = good();
  C.X[16 * 7 + 2] = inf;  // edge 0 of problem 2
  refuse(h, C, "edge_transformation: edge 0 is not finite", 2);
  C = good();
  C.X[16 * 2 + 15] = 2.0;
  refuse(h, C, "edge_transformation: last row of edge 2 must be 0 0 0 1", 0);
  C = good();
  C.L[36 * 1 + 6 * 1 + 4] = nan;  // upper triangle
  refuse(h, C, "edge_information: edge 1 is not finite", 0);
  C = good();
  C.src[8] = 3;  // edge 1 of problem 2 (n = 3)
  refuse(h, C, "edge_source: edge 1 is out of range", 2);
  C = good();
  C.tgt[0] = -1;
  refuse(h, C, "edge_target: edge 0 is out of range", 0);
  C = good();
  C.tgt[9] = C.src[9];
  refuse(h, C, "edge_source == edge_target at edge 0", 5);
  C = good();
  C.opt[2].reference_node = 3;
  refuse(h, C, "options.reference_node must be < n_nodes", 2);
  C = good();
  C.opt[3].reference_node = 0;  // n = 0
  refuse(h, C, "options.reference_node must be < n_nodes", 3);
  C = good();
  C.opt[0].max_iteration = -1;
  refuse(h, C, "options.max_iteration must be >= 0", 0);
  C = good();
  C.opt[5].max_iteration_lm = -2;
  refuse(h, C, "options.max_iteration_lm must be >= 0", 5);
  C = good();
  C.opt[0].max_iteration = TEASER_HIP_POSEGRAPH_MAX_ITERATION + 1;
  refuse(h, C, "options.max_iteration exceeds", 0);
  C = good();
  C.opt[0].max_iteration_lm = TEASER_HIP_POSEGRAPH_MAX_ITERATION_LM + 1;
  refuse(h, C, "options.max_iteration_lm exceeds", 0);
  C = good();
  C.opt[4].min_right_term = nan;
  refuse(h, C, "options.min_right_term is not finite", 4);
  C = good();
  C.opt[1].edge_prune_threshold = inf;
  refuse(h, C, "options.edge_prune_threshold is not finite", 1);
  C = good();
  C.n[1] = -1;
  refuse(h, C, "n_nodes must be >= 0", 1);
  C = good();
  C.n[4] = TEASER_HIP_POSEGRAPH_MAX_NODES + 1;
  refuse(h, C, "n_nodes exceeds TEASER_HIP_POSEGRAPH_MAX_NODES", 4);
  C = good();
  C.m[0] = TEASER_HIP_POSEGRAPH_MAX_EDGES + 1;
  refuse(h, C, "n_edges exceeds TEASER_HIP_POSEGRAPH_MAX_EDGES", 0);
  {  // the information matrix is NOT checked for definiteness, and its lower triangle is never read (NaN there)
    Batch D = good();
    for (int q = 0; q < 6; ++q) D.L[36 * 0 + 7 * q] = -1.0;
    Outputs O(D);
    EXPECT(optimize(h, D, O) == TEASER_HIP_OK);
  }
  {  // the handle stays usable after the refusals
    Outputs O(B);
    EXPECT(optimize(h, B, O) == TEASER_HIP_OK && std::string(teaser_hip_posegraph_last_error(h)).empty());
  }
  EXPECT(teaser_hip_posegraph_destroy(h) == TEASER_HIP_OK);
  printf("launches %d mismatches %d\n", g_launches, g_bad);
  return g_bad ? 1 : 0;
}
