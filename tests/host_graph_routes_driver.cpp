// Driver of csrc/solver.hip's graph routing against the HIP stub (tests/test_host_graph_routes.py, with
// tests/host_route_stub_launchers.cpp recording the phase of every launch_tim_graph_mfma call).  One handle walks
//   fresh handle, all-closed batch, all-closed batch, 1 of 32 open, 8 of 32 open, all-closed batch, all-closed batch
// and the phases seen must follow the rule of solve_packed_enqueue: K1 stores nothing (kTimNoStore on phases 1 and 2,
// kTimClosurePairs in front of the closure) exactly when the handle's previous closure batch left at most 1/32 of its
// problems open; otherwise the upper triangle (kTimUpperOnly).  kTimRebuildOpen appears exactly on the no-store batches
// whose heuristic stage is enqueued (behind the closure, or by the finish half under heu_skip_closed = 1),
// kTimMirrorOpen on the others'; the bitmap getter triggers kTimRebuild once.  Usage: driver <heu_skip_closed 0|1>
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "internal.h"
#include "teaser_hip.h"

extern std::atomic<unsigned> g_stub_open_mask, g_stub_closed_mask;
extern std::atomic<int> g_stub_heuristic_stages;
extern std::vector<int> g_route_phases;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
      std::exit(3);                                                          \
    }                                                                        \
  } while (0)

static int count(int phase) { return (int)std::count(g_route_phases.begin(), g_route_phases.end(), phase); }

int main(int argc, char** argv) {
  using namespace thip;
  const int skip_closed = argc > 1 ? std::atoi(argv[1]) : 0;
  CHECK(teaser_hip_set_option(nullptr, "heu_skip_closed", skip_closed) == TEASER_HIP_OK);
  teaser_params_c P;
  CHECK(teaser_hip_params_default(&P) == TEASER_HIP_OK);
  P.estimate_scaling = 0;
  teaser_hip_solver* h = nullptr;
  CHECK(teaser_hip_solver_create(&P, 0, &h) == TEASER_HIP_OK);
  constexpr int kBatch = 32, kN = 40;
  std::vector<double> src(3 * kBatch * kN), dst(3 * kBatch * kN);
  for (size_t i = 0; i < src.size(); ++i) src[i] = dst[i] = (double)(i % 97) * 0.01;
  std::vector<int32_t> n(kBatch, kN);
  std::vector<int64_t> off(kBatch);
  for (int b = 0; b < kBatch; ++b) off[(size_t)b] = (int64_t)b * kN;
  std::vector<teaser_solution_c> out(kBatch);
  g_stub_open_mask.store(0u);  // (the stub's peel proves every problem the closure leaves to it: no bound stage)

  struct Step { unsigned closed; int open; bool nostore; };
  const Step steps[] = {
      {~0u, 0, false},          // a fresh handle: the storing route
      {~0u, 0, true},           // behind 0 of 32
      {~0u ^ (1u << 5), 1, true},   // behind 0 of 32; leaves 1 of 32
      {~0xffu, 8, true},        // behind 1 of 32: 32 <= 32; leaves 8 of 32
      {~0u, 0, false},          // behind 8 of 32: 256 > 32
      {~0u, 0, true},           // behind 0 of 32
  };
  bool prev_all_closed = false;  // (what heu_skip_closed = 1 looks at)
  for (const Step& st : steps) {
    g_route_phases.clear();
    const int stages0 = g_stub_heuristic_stages.load();
    g_stub_closed_mask.store(st.closed);
    CHECK(teaser_hip_solve_batch_device(h, src.data(), dst.data(), off.data(), n.data(), kBatch, out.data()) == TEASER_HIP_OK);
    const int stages = g_stub_heuristic_stages.load() - stages0;
    const int flag = st.nostore ? kTimNoStore : kTimUpperOnly;
    // the K1 phase: pre-pass, K1 and fix-up with the route's store flag, in this order, once each
    CHECK(g_route_phases.size() >= 3 && g_route_phases[0] == 0 && g_route_phases[1] == (1 | flag) && g_route_phases[2] == (2 | flag));
    CHECK(count(1 | kTimNoStore) + count(1 | kTimUpperOnly) + count(1) == 1);
    CHECK(count(2 | kTimNoStore) + count(2 | kTimUpperOnly) + count(2) == 1);
    // the closure's pair phase: right behind the fix-up, on the no-store route only
    CHECK(count(kTimClosurePairs) == (st.nostore ? 1 : 0));
    if (st.nostore) CHECK(g_route_phases[3] == kTimClosurePairs);
    // the heuristic stage: enqueued behind the closure, or by the finish half for the problems left open
    const bool enqueued_behind = !(skip_closed && prev_all_closed);
    CHECK(stages == ((enqueued_behind || st.open > 0) ? 1 : 0));
    CHECK(count(kTimRebuildOpen) == (st.nostore ? stages : 0));
    CHECK(count(kTimMirrorOpen) == (st.nostore ? 0 : stages));
    CHECK(count(kTimRebuild) == 0 && count(kTimMirror) == 0);
    int32_t route = -1;
    int64_t rebuilt = -1;
    CHECK(teaser_hip_get_graph_route(h, 0, &route, &rebuilt) == TEASER_HIP_OK);
    CHECK(route == (st.nostore ? 2 : 1) && rebuilt == (st.nostore ? st.open : 0));
    for (int b = 0; b < kBatch; ++b) CHECK(out[(size_t)b].n == kN);
    prev_all_closed = st.open == 0;
  }
  // the getters behind the last (no-store) batch: one rebuild of every problem, whichever getter comes first and however
  // many calls follow
  g_route_phases.clear();
  std::vector<uint64_t> bm((size_t)kN * 8);
  for (int rep = 0; rep < 2; ++rep)
    for (int b : {3, 0}) {
      int64_t len = kN;
      CHECK(teaser_hip_get_inlier_graph_bitmap(h, b, bm.data(), &len) == TEASER_HIP_OK && len == kN);
      int32_t stride = 0;
      len = (int64_t)bm.size();
      CHECK(teaser_hip_get_inlier_graph_rows(h, b, bm.data(), &len, &stride) == TEASER_HIP_OK && stride == 8 && len == 8 * kN);
    }
  CHECK(g_route_phases.size() == 1 && g_route_phases[0] == kTimRebuild);
  int32_t route = -1;
  int64_t rebuilt = -1;
  CHECK(teaser_hip_get_graph_route(h, 0, &route, &rebuilt) == TEASER_HIP_OK && route == 2 && rebuilt == kBatch);
  // a sizing call (buf == NULL) rebuilds nothing
  g_stub_closed_mask.store(~0u);
  CHECK(teaser_hip_solve_batch_device(h, src.data(), dst.data(), off.data(), n.data(), kBatch, out.data()) == TEASER_HIP_OK);
  g_route_phases.clear();
  int64_t len = 0;
  CHECK(teaser_hip_get_inlier_graph_bitmap(h, 0, nullptr, &len) == TEASER_HIP_OK && len == kN);
  CHECK(g_route_phases.empty());
  teaser_hip_solver_destroy(h);
  std::printf("ok skip_closed %d\n", skip_closed);
  return 0;
}
