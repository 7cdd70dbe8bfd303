
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "hip/hip_runtime.h"
#include "teaser_hip.h"
extern std::atomic<unsigned> g_stub_open_mask, g_stub_closed_mask;
#define CALL(x) do { stub_log("== %s", #x); int rc_ = (x); stub_log("-> %d", rc_); } while (0)
int main() {
  teaser_params_c p; teaser_hip_params_default(&p); p.estimate_scaling = 0;
  teaser_hip_solver* h = nullptr;
  CALL(teaser_hip_solver_create(&p, 0, &h));
  const int32_t n[3] = {40, 100, 17};
  std::vector<double> pts(3 * 200, 0.5);
  const double* sp[3] = {pts.data(), pts.data(), pts.data()};
  teaser_solution_c out[3];
  g_stub_open_mask = 1;  // problem 0 open: host bound path + exact search, next batch speculative
  CALL(teaser_hip_solve_batch(h, sp, sp, n, 3, out));
  CALL(teaser_hip_solve_batch(h, sp, sp, n, 3, out));
  g_stub_open_mask = 0; g_stub_closed_mask = 6;
  CALL(teaser_hip_solve_batch(h, sp, sp, n, 3, out));
  g_stub_closed_mask = 0;
  const int64_t off[3] = {0, 40, 140};
  int32_t t0 = -1, t1 = -1;
  CALL(teaser_hip_submit_batch(h, pts.data(), pts.data(), off, n, 3, TEASER_HIP_INPUT_HOST, &t0));
  CALL(teaser_hip_wait(h, t0, out));
  CALL(teaser_hip_submit_batch(h, pts.data(), pts.data(), off, n, 3, TEASER_HIP_INPUT_HOST, &t0));
  CALL(teaser_hip_submit_batch(h, pts.data(), pts.data(), off, n, 3, TEASER_HIP_INPUT_HOST, &t1));
  CALL(teaser_hip_wait(h, t0, out));
  CALL(teaser_hip_wait(h, t1, out));
  // stage calls, small route then large route
  std::vector<uint64_t> bm((size_t)1000 * 16, ~0ull);
  std::vector<int32_t> cl(1000); int32_t cs = 0, er = 0;
  g_stub_open_mask = 1;
  CALL(teaser_hip_max_clique(h, bm.data(), 100, cl.data(), &cs, &er));
  CALL(teaser_hip_max_clique(h, bm.data(), 1000, cl.data(), &cs, &er));
  g_stub_open_mask = 0;
  CALL(teaser_hip_max_clique(h, bm.data(), 768, cl.data(), &cs, &er));
  CALL(teaser_hip_max_clique(h, bm.data(), 769, cl.data(), &cs, &er));
  const int big = (1 << 18) + 1;
  std::vector<double> x((size_t)3 * big, 1.0); std::vector<uint8_t> mask((size_t)big);
  double est = 0;
  CALL(teaser_hip_scalar_tls(h, x.data(), x.data(), 17, &est, mask.data()));
  CALL(teaser_hip_scalar_tls(h, x.data(), x.data(), 1 << 18, &est, nullptr));
  CALL(teaser_hip_scalar_tls(h, x.data(), x.data(), big, &est, mask.data()));
  CALL(teaser_hip_solve_for_scale(h, x.data(), x.data(), 100, &est, mask.data()));   // fixed scale
  double tr[3], R[9];
  CALL(teaser_hip_solve_for_translation(h, x.data(), x.data(), 50, tr, mask.data()));
  CALL(teaser_hip_solve_for_rotation(h, x.data(), x.data(), 50, 0.01, R, mask.data(), nullptr, nullptr));
  p.estimate_scaling = 1;
  CALL(teaser_hip_solver_reset(h, &p));
  CALL(teaser_hip_solve_for_scale(h, x.data(), x.data(), 100, &est, mask.data()));
  CALL(teaser_hip_solve_for_scale(h, x.data(), x.data(), big, &est, mask.data()));
  CALL(teaser_hip_solve_for_scale(h, x.data(), x.data(), big, &est, nullptr));
  p.estimate_scaling = 0; p.inlier_selection_mode = TEASER_INLIER_KCORE_HEU;
  CALL(teaser_hip_solver_reset(h, &p));
  CALL(teaser_hip_max_clique(h, bm.data(), 100, cl.data(), &cs, &er));
  p.inlier_selection_mode = TEASER_INLIER_PMC_EXACT;
  CALL(teaser_hip_solver_reset(h, &p));
  CALL(teaser_hip_solve_batch(h, sp, sp, n, 3, out));   // views back after the stage calls
  CALL(teaser_hip_set_pipeline_depth(h, 1));
  CALL(teaser_hip_submit_batch(h, pts.data(), pts.data(), off, n, 3, 0, &t0));
  CALL(teaser_hip_wait(h, t0, out));
  CALL(teaser_hip_set_pipeline_depth(h, 3));
  CALL(teaser_hip_submit_batch(h, pts.data(), pts.data(), off, n, 3, 0, &t0));
  CALL(teaser_hip_wait(h, t0, out));
  CALL(teaser_hip_solver_destroy(h));
  return 0;
}
