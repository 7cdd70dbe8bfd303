// teaser::globalOptimization (include/teaser/posegraph.h) used like Open3D's GlobalOptimization.
//   posegraph_example                   a chain of three nodes with one displaced start pose: the optimiser puts it
//                                       back; 0 ok, 1 wrong result
//   posegraph_example GRAPH RESULT      reads a graph file and writes a result file, both in the format of
//                                       tests/posegraph_emulation.cpp, through the in-place call and a trace of 64 rows
// Exit code 77: no MI355X visible (loud failure, no CPU path); 1: any other failure.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "teaser/posegraph.h"

int main(int argc, char** argv) {
  try {
    teaser::PoseGraphOptimizer optimizer;
    teaser::GlobalOptimizationLevenbergMarquardt lm;
    if (argc == 3) {
      FILE* in = std::fopen(argv[1], "r");
      if (!in) return 2;
      int n = 0, m = 0;
      teaser::GlobalOptimizationConvergenceCriteria cr;
      teaser::GlobalOptimizationOption op;
      bool ok = std::fscanf(in, "%d %d", &n, &m) == 2;
      ok = ok && std::fscanf(in, "%d %d %lf %lf %lf %lf %lf %lf %lf %lf %lf %d", &cr.max_iteration, &cr.max_iteration_lm,
                             &cr.min_relative_increment, &cr.min_relative_residual_increment, &cr.min_right_term,
                             &cr.min_residual, &cr.upper_scale_factor, &cr.lower_scale_factor,
                             &op.max_correspondence_distance, &op.edge_prune_threshold, &op.preference_loop_closure,
                             &op.reference_node) == 12;
      if (!ok || n < 0 || m < 0 || n > 4096 || m > 65536) return 2;
      teaser::PoseGraph g;
      g.nodes.resize((size_t)n);
      g.edges.resize((size_t)m);
      for (auto& node : g.nodes)
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) ok = ok && std::fscanf(in, "%lf", &node.pose(r, c)) == 1;
      for (auto& e : g.edges) {
        int unc = 0;
        ok = ok && std::fscanf(in, "%d %d %d", &e.source_node_id, &e.target_node_id, &unc) == 3;
        e.uncertain = unc != 0;
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) ok = ok && std::fscanf(in, "%lf", &e.transformation(r, c)) == 1;
        for (int r = 0; r < 6; ++r)
          for (int c = 0; c < 6; ++c) ok = ok && std::fscanf(in, "%lf", &e.information(r, c)) == 1;
      }
      std::fclose(in);
      if (!ok) return 2;
      const teaser::GlobalOptimizationResult res = optimizer.globalOptimization(g, lm, cr, op, 64);
      size_t gone = 0;
      for (bool p : res.pruned) gone += p;
      if (g.edges.size() + gone != (size_t)m) return 1;  // the in-place call removed exactly the pruned edges
      FILE* out = std::fopen(argv[2], "w");
      if (!out) return 2;
      const teaser_posegraph_result_c& rec = res.record;
      std::fprintf(out, "%d %d %d %d %d %.17g %.17g %.17g %.17g\n", rec.status, rec.iterations[0], rec.iterations[1],
                   rec.trials[0], rec.trials[1], rec.F0, rec.F, rec.mu[0], rec.mu[1]);
      for (const auto& node : g.nodes) {
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) std::fprintf(out, "%.17g ", node.pose(r, c));
        std::fprintf(out, "\n");
      }
      for (int k = 0; k < m; ++k) std::fprintf(out, "%.17g %d\n", res.confidence[(size_t)k], (int)res.pruned[(size_t)k]);
      std::fprintf(out, "%zu\n", res.trace.size());
      for (const auto& t : res.trace)
        std::fprintf(out, "%d %.17g %.17g %.17g %d %d\n", t.pass, t.lam, t.rho, t.F_new, t.accepted, t.factorised);
      std::fclose(out);
      return 0;
    }
    // three nodes on the x axis, edges 1 -> 0 and 2 -> 1 that each measure a shift of 1; node 2 starts 0.3 off
    teaser::PoseGraph g;
    g.nodes.resize(3);
    for (int i = 0; i < 3; ++i) g.nodes[(size_t)i].pose(0, 3) = (double)i;
    g.nodes[2].pose(1, 3) = 0.3;
    for (int i = 0; i < 2; ++i) {
      teaser::PoseGraphEdge e;
      e.source_node_id = i + 1;
      e.target_node_id = i;
      e.transformation(0, 3) = 1.0;
      g.edges.push_back(e);
    }
    const teaser::GlobalOptimizationResult res = teaser::globalOptimization(g);
    bool ok = res.record.F0 > 0.08 && res.record.F < 1e-6 && g.edges.size() == 2 && res.record.iterations[0] >= 1;
    for (int i = 0; i < 3; ++i)
      ok = ok && std::fabs(g.nodes[(size_t)i].pose(0, 3) - i) < 1e-3 && std::fabs(g.nodes[(size_t)i].pose(1, 3)) < 1e-3;
    bool threw = false;
    try {
      teaser::globalOptimization(g, teaser::GlobalOptimizationGaussNewton());
    } catch (const std::logic_error&) {
      threw = true;
    }
    std::printf("F0 %.3g F %.3g status %d iterations %d\n", res.record.F0, res.record.F, res.record.status,
                res.record.iterations[0]);
    return ok && threw ? 0 : 1;
  } catch (const teaser::PoseGraphError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return std::string(e.what()).find("status 3") != std::string::npos ? 77 : 1;
  }
}
