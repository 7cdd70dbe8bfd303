// teaser/posegraph.h -- pose-graph optimisation on the GPU with the surface of open3d::pipelines::registration:
// PoseGraph, PoseGraphNode, PoseGraphEdge, GlobalOptimizationOption, GlobalOptimizationConvergenceCriteria,
// GlobalOptimizationLevenbergMarquardt and GlobalOptimization.  The arithmetic is written out in include/teaser_hip.h,
// "Pose-graph optimisation"; a call optimises every graph it is given in one launch, a workgroup per graph.
// Header-only over the C ABI; there is no CPU path (no MI355X: PoseGraphError with TEASER_HIP_ERR_NO_DEVICE).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "teaser/handle.h"
#include "teaser/icp.h"
#include "teaser_hip.h"

namespace teaser {

struct PoseGraphNode {
  Matrix4 pose = Matrix4::Identity();
};

// transformation aligns the source node's cloud to the target node's; information is the matrix of
// getInformationMatrixFromPointClouds (rotation block first).
struct PoseGraphEdge {
  int source_node_id = -1;
  int target_node_id = -1;
  Matrix4 transformation = Matrix4::Identity();
  Matrix6 information = identity6();
  bool uncertain = false;
  double confidence = 1.0;
  static Matrix6 identity6() {
    Matrix6 m;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) m(r, c) = r == c ? 1.0 : 0.0;
    return m;
  }
};

struct PoseGraph {
  std::vector<PoseGraphNode> nodes;
  std::vector<PoseGraphEdge> edges;
};

struct GlobalOptimizationOption {
  double max_correspondence_distance = 0.03;
  double edge_prune_threshold = 0.25;
  double preference_loop_closure = 1.0;
  int reference_node = -1;
};

struct GlobalOptimizationConvergenceCriteria {
  int max_iteration = 100;
  double min_relative_increment = 1e-6;
  double min_relative_residual_increment = 1e-6;
  double min_right_term = 1e-6;
  double min_residual = 1e-6;
  int max_iteration_lm = 20;
  double upper_scale_factor = 2.0 / 3.0;
  double lower_scale_factor = 1.0 / 3.0;
};

struct GlobalOptimizationMethod {
  virtual ~GlobalOptimizationMethod() = default;
  virtual bool implemented() const = 0;
};
struct GlobalOptimizationLevenbergMarquardt : GlobalOptimizationMethod {
  bool implemented() const override { return true; }
};
// Named for the surface's sake: globalOptimization throws std::logic_error for it.
struct GlobalOptimizationGaussNewton : GlobalOptimizationMethod {
  bool implemented() const override { return false; }
};

class PoseGraphError : public std::runtime_error {
 public:
  PoseGraphError(int32_t status, const std::string& what) : std::runtime_error(what), status_(status) {}
  int32_t status() const { return status_; }

 private:
  int32_t status_;
};

// One graph's result (teaser_posegraph_result_c and the per-node / per-edge outputs).
struct GlobalOptimizationResult {
  std::vector<Matrix4> poses;
  std::vector<double> confidence;
  std::vector<bool> pruned;
  std::vector<teaser_posegraph_trace_c> trace;  // as many rows as the call was given room for
  teaser_posegraph_result_c record{};
};

class PoseGraphOptimizer {
 public:
  // Optimises every graph in one call; the graphs are not changed.  trace_rows: room for that many trial rows per graph.
  std::vector<GlobalOptimizationResult> globalOptimizationBatch(
      const std::vector<const PoseGraph*>& graphs, const GlobalOptimizationMethod& method,
      const std::vector<GlobalOptimizationConvergenceCriteria>& criteria,
      const std::vector<GlobalOptimizationOption>& option, int trace_rows = 0) {
    if (!method.implemented())
      throw std::logic_error("globalOptimization implements GlobalOptimizationLevenbergMarquardt only");
    const size_t B = graphs.size();
    if ((criteria.size() != 1 && criteria.size() != B) || (option.size() != 1 && option.size() != B))
      throw std::invalid_argument("globalOptimizationBatch: one criteria / option, or one per graph");
    if (trace_rows < 0) throw std::invalid_argument("globalOptimizationBatch: trace_rows must be >= 0");
    std::vector<int32_t> n(B), m(B), src, tgt, cap(B, trace_rows);
    std::vector<double> poses, X, L;
    std::vector<uint8_t> unc;
    std::vector<teaser_posegraph_option_c> opts(B);
    for (size_t b = 0; b < B; ++b) {
      const PoseGraph& g = *graphs[b];
      n[b] = (int32_t)g.nodes.size();
      m[b] = (int32_t)g.edges.size();
      for (const PoseGraphNode& node : g.nodes)
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) poses.push_back(node.pose(r, c));
      for (const PoseGraphEdge& e : g.edges) {
        src.push_back(e.source_node_id);
        tgt.push_back(e.target_node_id);
        unc.push_back(e.uncertain ? 1 : 0);
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) X.push_back(e.transformation(r, c));
        for (int r = 0; r < 6; ++r)
          for (int c = 0; c < 6; ++c) L.push_back(e.information(r, c));
      }
      const GlobalOptimizationConvergenceCriteria& cr = criteria[criteria.size() == 1 ? 0 : b];
      const GlobalOptimizationOption& op = option[option.size() == 1 ? 0 : b];
      teaser_posegraph_option_c& o = opts[b];
      teaser_hip_posegraph_option_default(&o);
      o.max_iteration = cr.max_iteration;
      o.max_iteration_lm = cr.max_iteration_lm;
      o.min_relative_increment = cr.min_relative_increment;
      o.min_relative_residual_increment = cr.min_relative_residual_increment;
      o.min_right_term = cr.min_right_term;
      o.min_residual = cr.min_residual;
      o.upper_scale_factor = cr.upper_scale_factor;
      o.lower_scale_factor = cr.lower_scale_factor;
      o.max_correspondence_distance = op.max_correspondence_distance;
      o.edge_prune_threshold = op.edge_prune_threshold;
      o.preference_loop_closure = op.preference_loop_closure;
      o.reference_node = op.reference_node;
    }
    std::vector<GlobalOptimizationResult> out(B);
    if (B == 0) return out;
    h_.create("PoseGraphOptimizer");
    std::vector<double> poses_out(poses.size() + 1), conf(src.size() + 1);
    std::vector<uint8_t> pruned(src.size() + 1);
    std::vector<teaser_posegraph_result_c> rec(B);
    std::vector<teaser_posegraph_trace_c> rows((size_t)trace_rows * B + 1);
    const int32_t rc = teaser_hip_posegraph_optimize_batch(
        h_, (int32_t)B, n.data(), poses.data(), m.data(), src.data(), tgt.data(), X.data(), L.data(), unc.data(),
        opts.data(), poses_out.data(), conf.data(), pruned.data(), rec.data(), trace_rows ? rows.data() : nullptr,
        cap.data());
    if (rc != TEASER_HIP_OK)
      throw PoseGraphError(rc, std::string("globalOptimization: ") + teaser_hip_posegraph_last_error(h_));
    size_t no = 0, mo = 0;
    for (size_t b = 0; b < B; ++b) {
      GlobalOptimizationResult& r = out[b];
      r.record = rec[b];
      r.poses.resize((size_t)n[b]);
      for (int i = 0; i < n[b]; ++i)
        for (int rr = 0; rr < 4; ++rr)
          for (int c = 0; c < 4; ++c) r.poses[(size_t)i](rr, c) = poses_out[16 * (no + i) + 4 * rr + c];
      r.confidence.assign(conf.begin() + mo, conf.begin() + mo + m[b]);
      r.pruned.resize((size_t)m[b]);
      for (int k = 0; k < m[b]; ++k) r.pruned[(size_t)k] = pruned[mo + k] != 0;
      const int kept = rec[b].n_trace < trace_rows ? rec[b].n_trace : trace_rows;
      r.trace.assign(rows.begin() + (size_t)trace_rows * b, rows.begin() + (size_t)trace_rows * b + kept);
      no += (size_t)n[b];
      mo += (size_t)m[b];
    }
    return out;
  }

  // Open3D's GlobalOptimization: works IN PLACE -- the node poses are replaced, every edge's confidence is set, and
  // the edges pruned after the first pass are removed.
  GlobalOptimizationResult globalOptimization(PoseGraph& graph, const GlobalOptimizationMethod& method,
                                              const GlobalOptimizationConvergenceCriteria& criteria,
                                              const GlobalOptimizationOption& option, int trace_rows = 0) {
    GlobalOptimizationResult r = globalOptimizationBatch({&graph}, method, {criteria}, {option}, trace_rows)[0];
    for (size_t i = 0; i < graph.nodes.size(); ++i) graph.nodes[i].pose = r.poses[i];
    std::vector<PoseGraphEdge> kept;
    for (size_t k = 0; k < graph.edges.size(); ++k) {
      graph.edges[k].confidence = r.confidence[k];
      if (!r.pruned[k]) kept.push_back(graph.edges[k]);
    }
    graph.edges.swap(kept);
    return r;
  }

 private:
  detail::LazyPoseGraph h_;
};

// The free functions, on an optimizer of their own (a handle per call: keep a PoseGraphOptimizer for repeated use).
inline GlobalOptimizationResult globalOptimization(
    PoseGraph& graph, const GlobalOptimizationMethod& method = GlobalOptimizationLevenbergMarquardt(),
    const GlobalOptimizationConvergenceCriteria& criteria = GlobalOptimizationConvergenceCriteria(),
    const GlobalOptimizationOption& option = GlobalOptimizationOption()) {
  PoseGraphOptimizer opt;
  return opt.globalOptimization(graph, method, criteria, option);
}

inline std::vector<GlobalOptimizationResult> globalOptimizationBatch(
    const std::vector<PoseGraph>& graphs, const GlobalOptimizationMethod& method = GlobalOptimizationLevenbergMarquardt(),
    const GlobalOptimizationConvergenceCriteria& criteria = GlobalOptimizationConvergenceCriteria(),
    const GlobalOptimizationOption& option = GlobalOptimizationOption()) {
  PoseGraphOptimizer opt;
  std::vector<const PoseGraph*> ptrs;
  for (const PoseGraph& g : graphs) ptrs.push_back(&g);
  return opt.globalOptimizationBatch(ptrs, method, {criteria}, {option});
}

}  // namespace teaser
