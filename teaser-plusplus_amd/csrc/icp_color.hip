// icp_color.hip -- host side of Colored ICP on the ICP handle (include/teaser_hip.h, "ICP refinement: Colored ICP"):
// the entry points that take colours (teaser_hip_icp_batch_color, _solve_color), the colour-gradient call
// (teaser_hip_icp_color_gradients_batch) and the gradient stage both run.
// Kernels: icp_color_gradient_kernel (kernels_icp_color.hip), icp_corr_kernel<3> / icp_finalize_kernel<3>
// (kernels_icp.hip); design in DESIGN.md section 22.
//
// The iterations are icp_run_batch's (icp.hip).  What a coloured call adds arrives through its pre-index hook: the
// colours reduced to one intensity per point and uploaded, the per-problem records, and -- for the coloured problems
// that give no gradients -- the index over the target with the gradient radius and the gradient kernel, which writes
// into the records the correspondence pass gathers from.  icp_run_batch reaches the mode-3 launcher through the
// function it is handed (color_iterate), so icp.hip names no launcher of this file's kernels.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_common.h"
#include "icp_host.h"
#include "icp_internal.h"
#include "teaser_hip.h"

using namespace thip;

static_assert(sizeof(teaser_icp_color_c) == 24, "the header states the record's size");

namespace {

inline double intensity(const double* c) { return ((c[0] + c[1]) + c[2]) / 3.0; }

inline bool good_radius(double r) { return std::isfinite(r) && r > 0 && std::isfinite(r * r) && r * r > 0; }

// The descriptors of one gradient pass: per cloud an IcpDesc with the grid of the gradient radius and an IcpGradDesc;
// a cloud that takes no part has n_t = 0 and no blocks.
struct GradPlan {
  IcpIndex ix;
  std::vector<IcpGradDesc> gd;
  std::vector<int32_t> blk;
  int top_nn = 0;
};

// Appends cloud b (n points at points[b]; n = 0: takes no part).  t_off < 0: the clouds are packed one after the other;
// else the cloud's first point in the caller's own packing of B_Q, B_NORMALS and B_COLOR_T.
void plan_cloud(GradPlan& P, int b, int32_t n, const double* const* points, double radius, int32_t max_nn,
                int64_t t_off) {
  IcpDesc& d = add_problem(P.ix, b, 0, n, points, n > 0 ? radius : 1.0, 0);
  if (t_off >= 0) d.t_off = t_off;
  d.blk_off = (int32_t)P.blk.size();
  d.nblk = (n + kIcpCovBlock - 1) / kIcpCovBlock;
  for (int k = 0; k < d.nblk; ++k) P.blk.push_back(b);
  IcpGradDesc g = {n > 0 ? max_nn : 0, 0};
  P.gd.push_back(g);
  if (n > 0) P.top_nn = std::max(P.top_nn, max_nn);
}

// Uploads the plan's descriptors and block maps (B_N*), builds the index over the points in B_Q (packed at the
// descriptors' t_off) and enqueues the gradient kernel: normals from B_NORMALS, intensities from and gradients into
// B_COLOR_T.  The index buffers (B_TBUCKET .. B_QJ) must have been sized by the caller.
int32_t launch_gradients(teaser_hip_icp* h, const GradPlan& P) {
  if (P.blk.empty()) return TEASER_HIP_OK;
  const size_t batch = P.ix.desc.size();
  DevBuf* B = h->buf;
  hipStream_t s = h->stream;
  const struct {
    int buf;
    const void* src;
    size_t n;
  } copies[] = {{B_NDESC, P.ix.desc.data(), sizeof(IcpDesc) * batch},
                {B_NREC, P.gd.data(), sizeof(IcpGradDesc) * batch},
                {B_NBLK, P.blk.data(), sizeof(int32_t) * P.blk.size()},
                {B_NTBLK, P.ix.tblk_prob.data(), sizeof(int32_t) * P.ix.tblk_prob.size()}};
  for (const auto& c : copies) {
    if (!B[c.buf].ensure(std::max<size_t>(c.n, 1))) return fail(h, TEASER_HIP_ERR_OOM, "hipMalloc failed (colour gradients)");
    if (c.n) FCHK(h, hipMemcpyAsync(B[c.buf].p, c.src, c.n, hipMemcpyHostToDevice, s), "hipMemcpyAsync (colour gradients)");
  }
  if (P.ix.b_off) FCHK(h, hipMemsetAsync(B[B_BCOUNT].p, 0, sizeof(int32_t) * P.ix.b_off, s), "hipMemsetAsync");
  const IcpDesc* desc = B[B_NDESC].as<IcpDesc>();
  launch_icp_index(s, desc, B[B_NTBLK].as<int32_t>(), (int)P.ix.tblk_prob.size(), (int)batch, B[B_Q].as<double>(),
                   B[B_TBUCKET].as<int32_t>(), B[B_BCOUNT].as<int32_t>(), B[B_BSTART].as<int32_t>(),
                   B[B_CURSOR].as<int32_t>(), B[B_QS].as<double>(), B[B_QJ].as<int32_t>());
  launch_icp_color_gradients(s, desc, B[B_NREC].as<IcpGradDesc>(), B[B_NBLK].as<int32_t>(), (int)P.blk.size(), P.top_nn,
                             B[B_Q].as<double>(), B[B_QS].as<double>(), B[B_QJ].as<int32_t>(),
                             B[B_BSTART].as<int32_t>(), B[B_NORMALS].as<double>(), B[B_COLOR_T].as<double>());
  FCHK(h, hipGetLastError(), "colour gradient kernel launch");
  return TEASER_HIP_OK;
}

// teaser_hip_icp_batch_color: the caller's arrays, for the hook (which runs behind icp_run_batch's checks), and what the
// hook uploads from: it has to outlive the copies, that is the call's synchronisations
struct ColorCtx {
  const double* const* dst;
  const teaser_icp_params_c* params;
  const double* const* src_colors;
  const double* const* dst_colors;
  const double* const* dst_gradients;
  const teaser_icp_color_c* color;
  std::vector<IcpColorDesc> cd;
  GradPlan plan;
};

teaser_icp_color_c color_record(const ColorCtx& C, int b) {
  teaser_icp_color_c r;
  teaser_hip_icp_color_default(&r);
  return C.color ? C.color[b] : r;
}

double gradient_radius(const teaser_icp_color_c& r, double max_correspondence_distance) {
  return r.gradient_radius <= 0 ? 2.0 * max_correspondence_distance : r.gradient_radius;
}

int32_t color_hook(teaser_hip_icp* h, void* ctx, const IcpIndex& ix) {
  ColorCtx& C = *static_cast<ColorCtx*>(ctx);
  const int batch = (int)ix.desc.size();
  DevBuf* B = h->buf;
  hipStream_t s = h->stream;
  // the records, one intensity per source point, {gradient, intensity} per target point; rows of problems of the other
  // methods are never read
  std::vector<IcpColorDesc>& cd = C.cd;
  cd.assign((size_t)batch, IcpColorDesc());
  const size_t n_s = (size_t)ix.s_off, n_t = (size_t)ix.t_off;
  h->cstage.assign(n_s + 4 * n_t, 0.0);
  double* is = h->cstage.data();
  double* rt = is + n_s;
  GradPlan& P = C.plan;
  P = GradPlan();
  for (int b = 0; b < batch; ++b) {
    const IcpDesc& d = ix.desc[(size_t)b];
    cd[(size_t)b].sg = cd[(size_t)b].sp = 0.0;
    if (d.method != kIcpMethodColor) {
      plan_cloud(P, b, 0, C.dst, 1.0, 0, d.t_off);
      continue;
    }
    const teaser_icp_color_c r = color_record(C, b);
    cd[(size_t)b].sg = sqrt(r.lambda_geometric);
    cd[(size_t)b].sp = sqrt(1.0 - r.lambda_geometric);
    for (int64_t i = 0; i < d.n_s; ++i) is[d.s_off + i] = intensity(C.src_colors[b] + 3 * i);
    const double* g = C.dst_gradients ? C.dst_gradients[b] : nullptr;
    for (int64_t j = 0; j < d.n_t; ++j) {
      double* o = rt + 4 * (d.t_off + j);
      if (g) o[0] = g[3 * j], o[1] = g[3 * j + 1], o[2] = g[3 * j + 2];
      o[3] = intensity(C.dst_colors[b] + 3 * j);
    }
    plan_cloud(P, b, g ? 0 : d.n_t, C.dst, gradient_radius(r, C.params[b].max_correspondence_distance),
               r.gradient_max_nn, d.t_off);
  }
  const struct {
    int buf;
    const void* src;
    size_t n;
  } copies[] = {{B_COLOR_DESC, cd.data(), sizeof(IcpColorDesc) * cd.size()},
                {B_COLOR_S, is, sizeof(double) * n_s},
                {B_COLOR_T, rt, sizeof(double) * 4 * n_t}};
  for (const auto& c : copies) {
    if (!B[c.buf].ensure(std::max<size_t>(c.n, 8))) return fail(h, TEASER_HIP_ERR_OOM, "hipMalloc failed (colours)");
    if (c.n) FCHK(h, hipMemcpyAsync(B[c.buf].p, c.src, c.n, hipMemcpyHostToDevice, s), "hipMemcpyAsync (colours)");
  }
  return launch_gradients(h, P);
}

void color_iterate(teaser_hip_icp* h, void*, int n_blk, int batch) {
  DevBuf* B = h->buf;
  const IcpColorArgs col = {B[B_COLOR_DESC].as<IcpColorDesc>(), B[B_COLOR_T].as<double>(), B[B_COLOR_S].as<double>()};
  launch_icp_iteration_color(h->stream, B[B_DESC].as<IcpDesc>(), B[B_STATE].as<IcpState>(), B[B_BLK].as<int32_t>(),
                             n_blk, batch, B[B_X].as<double>(), B[B_QS].as<double>(), B[B_QJ].as<int32_t>(),
                             B[B_BSTART].as<int32_t>(), B[B_NORMALS].as<double>(), B[B_COV_S].as<double>(),
                             B[B_COV_T].as<double>(), B[B_MATCH].as<int32_t>(), B[B_PARTIALS].as<double>(), col);
}

int32_t check_max_nn(teaser_hip_icp* h, int32_t max_nn, const char* arg, int b) {
  if (max_nn < 4 || max_nn > kIcpCovMaxNN)
    return fail(h, TEASER_HIP_ERR_BAD_ARG,
                std::string(arg) + " must lie in [4, " + std::to_string(kIcpCovMaxNN) + "]" + at(b));
  return TEASER_HIP_OK;
}

}  // namespace

extern "C" {

int32_t teaser_hip_icp_color_default(teaser_icp_color_c* color) {
  if (!color) return TEASER_HIP_ERR_BAD_ARG;
  color->lambda_geometric = 0.968;  // Open3D's TransformationEstimationForColoredICP
  color->gradient_radius = 0.0;     // 2 max_correspondence_distance
  color->gradient_max_nn = 30;
  color->reserved = 0;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_icp_batch_color(teaser_hip_icp* h, int32_t batch, const double* const* src, const int32_t* n_src,
                                   const double* const* dst, const int32_t* n_dst, const double* init,
                                   const teaser_icp_params_c* params, teaser_icp_result_c* out, int32_t* const* corr,
                                   const double* const* dst_normals, const teaser_icp_estimation_c* est,
                                   const double* const* src_cov, const double* const* dst_cov,
                                   const double* const* src_colors, const double* const* dst_colors,
                                   const double* const* dst_gradients, const teaser_icp_color_c* color) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  // What only a coloured problem has is checked here; the counts these checks read are used only where they are
  // valid, everything else is icp_run_batch's to refuse.
  bool any = false;
  if (est && n_src && n_dst && params)
    for (int b = 0; b < batch; ++b) {
      if (est[b].method != kIcpMethodColor) continue;
      any = true;
      teaser_icp_color_c r;
      teaser_hip_icp_color_default(&r);
      if (color) r = color[b];
      if (!std::isfinite(r.lambda_geometric) || r.lambda_geometric < 0 || r.lambda_geometric > 1)
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "color: lambda_geometric must lie in [0, 1]" + at(b));
      const int32_t rc = check_max_nn(h, r.gradient_max_nn, "color: gradient_max_nn", b);
      if (rc != TEASER_HIP_OK) return rc;
      if (r.reserved != 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "color: reserved must be 0" + at(b));
      const double mcd = params[b].max_correspondence_distance;
      if (good_radius(mcd) && !good_radius(gradient_radius(r, mcd)))
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "color: gradient_radius (and its square) must be finite and > 0" + at(b));
      if (n_src[b] > 0) {
        if (!src_colors || !src_colors[b])
          return fail(h, TEASER_HIP_ERR_BAD_ARG, "src_colors is NULL for a Colored-ICP problem" + at(b));
        if (!finite_points(src_colors[b], n_src[b]))
          return fail(h, TEASER_HIP_ERR_BAD_ARG, "src_colors has a non-finite component" + at(b));
      }
      if (n_dst[b] > 0) {
        if (!dst_colors || !dst_colors[b])
          return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst_colors is NULL for a Colored-ICP problem" + at(b));
        if (!finite_points(dst_colors[b], n_dst[b]))
          return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst_colors has a non-finite component" + at(b));
        if (dst_gradients && dst_gradients[b] && !finite_points(dst_gradients[b], n_dst[b]))
          return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst_gradients has a non-finite component" + at(b));
      }
    }
  if (!any)  // methods 0 - 2 only: the call teaser_hip_icp_batch_cov makes
    return icp_run_batch(h, batch, src, n_src, dst, n_dst, init, params, out, corr, dst_normals, est, src_cov, dst_cov,
                         kIcpMethodColor, nullptr, nullptr, nullptr);
  ColorCtx C = {dst, params, src_colors, dst_colors, dst_gradients, color, {}, {}};
  return icp_run_batch(h, batch, src, n_src, dst, n_dst, init, params, out, corr, dst_normals, est, src_cov, dst_cov,
                       kIcpMethodColor, nullptr, color_hook, &C, color_iterate);
}

int32_t teaser_hip_icp_solve_color(teaser_hip_icp* h, const double* src, int32_t n_src, const double* dst,
                                   int32_t n_dst, const double* init, const teaser_icp_params_c* params,
                                   teaser_icp_result_c* out, int32_t* corr, const double* dst_normals,
                                   const teaser_icp_estimation_c* est, const double* src_cov, const double* dst_cov,
                                   const double* src_colors, const double* dst_colors, const double* dst_gradients,
                                   const teaser_icp_color_c* color) {
  int32_t* const corrs[1] = {corr};
  return teaser_hip_icp_batch_color(h, 1, &src, &n_src, &dst, &n_dst, init, params, out, corrs,
                                    dst_normals ? &dst_normals : nullptr, est, src_cov ? &src_cov : nullptr,
                                    dst_cov ? &dst_cov : nullptr, src_colors ? &src_colors : nullptr,
                                    dst_colors ? &dst_colors : nullptr, dst_gradients ? &dst_gradients : nullptr, color);
}

int32_t teaser_hip_icp_color_gradients_batch(teaser_hip_icp* h, int32_t batch, const double* const* points,
                                             const int32_t* n, const double* const* normals,
                                             const double* const* colors, const double* radius, const int32_t* max_nn,
                                             double* const* out) {
  const CallStart c = begin_cloud_call(h, batch, points, n, false);
  if (c.done) return c.rc;
  if (!radius) return fail(h, TEASER_HIP_ERR_BAD_ARG, "radius must not be NULL");
  if (!max_nn) return fail(h, TEASER_HIP_ERR_BAD_ARG, "max_nn must not be NULL");
  for (int b = 0; b < batch; ++b) {
    if (!good_radius(radius[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "radius (and its square) must be finite and > 0" + at(b));
    const int32_t rc = check_max_nn(h, max_nn[b], "max_nn", b);
    if (rc != TEASER_HIP_OK) return rc;
    if (n[b] == 0) continue;
    if (!normals || !normals[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "normals is NULL" + at(b));
    if (!colors || !colors[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "colors is NULL" + at(b));
    if (!out || !out[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "out is NULL" + at(b));
    if (!finite_points(normals[b], n[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "normals has a non-finite component" + at(b));
    if (!finite_points(colors[b], n[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "colors has a non-finite component" + at(b));
  }
  if (c.total == 0) return TEASER_HIP_OK;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");

  GradPlan P;
  for (int b = 0; b < batch; ++b) plan_cloud(P, b, n[b], points, radius[b], max_nn[b], -1);
  const int64_t t_off = P.ix.t_off;
  size_t bytes[B_COUNT] = {};
  index_bytes(P.ix, 0, false, bytes);
  bytes[B_DESC] = bytes[B_TBLK] = bytes[B_BLK] = 0;  // launch_gradients keeps the descriptors and the block maps in B_N*
  bytes[B_NORMALS] = sizeof(double) * 3 * t_off;
  bytes[B_COLOR_T] = sizeof(double) * 4 * t_off;
  int32_t rc = ensure_buffers(h, bytes, "hipMalloc failed (colour gradient buffers)");
  if (rc != TEASER_HIP_OK) return rc;
  DevBuf* B = h->buf;
  hipStream_t s = h->stream;
  h->stage.resize((size_t)(3 * t_off));
  if ((rc = upload_points(h, batch, points, n, 0, "hipMemcpyAsync (points)")) != TEASER_HIP_OK) return rc;
  h->cstage.assign((size_t)(4 * t_off), 0.0);
  for (int b = 0; b < batch; ++b) {
    const IcpDesc& d = P.ix.desc[(size_t)b];
    if (d.n_t == 0) continue;
    FCHK(h, hipMemcpyAsync(B[B_NORMALS].as<double>() + 3 * d.t_off, normals[b], 24 * (size_t)d.n_t,
                           hipMemcpyHostToDevice, s),
         "hipMemcpyAsync (normals)");
    for (int64_t j = 0; j < d.n_t; ++j) h->cstage[(size_t)(4 * (d.t_off + j) + 3)] = intensity(colors[b] + 3 * j);
  }
  FCHK(h, hipMemcpyAsync(B[B_COLOR_T].p, h->cstage.data(), bytes[B_COLOR_T], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (intensities)");
  if ((rc = launch_gradients(h, P)) != TEASER_HIP_OK) return rc;
  FCHK(h, hipMemcpyAsync(h->cstage.data(), B[B_COLOR_T].p, bytes[B_COLOR_T], hipMemcpyDeviceToHost, s),
       "hipMemcpyAsync (gradients)");
  FCHK(h, hipStreamSynchronize(s), "colour gradients");
  for (int b = 0; b < batch; ++b) {
    const IcpDesc& d = P.ix.desc[(size_t)b];
    for (int64_t j = 0; j < d.n_t; ++j)
      for (int k = 0; k < 3; ++k) out[b][3 * j + k] = h->cstage[(size_t)(4 * (d.t_off + j) + k)];
  }
  return TEASER_HIP_OK;
}

}  // extern "C"
