// icp.hip -- host side of the batched ICP (include/teaser_hip.h, "ICP refinement": point-to-point, point-to-plane
// with robust kernels, Generalized ICP, Colored ICP) and of the covariance estimation on the same handle: argument validation,
// the per-call index and the iteration loop.  The handle's other calls: icp_outlier.hip, icp_normals.hip,
// icp_keypoints.hip, icp_color.hip (the Colored-ICP entry points and their checks); what they share: icp_host.h.
// Kernels: kernels_icp.hip.
//
// The host enqueues iterations in groups of kIcpGroup (two launches each); after a group ONE small copy of the
// number of unfinished problems decides whether another group follows.  There is no host round trip inside a group:
// a problem that finishes mid-group makes its remaining launches return at once.
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

namespace {

constexpr int kIcpGroup = 8;
static_assert(kIcpCovMaxNN == TEASER_HIP_ICP_COV_MAX_NN, "the header states K");
static_assert(kIcpKnnMax == TEASER_HIP_ICP_KNN_MAX, "the header states the largest k");

// the six entries of the contract (upper triangle) of n row-major 3 x 3 matrices
bool finite_cov(const double* c, int64_t n) {
  static const int kUpper[6] = {0, 1, 2, 4, 5, 8};
  for (int64_t k = 0; k < n; ++k)
    for (int u : kUpper)
      if (!std::isfinite(c[9 * k + u])) return false;
  return true;
}

void pack_cov(const double* c, int64_t n, double* out) {
  static const int kUpper[6] = {0, 1, 2, 4, 5, 8};
  for (int64_t k = 0; k < n; ++k)
    for (int u = 0; u < 6; ++u) out[6 * k + u] = c[9 * k + kUpper[u]];
}

int32_t validate(teaser_hip_icp* h, int32_t batch, const double* const* src, const int32_t* n_src,
                 const double* const* dst, const int32_t* n_dst, const double* init,
                 const teaser_icp_params_c* params, teaser_icp_result_c* out, const double* const* dst_normals,
                 const teaser_icp_estimation_c* est, const double* const* src_cov, const double* const* dst_cov,
                 int max_method, const teaser_icp_normal_search_c* nsearch) {
  if (batch < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0");
  if (batch == 0) return TEASER_HIP_OK;
  if (!n_src || !n_dst) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src / n_dst must not be NULL");
  if (!params) return fail(h, TEASER_HIP_ERR_BAD_ARG, "params must not be NULL");
  if (!out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "out must not be NULL");
  int64_t total_s = 0, total_t = 0;
  for (int b = 0; b < batch; ++b) {
    const teaser_icp_params_c& p = params[b];
    const double r = p.max_correspondence_distance;
    if (!std::isfinite(r) || !(r > 0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "max_correspondence_distance must be finite and > 0" + at(b));
    if (!std::isfinite(r * r) || !(r * r > 0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "max_correspondence_distance squared must be finite and > 0" + at(b));
    if (p.max_iteration < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "max_iteration must be >= 0" + at(b));
    if (!std::isfinite(p.relative_fitness) || p.relative_fitness < 0)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "relative_fitness must be finite and >= 0" + at(b));
    if (!std::isfinite(p.relative_rmse) || p.relative_rmse < 0)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "relative_rmse must be finite and >= 0" + at(b));
    if (n_src[b] < 0 || n_dst[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src / n_dst must be >= 0" + at(b));
    if (n_src[b] > 0 && (!src || !src[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "src is NULL" + at(b));
    if (n_dst[b] > 0 && (!dst || !dst[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst is NULL" + at(b));
    if (n_src[b] > 0 && !finite_points(src[b], n_src[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "src has a non-finite coordinate" + at(b));
    if (n_dst[b] > 0 && !finite_points(dst[b], n_dst[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst has a non-finite coordinate" + at(b));
    if (init) {
      const double* T = init + 16 * (int64_t)b;
      for (int k = 0; k < 16; ++k)
        if (!std::isfinite(T[k])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "init is not finite" + at(b));
      if (T[12] != 0 || T[13] != 0 || T[14] != 0 || T[15] != 1)
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "init: last row must be 0 0 0 1" + at(b));
    }
    if (est) {
      const teaser_icp_estimation_c& m = est[b];
      if (m.method < kIcpMethodPoint || m.method > max_method)
        return fail(h, TEASER_HIP_ERR_BAD_ARG,
                    (m.method == kIcpMethodGicp    ? "est: method 2 (Generalized ICP) needs the _cov entry points"
                     : m.method == kIcpMethodColor ? "est: method 3 (Colored ICP) needs the _color entry points"
                                                   : "est: unknown method") + at(b));
      if (m.kernel < kIcpKernelL2 || m.kernel > kIcpKernelTukey)
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "est: unknown kernel" + at(b));
      if (m.method == kIcpMethodPoint && m.kernel != kIcpKernelL2)
        return fail(h, TEASER_HIP_ERR_BAD_ARG,
                    "est: a kernel other than L2 needs point-to-plane (kernel given with point-to-point)" + at(b));
      if (m.kernel != kIcpKernelL2 && (!std::isfinite(m.kernel_k) || !(m.kernel_k > 0)))
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "est: kernel_k must be finite and > 0" + at(b));
      if (m.method == kIcpMethodGicp) {
        if (m.kernel != kIcpKernelL2)
          return fail(h, TEASER_HIP_ERR_BAD_ARG, "est: Generalized ICP takes the L2 kernel only" + at(b));
        if (n_src[b] > 0) {
          if (!src_cov || !src_cov[b])
            return fail(h, TEASER_HIP_ERR_BAD_ARG, "src_cov is NULL for a Generalized-ICP problem" + at(b));
          if (!finite_cov(src_cov[b], n_src[b]))
            return fail(h, TEASER_HIP_ERR_BAD_ARG, "src_cov has a non-finite entry" + at(b));
        }
        if (n_dst[b] > 0) {
          if (!dst_cov || !dst_cov[b])
            return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst_cov is NULL for a Generalized-ICP problem" + at(b));
          if (!finite_cov(dst_cov[b], n_dst[b]))
            return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst_cov has a non-finite entry" + at(b));
        }
      }
      const bool estimated = nsearch && nsearch[b].max_nn != 0 && !(dst_normals && dst_normals[b]);
      if (m.method == kIcpMethodColor && n_dst[b] > 0) {
        if (!dst_normals || !dst_normals[b])
          return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst_normals is NULL for a Colored-ICP problem" + at(b));
        if (!finite_points(dst_normals[b], n_dst[b]))
          return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst_normals has a non-finite component" + at(b));
      }
      if (m.method == kIcpMethodPlane && n_dst[b] > 0 && !estimated) {
        if (!dst_normals || !dst_normals[b])
          return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst_normals is NULL for a point-to-plane problem" + at(b));
        if (!finite_points(dst_normals[b], n_dst[b]))
          return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst_normals has a non-finite component" + at(b));
      }
    }
    total_s += n_src[b];
    total_t += n_dst[b];
  }
  if (total_s >= INT32_MAX || total_t >= INT32_MAX / 2)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "too many points in one call");
  return TEASER_HIP_OK;
}

}  // namespace

extern "C" {

int32_t teaser_hip_icp_params_default(teaser_icp_params_c* p) {
  if (!p) return TEASER_HIP_ERR_BAD_ARG;
  p->max_correspondence_distance = 0;  // required argument of registration_icp
  p->max_iteration = 30;               // Open3D ICPConvergenceCriteria
  p->relative_fitness = 1e-6;
  p->relative_rmse = 1e-6;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_icp_create(int32_t device, teaser_hip_icp** out) {
  const int32_t rc = open_handle(device, out);
  if (rc == TEASER_HIP_OK && hipHostMalloc((void**)&(*out)->h_live, sizeof(int32_t)) != hipSuccess) {
    delete *out;
    *out = nullptr;
    return TEASER_HIP_ERR_HIP;
  }
  return rc;
}

int32_t teaser_hip_icp_destroy(teaser_hip_icp* h) { return close_handle(h); }

const char* teaser_hip_icp_last_error(const teaser_hip_icp* h) { return h ? h->err.c_str() : ""; }

int32_t teaser_hip_icp_fill_scratch(teaser_hip_icp* h, int32_t byte, int64_t* bytes_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  // every device buffer up to its capacity; the host staging up to its current size.  h_live's four bytes are staging
  // too: every iteration group copies the live count into them before it reads them.
  ScratchSpan spans[B_COUNT + 4];
  for (int k = 0; k < B_COUNT; ++k) spans[k] = span_of(h->buf[k]);
  spans[B_COUNT] = {h->stage.data(), sizeof(double) * h->stage.size(), false};
  spans[B_COUNT + 1] = {h->back.data(), sizeof(double) * h->back.size(), false};
  spans[B_COUNT + 2] = {h->cstage.data(), sizeof(double) * h->cstage.size(), false};
  spans[B_COUNT + 3] = {h->h_live, sizeof(int32_t), false};
  return fill_scratch(h, byte, spans, B_COUNT + 4, bytes_out);
}

int32_t teaser_hip_icp_estimation_default(teaser_icp_estimation_c* est) {
  if (!est) return TEASER_HIP_ERR_BAD_ARG;
  est->method = kIcpMethodPoint;
  est->kernel = kIcpKernelL2;
  est->kernel_k = 1.0;  // Open3D's default parameter of every robust kernel; ignored for L2
  return TEASER_HIP_OK;
}

int32_t teaser_hip_icp_batch(teaser_hip_icp* h, int32_t batch, const double* const* src, const int32_t* n_src,
                             const double* const* dst, const int32_t* n_dst, const double* init,
                             const teaser_icp_params_c* params, teaser_icp_result_c* out, int32_t* const* corr) {
  return teaser_hip_icp_batch_ex(h, batch, src, n_src, dst, n_dst, init, params, out, corr, nullptr, nullptr);
}

int32_t teaser_hip_icp_batch_ex(teaser_hip_icp* h, int32_t batch, const double* const* src, const int32_t* n_src,
                                const double* const* dst, const int32_t* n_dst, const double* init,
                                const teaser_icp_params_c* params, teaser_icp_result_c* out, int32_t* const* corr,
                                const double* const* dst_normals, const teaser_icp_estimation_c* est) {
  return icp_run_batch(h, batch, src, n_src, dst, n_dst, init, params, out, corr, dst_normals, est, nullptr, nullptr,
                       kIcpMethodPlane, nullptr, nullptr, nullptr);
}

int32_t teaser_hip_icp_batch_cov(teaser_hip_icp* h, int32_t batch, const double* const* src, const int32_t* n_src,
                                 const double* const* dst, const int32_t* n_dst, const double* init,
                                 const teaser_icp_params_c* params, teaser_icp_result_c* out, int32_t* const* corr,
                                 const double* const* dst_normals, const teaser_icp_estimation_c* est,
                                 const double* const* src_cov, const double* const* dst_cov) {
  return icp_run_batch(h, batch, src, n_src, dst, n_dst, init, params, out, corr, dst_normals, est, src_cov, dst_cov,
                       kIcpMethodGicp, nullptr, nullptr, nullptr);
}

}  // extern "C"

namespace thip {

// Every batched entry point (icp_host.h).
int32_t icp_run_batch(teaser_hip_icp* h, int32_t batch, const double* const* src, const int32_t* n_src,
                      const double* const* dst, const int32_t* n_dst, const double* init,
                      const teaser_icp_params_c* params, teaser_icp_result_c* out, int32_t* const* corr,
                      const double* const* dst_normals, const teaser_icp_estimation_c* est,
                      const double* const* src_cov, const double* const* dst_cov, int max_method,
                      const teaser_icp_normal_search_c* nsearch, IcpPreIndexHook hook, void* ctx,
                      IcpIterateFn iterate) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  int32_t rc = validate(h, batch, src, n_src, dst, n_dst, init, params, out, dst_normals, est, src_cov, dst_cov,
                        max_method, nsearch);
  if (rc != TEASER_HIP_OK || batch == 0) return rc;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");

  // ---- descriptors, block maps and initial state (host) ----
  IcpIndex ix;
  std::vector<IcpState> state((size_t)batch);
  int max_iter = 0;
  bool plane = false;  // any point-to-plane problem: the launches with the wider partials
  bool gicp = false;   // any Generalized-ICP problem: the third instantiation and the packed covariances
  bool color = false;  // any Colored-ICP problem: the fourth instantiation, reached through `iterate`
  for (int b = 0; b < batch; ++b) {
    const teaser_icp_params_c& p = params[b];
    IcpDesc& d = add_problem(ix, b, n_src[b], n_dst[b], dst, p.max_correspondence_distance,
                             (n_src[b] + kIcpBlock - 1) / kIcpBlock);
    d.rel_fitness = p.relative_fitness;
    d.rel_rmse = p.relative_rmse;
    d.max_iteration = p.max_iteration;
    max_iter = std::max(max_iter, p.max_iteration);
    if (est) {
      d.method = est[b].method;
      d.kernel = est[b].kernel;
      d.kernel_k = est[b].kernel == kIcpKernelL2 ? 0.0 : est[b].kernel_k;
      plane |= d.method == kIcpMethodPlane;
      gicp |= d.method == kIcpMethodGicp;
      color |= d.method == kIcpMethodColor;
    }
    IcpState& st = state[(size_t)b];
    memset(&st, 0, sizeof(st));
    static const double kEye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const double* T0 = init ? init + 16 * (int64_t)b : kEye;
    for (int k = 0; k < 16; ++k) st.T[k] = T0[k];
    for (int k = 0; k < 12; ++k) st.U[k] = T0[k];  // the first correspondence pass applies init to P
  }
  if (color && !iterate) return fail(h, TEASER_HIP_ERR_BAD_ARG, "est: method 3 (Colored ICP) needs the _color entry points");
  plane |= color;  // the normals and the wider partials
  const std::vector<IcpDesc>& desc = ix.desc;
  const int64_t s_off = ix.s_off, t_off = ix.t_off;
  const int n_blk = (int)ix.blk_prob.size();

  // ---- device buffers ----
  const size_t pts_s = (size_t)std::max<int64_t>(s_off, 1), pts_t = (size_t)std::max<int64_t>(t_off, 1);
  size_t bytes[B_COUNT] = {};
  index_bytes(ix, 1, hook != nullptr, bytes);  // (the hook's worklist)
  bytes[B_STATE] = sizeof(IcpState) * batch;
  bytes[B_X] = sizeof(double) * 3 * pts_s;
  bytes[B_MATCH] = std::max(bytes[B_MATCH], sizeof(int32_t) * pts_s);
  bytes[B_PARTIALS] = sizeof(double) * (plane || gicp ? kIcpPlaneSums : kIcpSums) * std::max(n_blk, 1);
  bytes[B_LIVE] = sizeof(int32_t);
  bytes[B_NORMALS] = plane ? sizeof(double) * 3 * pts_t : 0;
  bytes[B_COV_S] = gicp ? sizeof(double) * 6 * pts_s : 0;
  bytes[B_COV_T] = gicp ? sizeof(double) * 6 * pts_t : 0;
  if ((rc = ensure_buffers(h, bytes, "hipMalloc failed (ICP buffers)")) != TEASER_HIP_OK) return rc;
  hipStream_t s = h->stream;
  DevBuf* B = h->buf;

  h->stage.resize((size_t)((gicp ? 9 : 3) * (s_off + t_off)));  // points, then the packed covariances
  if ((rc = upload_inputs(h, ix, src, dst, n_dst, state.data(), bytes[B_STATE])) != TEASER_HIP_OK) return rc;
  for (int b = 0; b < batch; ++b) {  // one copy per point-to-plane problem, straight from the caller's normals
    const IcpDesc& d = desc[(size_t)b];
    if ((d.method == kIcpMethodPlane || d.method == kIcpMethodColor) && d.n_t > 0 && dst_normals &&
        dst_normals[b])  // else: the hook estimates them
      FCHK(h, hipMemcpyAsync(B[B_NORMALS].as<double>() + 3 * d.t_off, dst_normals[b], 24 * (size_t)d.n_t,
                             hipMemcpyHostToDevice, s),
           "hipMemcpyAsync (normals)");
  }
  if (gicp) {  // upper triangles packed 6 doubles per point; rows of other problems are never read
    double* cs = h->stage.data() + 3 * (s_off + t_off);
    double* ct = cs + 6 * s_off;
    for (int b = 0; b < batch; ++b) {
      const IcpDesc& d = desc[(size_t)b];
      if (d.method != kIcpMethodGicp) continue;
      if (d.n_s) pack_cov(src_cov[b], d.n_s, cs + 6 * d.s_off);
      if (d.n_t) pack_cov(dst_cov[b], d.n_t, ct + 6 * d.t_off);
    }
    if (s_off)
      FCHK(h, hipMemcpyAsync(B[B_COV_S].p, cs, sizeof(double) * 6 * s_off, hipMemcpyHostToDevice, s),
           "hipMemcpyAsync (source covariances)");
    if (t_off)
      FCHK(h, hipMemcpyAsync(B[B_COV_T].p, ct, sizeof(double) * 6 * t_off, hipMemcpyHostToDevice, s),
           "hipMemcpyAsync (target covariances)");
  }

  // ---- (self-estimated normals,) target index, then the iteration groups ----
  if (hook && (rc = hook(h, ctx, ix)) != TEASER_HIP_OK) return rc;
  if ((rc = launch_index(h, ix)) != TEASER_HIP_OK) return rc;
  int64_t passes = 0;  // correspondence passes enqueued: the first one + one per iteration
  for (;;) {
    for (int g = 0; g < kIcpGroup && passes <= (int64_t)max_iter; ++g, ++passes)
      if (color)
        iterate(h, ctx, n_blk, batch);
      else
        launch_icp_iteration(s, B[B_DESC].as<IcpDesc>(), B[B_STATE].as<IcpState>(), B[B_BLK].as<int32_t>(), n_blk,
                             batch, B[B_X].as<double>(), B[B_QS].as<double>(), B[B_QJ].as<int32_t>(),
                             B[B_BSTART].as<int32_t>(), B[B_NORMALS].as<double>(), B[B_COV_S].as<double>(),
                             B[B_COV_T].as<double>(), gicp ? 2 : plane ? 1 : 0, B[B_MATCH].as<int32_t>(),
                             B[B_PARTIALS].as<double>());
    launch_icp_live(s, B[B_STATE].as<IcpState>(), batch, B[B_LIVE].as<int32_t>());
    FCHK(h, hipGetLastError(), "ICP kernel launch");
    FCHK(h, hipMemcpyAsync(h->h_live, B[B_LIVE].p, sizeof(int32_t), hipMemcpyDeviceToHost, s),
         "hipMemcpyAsync (live count)");
    FCHK(h, hipStreamSynchronize(s), "ICP iterations");
    if (*h->h_live == 0) break;
    if (passes > (int64_t)max_iter) return fail(h, TEASER_HIP_ERR_HIP, "ICP: problems left unfinished");
  }

  // ---- results ----
  FCHK(h, hipMemcpyAsync(state.data(), B[B_STATE].p, bytes[B_STATE], hipMemcpyDeviceToHost, s),
       "hipMemcpyAsync (state)");
  bool want_corr = false;
  for (int b = 0; corr && b < batch; ++b) want_corr |= corr[b] != nullptr && n_src[b] > 0;
  std::vector<int32_t> match;
  if (want_corr) {
    match.resize((size_t)s_off);
    FCHK(h, hipMemcpyAsync(match.data(), B[B_MATCH].p, sizeof(int32_t) * s_off, hipMemcpyDeviceToHost, s),
         "hipMemcpyAsync (correspondences)");
  }
  FCHK(h, hipStreamSynchronize(s), "ICP results");
  for (int b = 0; b < batch; ++b) {
    const IcpState& st = state[(size_t)b];
    teaser_icp_result_c& o = out[b];
    for (int k = 0; k < 16; ++k) o.transformation[k] = st.T[k];
    o.fitness = st.fitness;
    o.inlier_rmse = st.rmse;
    o.iterations = st.iterations;
    o.n_correspondences = st.count;
    if (want_corr && corr[b] && n_src[b] > 0) {
      const int32_t* m = match.data() + desc[(size_t)b].s_off;
      int32_t k = 0;
      for (int32_t i = 0; i < n_src[b]; ++i)
        if (m[i] >= 0) {
          corr[b][2 * k] = i;
          corr[b][2 * k + 1] = m[i];
          ++k;
        }
    }
  }
  return TEASER_HIP_OK;
}

}  // namespace thip

extern "C" {

int32_t teaser_hip_icp_solve(teaser_hip_icp* h, const double* src, int32_t n_src, const double* dst, int32_t n_dst,
                             const double* init, const teaser_icp_params_c* params, teaser_icp_result_c* out,
                             int32_t* corr) {
  return teaser_hip_icp_solve_ex(h, src, n_src, dst, n_dst, init, params, out, corr, nullptr, nullptr);
}

int32_t teaser_hip_icp_solve_ex(teaser_hip_icp* h, const double* src, int32_t n_src, const double* dst,
                                int32_t n_dst, const double* init, const teaser_icp_params_c* params,
                                teaser_icp_result_c* out, int32_t* corr, const double* dst_normals,
                                const teaser_icp_estimation_c* est) {
  int32_t* const corrs[1] = {corr};
  return teaser_hip_icp_batch_ex(h, 1, &src, &n_src, &dst, &n_dst, init, params, out, corrs,
                                 dst_normals ? &dst_normals : nullptr, est);
}

int32_t teaser_hip_icp_solve_cov(teaser_hip_icp* h, const double* src, int32_t n_src, const double* dst,
                                 int32_t n_dst, const double* init, const teaser_icp_params_c* params,
                                 teaser_icp_result_c* out, int32_t* corr, const double* dst_normals,
                                 const teaser_icp_estimation_c* est, const double* src_cov, const double* dst_cov) {
  int32_t* const corrs[1] = {corr};
  return teaser_hip_icp_batch_cov(h, 1, &src, &n_src, &dst, &n_dst, init, params, out, corrs,
                                  dst_normals ? &dst_normals : nullptr, est, src_cov ? &src_cov : nullptr,
                                  dst_cov ? &dst_cov : nullptr);
}

int32_t teaser_hip_icp_covariances_batch(teaser_hip_icp* h, int32_t batch, const double* const* points,
                                         const int32_t* n, const double* radius, const int32_t* max_nn,
                                         const double* epsilon, double* const* out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (batch < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0");
  if (batch == 0) return TEASER_HIP_OK;
  if (!n) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must not be NULL");
  if (!radius) return fail(h, TEASER_HIP_ERR_BAD_ARG, "radius must not be NULL");
  if (!max_nn) return fail(h, TEASER_HIP_ERR_BAD_ARG, "max_nn must not be NULL");
  int64_t total = 0;
  for (int b = 0; b < batch; ++b) {
    const double r = radius[b], eps = epsilon ? epsilon[b] : 1e-3;
    if (!std::isfinite(r) || !(r > 0) || !std::isfinite(r * r) || !(r * r > 0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "radius (and its square) must be finite and > 0" + at(b));
    if (!std::isfinite(eps) || !(eps > 0)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "epsilon must be finite and > 0" + at(b));
    if (max_nn[b] < 3 || max_nn[b] > kIcpCovMaxNN)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "max_nn must lie in [3, " + std::to_string(kIcpCovMaxNN) + "]" + at(b));
    if (n[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must be >= 0" + at(b));
    if (n[b] > 0 && (!points || !points[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "points is NULL" + at(b));
    if (n[b] > 0 && (!out || !out[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "out is NULL" + at(b));
    if (n[b] > 0 && !finite_points(points[b], n[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "points has a non-finite coordinate" + at(b));
    total += n[b];
  }
  if (total >= INT32_MAX / 9) return fail(h, TEASER_HIP_ERR_BAD_ARG, "too many points in one call");
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");

  // the ICP grid over each cloud itself (the cloud is the descriptor's target), cell edge from its radius
  IcpIndex ix;
  std::vector<IcpCovDesc> cov((size_t)batch);
  int top_nn = 0;
  for (int b = 0; b < batch; ++b) {
    add_problem(ix, b, 0, n[b], points, radius[b], (n[b] + kIcpCovBlock - 1) / kIcpCovBlock);
    cov[(size_t)b].max_nn = max_nn[b];
    cov[(size_t)b].pad = 0;
    cov[(size_t)b].eps = epsilon ? epsilon[b] : 1e-3;
    if (n[b] > 0) top_nn = std::max(top_nn, max_nn[b]);
  }
  const std::vector<IcpDesc>& desc = ix.desc;
  const int64_t t_off = ix.t_off;
  if (t_off == 0) return TEASER_HIP_OK;
  const int n_blk = (int)ix.blk_prob.size();
  // B_STATE holds the IcpCovDesc records and B_X the 9 doubles per point of the output during this call
  size_t bytes[B_COUNT] = {};
  index_bytes(ix, 0, false, bytes);
  bytes[B_STATE] = sizeof(IcpCovDesc) * batch;
  bytes[B_X] = sizeof(double) * 9 * t_off;
  int32_t rc = ensure_buffers(h, bytes, "hipMalloc failed (covariance buffers)");
  if (rc != TEASER_HIP_OK) return rc;
  hipStream_t s = h->stream;
  DevBuf* B = h->buf;
  h->stage.resize((size_t)(9 * t_off));
  rc = upload_inputs(h, ix, nullptr, points, n, cov.data(), bytes[B_STATE]);
  if (rc == TEASER_HIP_OK) rc = launch_index(h, ix);
  if (rc != TEASER_HIP_OK) return rc;
  launch_icp_covariances(s, B[B_DESC].as<IcpDesc>(), B[B_STATE].as<IcpCovDesc>(), B[B_BLK].as<int32_t>(), n_blk,
                         top_nn, B[B_Q].as<double>(), B[B_QS].as<double>(), B[B_QJ].as<int32_t>(),
                         B[B_BSTART].as<int32_t>(), B[B_X].as<double>());
  FCHK(h, hipGetLastError(), "covariance kernel launch");
  FCHK(h, hipMemcpyAsync(h->stage.data(), B[B_X].p, bytes[B_X], hipMemcpyDeviceToHost, s),
       "hipMemcpyAsync (covariances)");
  FCHK(h, hipStreamSynchronize(s), "covariance estimation");
  for (int b = 0; b < batch; ++b)
    if (n[b]) memcpy(out[b], &h->stage[(size_t)(9 * desc[(size_t)b].t_off)], 72 * (size_t)n[b]);
  return TEASER_HIP_OK;
}

}  // extern "C"
