// icp_normals.hip -- host side of normal estimation on the ICP handle (include/teaser_hip.h, "Normal estimation") and
// of the point-to-plane entry that estimates its own target normals (teaser_hip_icp_batch_auto).
// Kernels: icp_normals_kernel (kernels_icp.hip, hybrid search) and the covariance consumer of the self k-NN kernels
// (kernels_outlier.hip, k-NN search); design and launch count in DESIGN.md section 18.
//
// One plan serves both entries: per cloud an IcpDesc with the grid of its search (the radius for hybrid search, the
// self k-NN edge for k-NN search), an IcpKnnDesc and an IcpNormalDesc; the blocks of the hybrid clouds come first in
// the block map, those of the k-NN clouds after them, so each search kernel is launched on its own range.
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

static_assert(sizeof(teaser_icp_normal_search_c) == 48, "the header states the record's size");

namespace {

// One search record; `arg` names the argument in the message.
int32_t check_search(teaser_hip_icp* h, const teaser_icp_normal_search_c& r, int b, const char* arg) {
  const std::string a(arg);
  if (r.search < 0 || r.search > 1) return fail(h, TEASER_HIP_ERR_BAD_ARG, a + ": search must be 0 or 1" + at(b));
  if (r.orient < 0 || r.orient > 2) return fail(h, TEASER_HIP_ERR_BAD_ARG, a + ": orient must be 0, 1 or 2" + at(b));
  if (r.reserved != 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, a + ": reserved must be 0" + at(b));
  if (r.max_nn < 3 || r.max_nn > kIcpCovMaxNN)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, a + ": max_nn must lie in [3, " + std::to_string(kIcpCovMaxNN) + "]" + at(b));
  if (r.search == 0) {
    const double rad = r.radius;
    if (!std::isfinite(rad) || !(rad > 0) || !std::isfinite(rad * rad) || !(rad * rad > 0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, a + ": radius (and its square) must be finite and > 0" + at(b));
  }
  if (r.orient != 0 && !(std::isfinite(r.ref[0]) && std::isfinite(r.ref[1]) && std::isfinite(r.ref[2])))
    return fail(h, TEASER_HIP_ERR_BAD_ARG, a + ": ref must be finite" + at(b));
  return TEASER_HIP_OK;
}

// Appends cloud b (n points at points[b]; n = 0: skipped) with search record r.  t_off < 0: the clouds are packed one
// after the other; else the cloud's first point in the caller's own packing of B_Q.
void plan_cloud(teaser_hip_icp* h, NormalsPlan& P, int b, int32_t n, const double* const* points,
                const teaser_icp_normal_search_c& r, int64_t t_off, std::vector<int32_t>& hyb,
                std::vector<int32_t>& knn_blk) {
  IcpKnnDesc kd;
  memset(&kd, 0, sizeof(kd));
  kd.edge = 1.0;
  IcpNormalDesc nd;
  memset(&nd, 0, sizeof(nd));
  nd.cov_off = nd.eig_off = -1;
  double edge = 1.0;
  const bool is_knn = n > 0 && r.search == 1;
  if (n > 0) {
    nd.max_nn = r.max_nn;
    nd.orient = r.orient;
    for (int c = 0; c < 3; ++c) nd.ref[c] = r.orient ? r.ref[c] : 0.0;
    edge = r.radius;
    if (is_knn) {
      const int want = std::min(r.max_nn, n);
      bool rings_ok = true;
      kd.k = r.max_nn;
      kd.ring_cap = h->knn_ring_cap;
      kd.edge = edge = knn_edge(points[b], n, want, &rings_ok);
      if (!rings_ok) kd.ring_cap = 0;
      P.top_knn = std::max(P.top_knn, want);
    } else {
      P.top_hyb = std::max(P.top_hyb, r.max_nn);
    }
  }
  IcpDesc& d = add_problem(P.ix, b, 0, n, points, edge, 0);
  if (t_off >= 0) d.t_off = t_off;
  std::vector<int32_t>& map = is_knn ? knn_blk : hyb;
  d.blk_off = (int32_t)map.size();  // inside its own kernel's range of the block map
  d.nblk = (n + kIcpCovBlock - 1) / kIcpCovBlock;
  for (int k = 0; k < d.nblk; ++k) map.push_back(b);
  P.knn.push_back(kd);
  P.nd.push_back(nd);
}

void finish_plan(NormalsPlan& P, const std::vector<int32_t>& hyb, const std::vector<int32_t>& knn_blk) {
  P.n_hyb = (int)hyb.size();
  P.n_knn = (int)knn_blk.size();
  P.blk = hyb;
  P.blk.insert(P.blk.end(), knn_blk.begin(), knn_blk.end());
}

// Uploads the plan's descriptors and block maps (B_N*), builds the index over the points at d_q (packed at the
// descriptors' t_off) and enqueues the search launches.  The index and worklist buffers (B_TBUCKET .. B_QJ, B_MATCH:
// 2 int32 per point) must have been sized by the caller; counter: one int32 on the device, cleared here.
int32_t launch_normals(teaser_hip_icp* h, const NormalsPlan& P, const double* d_q, double* d_nrm, double* d_cov,
                       double* d_eig, int32_t* d_counter) {
  const size_t batch = P.ix.desc.size();
  DevBuf* B = h->buf;
  hipStream_t s = h->stream;
  const struct {
    int buf;
    const void* src;
    size_t n;
  } copies[] = {{B_NDESC, P.ix.desc.data(), sizeof(IcpDesc) * batch},
                {B_NKNN, P.knn.data(), sizeof(IcpKnnDesc) * batch},
                {B_NREC, P.nd.data(), sizeof(IcpNormalDesc) * batch},
                {B_NBLK, P.blk.data(), sizeof(int32_t) * P.blk.size()},
                {B_NTBLK, P.ix.tblk_prob.data(), sizeof(int32_t) * P.ix.tblk_prob.size()}};
  for (const auto& c : copies) {
    if (!B[c.buf].ensure(std::max<size_t>(c.n, 1))) return fail(h, TEASER_HIP_ERR_OOM, "hipMalloc failed (normals)");
    if (c.n) FCHK(h, hipMemcpyAsync(B[c.buf].p, c.src, c.n, hipMemcpyHostToDevice, s), "hipMemcpyAsync (normals)");
  }
  // the counters: the bucket counts of the index and the worklist's
  if (P.ix.b_off) FCHK(h, hipMemsetAsync(B[B_BCOUNT].p, 0, sizeof(int32_t) * P.ix.b_off, s), "hipMemsetAsync");
  FCHK(h, hipMemsetAsync(d_counter, 0, sizeof(int32_t), s), "hipMemsetAsync");
  const IcpDesc* desc = B[B_NDESC].as<IcpDesc>();
  launch_icp_index(s, desc, B[B_NTBLK].as<int32_t>(), (int)P.ix.tblk_prob.size(), (int)batch, d_q,
                   B[B_TBUCKET].as<int32_t>(), B[B_BCOUNT].as<int32_t>(), B[B_BSTART].as<int32_t>(),
                   B[B_CURSOR].as<int32_t>(), B[B_QS].as<double>(), B[B_QJ].as<int32_t>());
  launch_icp_normals_hybrid(s, desc, B[B_NREC].as<IcpNormalDesc>(), B[B_NBLK].as<int32_t>(), P.n_hyb, P.top_hyb, d_q,
                            B[B_QS].as<double>(), B[B_QJ].as<int32_t>(), B[B_BSTART].as<int32_t>(), d_nrm, d_cov,
                            d_eig);
  launch_icp_normals_knn(s, desc, B[B_NKNN].as<IcpKnnDesc>(), B[B_NREC].as<IcpNormalDesc>(),
                         B[B_NBLK].as<int32_t>() + P.n_hyb, P.n_knn, P.top_knn, d_q, B[B_QS].as<double>(),
                         B[B_QJ].as<int32_t>(), B[B_BSTART].as<int32_t>(), d_nrm, d_cov, d_eig,
                         B[B_MATCH].as<int32_t>(), d_counter);
  FCHK(h, hipGetLastError(), "normal estimation kernel launch");
  return TEASER_HIP_OK;
}

// teaser_hip_icp_batch_auto: the plan of the problems whose normals are estimated, and what the hook leaves behind
struct AutoCtx {
  NormalsPlan plan;
  bool copied = false;  // the worklist count was copied to h->back[0] behind the search launches
  bool any = false;
};

int32_t auto_hook(teaser_hip_icp* h, void* ctx, const IcpIndex&) {
  AutoCtx& A = *static_cast<AutoCtx*>(ctx);
  if (!A.any) return TEASER_HIP_OK;
  DevBuf* B = h->buf;
  // B_LIVE is free until the first iteration group ends: it holds the worklist counter meanwhile
  int32_t rc = launch_normals(h, A.plan, B[B_Q].as<double>(), B[B_NORMALS].as<double>(), nullptr, nullptr,
                              B[B_LIVE].as<int32_t>());
  if (rc != TEASER_HIP_OK) return rc;
  // into the handle's own buffer, which outlives every return of the call; read after the call's synchronisations
  if (h->back.empty()) h->back.resize(1);
  FCHK(h, hipMemcpyAsync(h->back.data(), B[B_LIVE].p, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream),
       "hipMemcpyAsync (worklist count)");
  A.copied = true;
  return TEASER_HIP_OK;
}

}  // namespace

namespace thip {

int32_t check_normal_search(teaser_hip_icp* h, const teaser_icp_normal_search_c& r, int b, const char* arg) {
  return check_search(h, r, b, arg);
}

void plan_normals_in_place(teaser_hip_icp* h, NormalsPlan& P, int32_t batch, const double* const* points,
                           const int32_t* n, const teaser_icp_normal_search_c* rec, const char* estimated) {
  std::vector<int32_t> hyb, knn_blk;
  int64_t t_off = 0;
  for (int b = 0; b < batch; ++b) {
    plan_cloud(h, P, b, estimated[b] ? n[b] : 0, points, rec[b], t_off, hyb, knn_blk);
    P.nd.back().nrm_off = t_off;
    t_off += n[b];
  }
  finish_plan(P, hyb, knn_blk);
}

int32_t launch_normals_plan(teaser_hip_icp* h, const NormalsPlan& P, const double* d_q, double* d_nrm,
                            int32_t* d_counter) {
  return launch_normals(h, P, d_q, d_nrm, nullptr, nullptr, d_counter);
}

}  // namespace thip

extern "C" {

int32_t teaser_hip_icp_normals_batch(teaser_hip_icp* h, int32_t batch, const double* const* points, const int32_t* n,
                                     const teaser_icp_normal_search_c* search, double* const* normals_out,
                                     double* const* cov_out, double* const* eig_out) {
  const CallStart c = begin_cloud_call(h, batch, points, n, true);
  if (c.done) return c.rc;
  int32_t rc = TEASER_HIP_OK;
  if (!search) return fail(h, TEASER_HIP_ERR_BAD_ARG, "search must not be NULL");
  for (int b = 0; b < batch; ++b) {
    if ((rc = check_search(h, search[b], b, "search")) != TEASER_HIP_OK) return rc;
    if (n[b] > 0 && (!normals_out || !normals_out[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "normals_out is NULL" + at(b));
  }
  if (c.total == 0) return TEASER_HIP_OK;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");

  NormalsPlan P;
  std::vector<int32_t> hyb, knn_blk;
  int64_t cov_rows = 0, eig_rows = 0;
  for (int b = 0; b < batch; ++b) {
    plan_cloud(h, P, b, n[b], points, search[b], -1, hyb, knn_blk);
    IcpNormalDesc& nd = P.nd.back();
    nd.nrm_off = P.ix.desc.back().t_off;
    if (n[b] > 0 && cov_out && cov_out[b]) {
      nd.cov_off = cov_rows;
      cov_rows += n[b];
    }
    if (n[b] > 0 && eig_out && eig_out[b]) {
      nd.eig_off = eig_rows;
      eig_rows += n[b];
    }
  }
  finish_plan(P, hyb, knn_blk);
  const int64_t t_off = P.ix.t_off;
  // B_X: normals, then covariances, then eigenvalues (only the rows asked for), then the worklist counter
  const size_t o_cov = sizeof(double) * 3 * t_off, o_eig = o_cov + sizeof(double) * 9 * cov_rows,
               o_cnt = o_eig + sizeof(double) * 3 * eig_rows, out_bytes = o_cnt + sizeof(int32_t);
  size_t bytes[B_COUNT] = {};
  index_bytes(P.ix, 0, true, bytes);
  bytes[B_DESC] = bytes[B_TBLK] = 0;  // launch_normals keeps the descriptors and the block maps in B_N*
  bytes[B_X] = out_bytes;
  if ((rc = ensure_buffers(h, bytes, "hipMalloc failed (normals buffers)")) != TEASER_HIP_OK) return rc;
  DevBuf* B = h->buf;
  h->stage.resize((size_t)(3 * t_off));
  if ((rc = upload_points(h, batch, points, n, 0, "hipMemcpyAsync (points)")) != TEASER_HIP_OK) return rc;
  char* out = B[B_X].as<char>();
  if ((rc = launch_normals(h, P, B[B_Q].as<double>(), (double*)out, (double*)(out + o_cov), (double*)(out + o_eig),
                           (int32_t*)(out + o_cnt))) != TEASER_HIP_OK)
    return rc;
  if ((rc = copy_back(h, 0, out_bytes, "normal estimation", nullptr)) != TEASER_HIP_OK) return rc;
  read_fallbacks(h, o_cnt);
  const char* back = (const char*)h->back.data();
  for (int b = 0; b < batch; ++b) {
    if (n[b] == 0) continue;
    const IcpNormalDesc& nd = P.nd[(size_t)b];
    memcpy(normals_out[b], back + sizeof(double) * 3 * nd.nrm_off, 24 * (size_t)n[b]);
    if (nd.cov_off >= 0) memcpy(cov_out[b], back + o_cov + sizeof(double) * 9 * nd.cov_off, 72 * (size_t)n[b]);
    if (nd.eig_off >= 0) memcpy(eig_out[b], back + o_eig + sizeof(double) * 3 * nd.eig_off, 24 * (size_t)n[b]);
  }
  return TEASER_HIP_OK;
}

int32_t teaser_hip_icp_batch_auto(teaser_hip_icp* h, int32_t batch, const double* const* src, const int32_t* n_src,
                                  const double* const* dst, const int32_t* n_dst, const double* init,
                                  const teaser_icp_params_c* params, teaser_icp_result_c* out, int32_t* const* corr,
                                  const double* const* dst_normals, const teaser_icp_estimation_c* est,
                                  const double* const* src_cov, const double* const* dst_cov,
                                  const teaser_icp_normal_search_c* nsearch) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  // which problems estimate their normals: point-to-plane, no normals given, a record with max_nn != 0
  std::vector<char> estimated((size_t)std::max(batch, 0), 0);
  bool any = false;
  if (nsearch && est && n_dst && batch > 0)
    for (int b = 0; b < batch; ++b) {
      if (est[b].method != kIcpMethodPlane || nsearch[b].max_nn == 0 || (dst_normals && dst_normals[b])) continue;
      const int32_t rc = check_search(h, nsearch[b], b, "dst_normal_search");
      if (rc != TEASER_HIP_OK) return rc;
      estimated[(size_t)b] = 1;
      any = true;
    }
  if (!any)
    return icp_run_batch(h, batch, src, n_src, dst, n_dst, init, params, out, corr, dst_normals, est, src_cov, dst_cov,
                         kIcpMethodGicp, nullptr, nullptr, nullptr);
  // the records icp_run_batch's own checks see: max_nn != 0 exactly for the estimated problems
  std::vector<teaser_icp_normal_search_c> rec(nsearch, nsearch + batch);
  for (int b = 0; b < batch; ++b)
    if (!estimated[(size_t)b]) rec[(size_t)b].max_nn = 0;
  // The plan needs valid clouds; icp_run_batch checks them before it calls the hook, so it is built here only from
  // what is safe to read (n_dst >= 0, dst given, finite) and otherwise left to icp_run_batch's refusal.
  AutoCtx A;
  std::vector<int32_t> hyb, knn_blk;
  int64_t t_off = 0;
  bool ok = dst != nullptr;
  for (int b = 0; ok && b < batch; ++b)
    ok = n_dst[b] >= 0 && (n_dst[b] == 0 || (dst[b] && finite_points(dst[b], n_dst[b])));
  for (int b = 0; ok && b < batch; ++b) {
    const int32_t nb = estimated[(size_t)b] ? n_dst[b] : 0;
    plan_cloud(h, A.plan, b, nb, dst, rec[(size_t)b], t_off, hyb, knn_blk);
    A.plan.nd.back().nrm_off = t_off;  // the rows of the packed normals the correspondence pass gathers from
    A.any |= nb > 0;
    t_off += n_dst[b];
  }
  if (ok) finish_plan(A.plan, hyb, knn_blk);
  A.any &= ok;
  h->knn_fallbacks = 0;
  const int32_t rc = icp_run_batch(h, batch, src, n_src, dst, n_dst, init, params, out, corr, dst_normals, est,
                                   src_cov, dst_cov, kIcpMethodGicp, rec.data(), auto_hook, &A);
  if (rc == TEASER_HIP_OK && A.copied) {
    int32_t fallbacks = 0;
    memcpy(&fallbacks, h->back.data(), sizeof(int32_t));
    h->knn_fallbacks = fallbacks;
  }
  return rc;
}

int32_t teaser_hip_icp_solve_auto(teaser_hip_icp* h, const double* src, int32_t n_src, const double* dst,
                                  int32_t n_dst, const double* init, const teaser_icp_params_c* params,
                                  teaser_icp_result_c* out, int32_t* corr, const double* dst_normals,
                                  const teaser_icp_estimation_c* est, const double* src_cov, const double* dst_cov,
                                  const teaser_icp_normal_search_c* nsearch) {
  int32_t* const corrs[1] = {corr};
  return teaser_hip_icp_batch_auto(h, 1, &src, &n_src, &dst, &n_dst, init, params, out, corrs,
                                   dst_normals ? &dst_normals : nullptr, est, src_cov ? &src_cov : nullptr,
                                   dst_cov ? &dst_cov : nullptr, nsearch);
}

}  // extern "C"
