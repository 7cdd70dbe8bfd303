// icp_fpfh.hip -- host side of the Open3D-form FPFH on the ICP handle (include/teaser_hip.h, "FPFH (Open3D form)").
// Kernels: kernels_fpfh.hip and the search kernels of kernels_search.hip; device code: icp_fpfh_device.h; design, launch
// counts and the resource report: DESIGN.md section 29.
//
// One call: the clouds are packed into B_Q, their normals into the front of B_X (given ones uploaded, the others
// estimated there by the launches of icp_normals.hip), then the grids of the descriptor's own search are built.  A cloud
// is cut into PIECES of points whose neighbour lists (max_nn slots of 12 bytes per point) fit "fpfh_list_bytes", pieces
// are collected into PASSES under the same bound, and every pass is a fixed sequence of launches over all its pieces:
// the lists (hybrid pieces, then k-NN pieces), then the SPFH rows.  When every SPFH row of the call is written, the
// passes run again for the FPFH rows; a call of one pass keeps its lists, a call of several recomputes them.  A point's
// list, SPFH row and FPFH row do not depend on the piece or the pass it falls into, so the option changes no bit.
// The pieces, the passes and the list launches (plan_lists .. launch_lists, declared in icp_host.h) also serve
// icp_boundary.hip.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_common.h"
#include "icp_fpfh_device.h"
#include "icp_host.h"
#include "icp_internal.h"
#include "teaser_hip.h"

using namespace thip;

namespace thip {

int32_t check_list_search(teaser_hip_icp* h, const teaser_icp_normal_search_c& r, int b) {
  if (r.search == 2)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "search: radius-only search (KDTreeSearchParamRadius) is not supported, it is "
                                           "uncapped: there is no bounded sorted list to sum over" + at(b));
  if (r.search < 0 || r.search > 1) return fail(h, TEASER_HIP_ERR_BAD_ARG, "search: search must be 0 or 1" + at(b));
  if (r.orient != 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "search: orient must be 0" + at(b));
  if (r.reserved != 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "search: reserved must be 0" + at(b));
  if (r.max_nn < 2 || r.max_nn > kIcpKnnMax)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "search: max_nn must lie in [2, " + std::to_string(kIcpKnnMax) + "]" + at(b));
  if (r.search == 0) {
    const double rad = r.radius;
    if (!std::isfinite(rad) || !(rad > 0) || !std::isfinite(rad * rad) || !(rad * rad > 0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "search: radius (and its square) must be finite and > 0" + at(b));
  }
  return TEASER_HIP_OK;
}

void plan_lists(teaser_hip_icp* h, ListPlan& L, int32_t batch, const double* const* points, const int32_t* n,
                const teaser_icp_normal_search_c* search) {
  IcpIndex& ix = L.ix;
  std::vector<IcpDesc>& piece = L.piece;
  std::vector<IcpSearchDesc>& psd = L.psd;
  std::vector<ListPass>& passes = L.passes;
  int& top_hyb = L.top_hyb;
  int& top_knn = L.top_knn;
  const int64_t bound = h->fpfh_list_bytes;
  int64_t pass_bytes = 0;
  for (int b = 0; b < batch; ++b) {
    const teaser_icp_normal_search_c& r = search[b];
    double edge = r.search == 0 ? r.radius : 1.0;
    bool rings_ok = true;
    if (r.search == 1 && n[b] > 0) edge = knn_edge(points[b], n[b], std::min(r.max_nn, n[b]), &rings_ok);
    const IcpDesc cloud = add_problem(ix, b, 0, n[b], points, edge, 0);
    if (n[b] == 0) continue;
    if (r.search == 0) top_hyb = std::max(top_hyb, r.max_nn);
    else top_knn = std::max(top_knn, std::min(r.max_nn, n[b]));
    // points per piece: what the bound holds, in whole blocks, and never less than one block
    const int64_t per = std::max<int64_t>(bound / (12 * (int64_t)r.max_nn) / kIcpCovBlock, 1) * kIcpCovBlock;
    for (int64_t start = 0; start < n[b]; start += per) {
      const int32_t cnt = (int32_t)std::min<int64_t>(per, n[b] - start);
      const int64_t bytes = 12 * (int64_t)cnt * r.max_nn;
      if (passes.empty() || pass_bytes + bytes > bound) {
        passes.emplace_back();
        pass_bytes = 0;
      }
      ListPass& P = passes.back();
      IcpDesc d = cloud;
      d.n_s = cnt;
      d.s_off = cloud.t_off + start;
      d.nblk = (cnt + kIcpCovBlock - 1) / kIcpCovBlock;
      d.blk_off = r.search == 0 ? P.n_hyb : P.n_knn;  // inside its own kind's range of the pass
      IcpSearchDesc s;
      memset(&s, 0, sizeof(s));
      s.k = r.max_nn;
      s.ring_cap = rings_ok ? h->knn_ring_cap : 0;
      s.out_off = P.slots;
      s.edge = r.search == 1 ? edge : 1.0;
      (r.search == 0 ? P.hyb : P.knn).push_back((int32_t)piece.size());
      (r.search == 0 ? P.n_hyb : P.n_knn) += d.nblk;
      P.slots += (int64_t)cnt * r.max_nn;
      pass_bytes += bytes;
      piece.push_back(d);
      psd.push_back(s);
      L.cloud.push_back(b);
    }
  }
  std::vector<int32_t>& blk = L.blk;
  int64_t& max_slots = L.max_slots;
  for (ListPass& P : passes) {
    P.blk0 = (int64_t)blk.size();
    for (const std::vector<int32_t>* kind : {&P.hyb, &P.knn})
      for (int32_t p : *kind) blk.insert(blk.end(), (size_t)piece[(size_t)p].nblk, p);
    max_slots = std::max(max_slots, P.slots);
  }
}

void list_bytes(const ListPlan& L, size_t (&bytes)[B_COUNT]) {
  bytes[B_FPFH_DESC] = sizeof(IcpDesc) * L.piece.size();
  bytes[B_FPFH_SD] = sizeof(IcpSearchDesc) * L.psd.size();
  bytes[B_FPFH_BLK] = sizeof(int32_t) * L.blk.size();
  bytes[B_FPFH_LIST] = 12 * (size_t)L.max_slots;
}

int32_t upload_lists(teaser_hip_icp* h, const ListPlan& L) {
  DevBuf* B = h->buf;
  const struct {
    int buf;
    const void* src;
    size_t n;
  } copies[] = {{B_DESC, L.ix.desc.data(), sizeof(IcpDesc) * L.ix.desc.size()},
                {B_TBLK, L.ix.tblk_prob.data(), sizeof(int32_t) * L.ix.tblk_prob.size()},
                {B_FPFH_DESC, L.piece.data(), sizeof(IcpDesc) * L.piece.size()},
                {B_FPFH_SD, L.psd.data(), sizeof(IcpSearchDesc) * L.psd.size()},
                {B_FPFH_BLK, L.blk.data(), sizeof(int32_t) * L.blk.size()}};
  for (const auto& cp : copies)
    if (cp.n)
      FCHK(h, hipMemcpyAsync(B[cp.buf].p, cp.src, cp.n, hipMemcpyHostToDevice, h->stream), "hipMemcpyAsync (inputs)");
  return TEASER_HIP_OK;
}

int32_t launch_lists(teaser_hip_icp* h, const ListPlan& L, const ListPass& P, int32_t* counter) {
  DevBuf* B = h->buf;
  hipStream_t s = h->stream;
  const IcpDesc* d_piece = B[B_FPFH_DESC].as<IcpDesc>();
  const IcpSearchDesc* d_sd = B[B_FPFH_SD].as<IcpSearchDesc>();
  double* list_d2 = B[B_FPFH_LIST].as<double>();
  int32_t* list_idx = (int32_t*)(list_d2 + L.max_slots);
  const double* d_q = B[B_Q].as<double>();
  const int32_t* map = B[B_FPFH_BLK].as<int32_t>() + P.blk0;
  // (the hybrid search's per-query counts are not needed: a row's valid entries end at its first index -1; they go
  // to B_TBUCKET, which is free once the index is built)
  launch_icp_search_hybrid(s, d_piece, d_sd, map, P.n_hyb, L.top_hyb, d_q, B[B_QS].as<double>(), B[B_QJ].as<int32_t>(),
                           B[B_BSTART].as<int32_t>(), list_idx, list_d2, B[B_TBUCKET].as<int32_t>());
  if (P.n_knn) {
    FCHK(h, hipMemsetAsync(counter, 0, sizeof(int32_t), s), "hipMemsetAsync");
    launch_icp_search_knn(s, d_piece, d_sd, map + P.n_hyb, P.n_knn, L.top_knn, d_q, d_q, B[B_QS].as<double>(),
                          B[B_QJ].as<int32_t>(), B[B_BSTART].as<int32_t>(), list_idx, list_d2,
                          B[B_MATCH].as<int32_t>(), counter);
  }
  return TEASER_HIP_OK;
}

}  // namespace thip

extern "C" {

int32_t teaser_hip_icp_fpfh_batch(teaser_hip_icp* h, int32_t batch, const double* const* points,
                                  const double* const* normals, const int32_t* n,
                                  const teaser_icp_normal_search_c* search,
                                  const teaser_icp_normal_search_c* normal_search, double* const* fpfh_out,
                                  double* const* spfh_out, double* const* normals_out) {
  const CallStart c = begin_cloud_call(h, batch, points, n, true);
  if (c.done) return c.rc;
  int32_t rc = TEASER_HIP_OK;
  if (!search) return fail(h, TEASER_HIP_ERR_BAD_ARG, "search must not be NULL");
  std::vector<char> estimated((size_t)batch, 0);
  bool any_estimated = false, any_given = false, want_spfh = false, want_normals = false;
  for (int b = 0; b < batch; ++b) {
    if ((rc = check_list_search(h, search[b], b)) != TEASER_HIP_OK) return rc;
    if (n[b] == 0) continue;
    if (normals && normals[b]) {
      if (!finite_points(normals[b], n[b]))
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "normals has a non-finite component" + at(b));
      any_given = true;
    } else if (normal_search && normal_search[b].max_nn != 0) {
      if ((rc = check_normal_search(h, normal_search[b], b, "normal_search")) != TEASER_HIP_OK) return rc;
      estimated[(size_t)b] = 1;
      any_estimated = true;
    } else {
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "normals is NULL and normal_search gives no record" + at(b));
    }
    if (!fpfh_out || !fpfh_out[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "fpfh_out is NULL" + at(b));
    want_spfh |= spfh_out && spfh_out[b];
    want_normals |= normals_out && normals_out[b];
  }
  if (c.total == 0) return TEASER_HIP_OK;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");

  // the clouds with the grids of the descriptor's search, and their pieces
  ListPlan L;
  plan_lists(h, L, batch, points, n, search);
  const IcpIndex& ix = L.ix;
  const std::vector<ListPass>& passes = L.passes;
  const int64_t max_slots = L.max_slots;

  NormalsPlan NP;
  if (any_estimated) plan_normals_in_place(h, NP, batch, points, n, normal_search, estimated.data());

  // B_X: the normals, the FPFH rows, the SPFH rows (copied back from the first to the last part asked for), then the
  // worklist counter of the k-NN searches
  const size_t total = (size_t)c.total;
  const size_t o_fpfh = sizeof(double) * 3 * total, o_spfh = o_fpfh + sizeof(double) * kFpfhDim * total;
  const size_t o_cnt = o_spfh + sizeof(double) * kFpfhDim * total;
  size_t bytes[B_COUNT] = {};
  index_bytes(ix, 1, true, bytes);
  const size_t nb = (size_t)std::max(ix.b_off, NP.ix.b_off);
  bytes[B_BCOUNT] = bytes[B_BSTART] = bytes[B_CURSOR] = sizeof(int32_t) * std::max<size_t>(nb, 1);
  bytes[B_X] = o_cnt + 8;
  list_bytes(L, bytes);
  if ((rc = ensure_buffers(h, bytes, "hipMalloc failed (FPFH buffers)")) != TEASER_HIP_OK) return rc;
  DevBuf* B = h->buf;
  hipStream_t s = h->stream;
  char* out = B[B_X].as<char>();
  h->stage.resize(3 * total);
  if ((rc = upload_points(h, batch, points, n, 0, "hipMemcpyAsync (points)")) != TEASER_HIP_OK) return rc;
  if (any_given) {  // the rows of the estimated clouds are written by the normals' launches
    h->cstage.assign(3 * total, 0.0);
    for (int b = 0; b < batch; ++b)
      if (n[b] > 0 && !estimated[(size_t)b])
        memcpy(&h->cstage[(size_t)(3 * ix.desc[(size_t)b].t_off)], normals[b], 24 * (size_t)n[b]);
    FCHK(h, hipMemcpyAsync(out, h->cstage.data(), o_fpfh, hipMemcpyHostToDevice, s), "hipMemcpyAsync (normals)");
  }
  if ((rc = upload_lists(h, L)) != TEASER_HIP_OK) return rc;
  int32_t* counter = (int32_t*)(out + o_cnt);
  if (any_estimated &&
      (rc = launch_normals_plan(h, NP, B[B_Q].as<double>(), (double*)out, counter)) != TEASER_HIP_OK)
    return rc;
  if ((rc = launch_index(h, ix)) != TEASER_HIP_OK) return rc;

  const IcpDesc* d_piece = B[B_FPFH_DESC].as<IcpDesc>();
  const IcpSearchDesc* d_sd = B[B_FPFH_SD].as<IcpSearchDesc>();
  double* list_d2 = B[B_FPFH_LIST].as<double>();
  int32_t* list_idx = (int32_t*)(list_d2 + max_slots);
  const double* d_q = B[B_Q].as<double>();
  double* d_spfh = (double*)(out + o_spfh);
  for (const ListPass& P : passes) {
    if ((rc = launch_lists(h, L, P, counter)) != TEASER_HIP_OK) return rc;
    launch_icp_fpfh_spfh(s, d_piece, d_sd, B[B_FPFH_BLK].as<int32_t>() + P.blk0, P.n_hyb, P.n_knn, d_q,
                         (const double*)out, list_idx, d_spfh);
  }
  for (const ListPass& P : passes) {
    if (passes.size() > 1 && (rc = launch_lists(h, L, P, counter)) != TEASER_HIP_OK) return rc;
    launch_icp_fpfh(s, d_piece, d_sd, B[B_FPFH_BLK].as<int32_t>() + P.blk0, P.n_hyb, P.n_knn, list_idx, list_d2, d_spfh,
                    (double*)(out + o_fpfh));
  }
  const size_t lo = want_normals ? 0 : o_fpfh, hi = want_spfh ? o_cnt : o_spfh;
  if ((rc = copy_back(h, lo, hi - lo, "FPFH", "kernel launch (FPFH)")) != TEASER_HIP_OK) return rc;
  const char* back = (const char*)h->back.data();  // begins at byte lo of B_X
  for (int b = 0; b < batch; ++b) {
    if (n[b] == 0) continue;
    const size_t row = (size_t)ix.desc[(size_t)b].t_off, cnt = (size_t)n[b];
    memcpy(fpfh_out[b], back + (o_fpfh - lo) + sizeof(double) * kFpfhDim * row, sizeof(double) * kFpfhDim * cnt);
    if (spfh_out && spfh_out[b])
      memcpy(spfh_out[b], back + (o_spfh - lo) + sizeof(double) * kFpfhDim * row, sizeof(double) * kFpfhDim * cnt);
    if (normals_out && normals_out[b]) memcpy(normals_out[b], back + sizeof(double) * 3 * row, 24 * cnt);
  }
  return TEASER_HIP_OK;
}

}  // extern "C"
