// icp_boundary.hip -- host side of boundary-point detection on the ICP handle (include/teaser_hip.h, "Boundary points").
// Kernels: kernels_boundary.hip and the search kernels of kernels_search.hip; device code: icp_boundary_device.h; design,
// launch counts and the resource report: DESIGN.md section 30.
//
// One call has the shape of the Open3D-form FPFH (icp_fpfh.hip), whose pieces, passes, list scratch and list launches
// it uses as they are: the clouds are packed into B_Q, their normals into the front of B_X (given ones uploaded, the
// others estimated there by the launches of icp_normals.hip), the grids of the search are built, and every pass is the
// list launches followed by ONE boundary launch over all its pieces.  A point's result depends on its own list alone,
// so the lists are computed once whatever the number of passes, and "fpfh_list_bytes" changes no bit.  The boundary
// points of a cloud are counted on the device (int32 atomics: the sum does not depend on the order).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_common.h"
#include "icp_boundary_device.h"
#include "icp_host.h"
#include "icp_internal.h"
#include "teaser_hip.h"

using namespace thip;

extern "C" {

int32_t teaser_hip_icp_boundary_points_batch(teaser_hip_icp* h, int32_t batch, const double* const* points,
                                             const double* const* normals, const int32_t* n,
                                             const teaser_icp_normal_search_c* search,
                                             const teaser_icp_normal_search_c* normal_search,
                                             const double* angle_threshold, uint8_t* const* mask_out,
                                             int32_t* n_boundary_out, double* const* max_gap_out,
                                             int32_t* const* count_out, double* const* normals_out) {
  const CallStart c = begin_cloud_call(h, batch, points, n, true);
  if (c.done) return c.rc;
  int32_t rc = TEASER_HIP_OK;
  if (!search) return fail(h, TEASER_HIP_ERR_BAD_ARG, "search must not be NULL");
  if (!angle_threshold) return fail(h, TEASER_HIP_ERR_BAD_ARG, "angle_threshold must not be NULL");
  if (!n_boundary_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_boundary_out must not be NULL");
  std::vector<char> estimated((size_t)batch, 0);
  bool any_estimated = false, any_given = false, want_normals = false;
  for (int b = 0; b < batch; ++b) {
    if ((rc = check_list_search(h, search[b], b)) != TEASER_HIP_OK) return rc;
    const double thr = angle_threshold[b];
    if (!std::isfinite(thr) || !(thr >= 0.0) || !(thr <= 360.0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "angle_threshold must be finite and lie in [0, 360]" + at(b));
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
    if (!mask_out || !mask_out[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "mask_out is NULL" + at(b));
    want_normals |= normals_out && normals_out[b];
  }
  for (int b = 0; b < batch; ++b) n_boundary_out[b] = 0;
  if (c.total == 0) return TEASER_HIP_OK;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");

  // the clouds with the grids of the search, their pieces, and the pieces' own records
  ListPlan L;
  plan_lists(h, L, batch, points, n, search);
  const IcpIndex& ix = L.ix;
  const double pi = 3.14159265358979323846;
  std::vector<IcpBoundaryDesc> pbd(L.piece.size());
  for (size_t p = 0; p < pbd.size(); ++p) {
    memset(&pbd[p], 0, sizeof(IcpBoundaryDesc));
    pbd[p].threshold = (angle_threshold[L.cloud[p]] * pi) / 180.0;
    pbd[p].cloud = L.cloud[p];
  }

  NormalsPlan NP;
  if (any_estimated) plan_normals_in_place(h, NP, batch, points, n, normal_search, estimated.data());

  // B_X: the normals, max_gap, the list lengths, the clouds' counts, the worklist counter of the k-NN searches, the
  // mask (copied back from the first part asked for to the end)
  const size_t total = (size_t)c.total;
  const size_t o_gap = sizeof(double) * 3 * total, o_m = o_gap + sizeof(double) * total;
  const size_t o_nb = o_m + sizeof(int32_t) * total, o_cnt = o_nb + sizeof(int32_t) * (size_t)batch;
  const size_t o_mask = o_cnt + 8, o_end = o_mask + total;
  size_t bytes[B_COUNT] = {};
  index_bytes(ix, 1, true, bytes);
  const size_t nb = (size_t)std::max(ix.b_off, NP.ix.b_off);
  bytes[B_BCOUNT] = bytes[B_BSTART] = bytes[B_CURSOR] = sizeof(int32_t) * std::max<size_t>(nb, 1);
  bytes[B_X] = o_end;
  list_bytes(L, bytes);
  bytes[B_BND_DESC] = sizeof(IcpBoundaryDesc) * pbd.size();
  if ((rc = ensure_buffers(h, bytes, "hipMalloc failed (boundary buffers)")) != TEASER_HIP_OK) return rc;
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
    FCHK(h, hipMemcpyAsync(out, h->cstage.data(), o_gap, hipMemcpyHostToDevice, s), "hipMemcpyAsync (normals)");
  }
  if ((rc = upload_lists(h, L)) != TEASER_HIP_OK) return rc;
  FCHK(h, hipMemcpyAsync(B[B_BND_DESC].p, pbd.data(), bytes[B_BND_DESC], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (inputs)");
  FCHK(h, hipMemsetAsync(out + o_nb, 0, o_mask - o_nb, s), "hipMemsetAsync");
  int32_t* counter = (int32_t*)(out + o_cnt);
  if (any_estimated &&
      (rc = launch_normals_plan(h, NP, B[B_Q].as<double>(), (double*)out, counter)) != TEASER_HIP_OK)
    return rc;
  if ((rc = launch_index(h, ix)) != TEASER_HIP_OK) return rc;

  const int32_t* list_idx = (const int32_t*)(B[B_FPFH_LIST].as<double>() + L.max_slots);
  for (const ListPass& P : L.passes) {
    if ((rc = launch_lists(h, L, P, counter)) != TEASER_HIP_OK) return rc;
    launch_icp_boundary(s, B[B_FPFH_DESC].as<IcpDesc>(), B[B_FPFH_SD].as<IcpSearchDesc>(),
                        B[B_BND_DESC].as<IcpBoundaryDesc>(), B[B_FPFH_BLK].as<int32_t>() + P.blk0, P.n_hyb, P.n_knn,
                        B[B_Q].as<double>(), (const double*)out, list_idx, (uint8_t*)(out + o_mask),
                        (double*)(out + o_gap), (int32_t*)(out + o_m), (int32_t*)(out + o_nb));
  }
  const size_t lo = want_normals ? 0 : o_gap;
  if ((rc = copy_back(h, lo, o_end - lo, "boundary points", "kernel launch (boundary points)")) != TEASER_HIP_OK)
    return rc;
  const char* base = (const char*)h->back.data();  // begins at byte lo of B_X
  auto back = [&](size_t x) { return base + (x - lo); };
  memcpy(n_boundary_out, back(o_nb), sizeof(int32_t) * (size_t)batch);
  for (int b = 0; b < batch; ++b) {
    if (n[b] == 0) continue;
    const size_t row = (size_t)ix.desc[(size_t)b].t_off, cnt = (size_t)n[b];
    memcpy(mask_out[b], back(o_mask + row), cnt);
    if (max_gap_out && max_gap_out[b]) memcpy(max_gap_out[b], back(o_gap + sizeof(double) * row), sizeof(double) * cnt);
    if (count_out && count_out[b]) memcpy(count_out[b], back(o_m + sizeof(int32_t) * row), sizeof(int32_t) * cnt);
    if (normals_out && normals_out[b]) memcpy(normals_out[b], back(sizeof(double) * 3 * row), 24 * cnt);
  }
  return TEASER_HIP_OK;
}

}  // extern "C"
