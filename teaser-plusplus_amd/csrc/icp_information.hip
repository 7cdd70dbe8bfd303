// icp_information.hip -- host side of the information matrices on the ICP handle (include/teaser_hip.h,
// "Information matrices"): the entry checks, the call's index through the scaffold of icp_host.h, ONE correspondence
// pass of the point-to-point instantiation (max_iteration = 0: the evaluation teaser_hip_icp_batch returns for the
// same init, bit for bit, because it is the same launch on the same inputs), the reduction of
// kernels_icp_information.hip over the matches that pass left on the device, and one synchronisation.
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

extern "C" {

int32_t teaser_hip_icp_information_batch(teaser_hip_icp* h, int32_t batch, const double* const* src,
                                         const int32_t* n_src, const double* const* dst, const int32_t* n_dst,
                                         const double* transformation, const double* max_correspondence_distance,
                                         double* information, teaser_icp_result_c* out, int32_t* const* corr) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (batch < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0");
  if (batch == 0) return TEASER_HIP_OK;
  if (!n_src || !n_dst) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src / n_dst must not be NULL");
  if (!transformation) return fail(h, TEASER_HIP_ERR_BAD_ARG, "transformation must not be NULL");
  if (!max_correspondence_distance)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "max_correspondence_distance must not be NULL");
  if (!information) return fail(h, TEASER_HIP_ERR_BAD_ARG, "information must not be NULL");
  int64_t total_s = 0, total_t = 0;
  for (int b = 0; b < batch; ++b) {
    const double r = max_correspondence_distance[b];
    if (!std::isfinite(r) || !(r > 0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "max_correspondence_distance must be finite and > 0" + at(b));
    if (!std::isfinite(r * r) || !(r * r > 0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "max_correspondence_distance squared must be finite and > 0" + at(b));
    if (n_src[b] < 0 || n_dst[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src / n_dst must be >= 0" + at(b));
    if (n_src[b] > 0 && (!src || !src[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "src is NULL" + at(b));
    if (n_dst[b] > 0 && (!dst || !dst[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst is NULL" + at(b));
    if (n_src[b] > 0 && !finite_points(src[b], n_src[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "src has a non-finite coordinate" + at(b));
    if (n_dst[b] > 0 && !finite_points(dst[b], n_dst[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst has a non-finite coordinate" + at(b));
    const double* T = transformation + 16 * (int64_t)b;
    for (int k = 0; k < 16; ++k)
      if (!std::isfinite(T[k])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "transformation is not finite" + at(b));
    if (T[12] != 0 || T[13] != 0 || T[14] != 0 || T[15] != 1)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "transformation: last row must be 0 0 0 1" + at(b));
    total_s += n_src[b];
    total_t += n_dst[b];
  }
  if (total_s >= INT32_MAX || total_t >= INT32_MAX / 2)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "too many points in one call");
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");

  // ---- descriptors, block maps and the state of a problem that stops after its first correspondence pass ----
  IcpIndex ix;
  std::vector<IcpState> state((size_t)batch);
  for (int b = 0; b < batch; ++b) {
    add_problem(ix, b, n_src[b], n_dst[b], dst, max_correspondence_distance[b],
                (n_src[b] + kIcpBlock - 1) / kIcpBlock);  // max_iteration 0, point-to-point: the zeroes of add_problem
    IcpState& st = state[(size_t)b];
    memset(&st, 0, sizeof(st));
    const double* T = transformation + 16 * (int64_t)b;
    for (int k = 0; k < 16; ++k) st.T[k] = T[k];
    for (int k = 0; k < 12; ++k) st.U[k] = T[k];
  }
  const int64_t s_off = ix.s_off;
  const int n_blk = (int)ix.blk_prob.size();

  // ---- device buffers: B_PARTIALS holds the block partials (the correspondence pass's kIcpSums per block, then,
  // once its finalize has read them, this reduction's kIcpInfoSums), followed by 36 doubles per problem ----
  const size_t pts_s = (size_t)std::max<int64_t>(s_off, 1);
  const size_t part = (size_t)std::max(kIcpSums, kIcpInfoSums) * (size_t)std::max(n_blk, 1);
  size_t bytes[B_COUNT] = {};
  index_bytes(ix, 1, false, bytes);
  bytes[B_STATE] = sizeof(IcpState) * batch;
  bytes[B_X] = sizeof(double) * 3 * pts_s;
  bytes[B_MATCH] = sizeof(int32_t) * pts_s;
  bytes[B_PARTIALS] = sizeof(double) * (part + 36 * (size_t)batch);
  int32_t rc = ensure_buffers(h, bytes, "hipMalloc failed (information-matrix buffers)");
  if (rc != TEASER_HIP_OK) return rc;
  hipStream_t s = h->stream;
  DevBuf* B = h->buf;
  h->stage.resize((size_t)(3 * (s_off + ix.t_off)));
  if ((rc = upload_inputs(h, ix, src, dst, n_dst, state.data(), bytes[B_STATE])) != TEASER_HIP_OK) return rc;
  if ((rc = launch_index(h, ix)) != TEASER_HIP_OK) return rc;
  launch_icp_iteration(s, B[B_DESC].as<IcpDesc>(), B[B_STATE].as<IcpState>(), B[B_BLK].as<int32_t>(), n_blk, batch,
                       B[B_X].as<double>(), B[B_QS].as<double>(), B[B_QJ].as<int32_t>(), B[B_BSTART].as<int32_t>(),
                       nullptr, nullptr, nullptr, 0, B[B_MATCH].as<int32_t>(), B[B_PARTIALS].as<double>());
  double* d_info = B[B_PARTIALS].as<double>() + part;
  launch_icp_information(s, B[B_DESC].as<IcpDesc>(), B[B_BLK].as<int32_t>(), n_blk, batch, B[B_Q].as<double>(),
                         B[B_MATCH].as<int32_t>(), B[B_PARTIALS].as<double>(), d_info);
  FCHK(h, hipGetLastError(), "information-matrix kernel launch");

  // ---- results: one synchronisation ----
  FCHK(h, hipMemcpyAsync(information, d_info, sizeof(double) * 36 * (size_t)batch, hipMemcpyDeviceToHost, s),
       "hipMemcpyAsync (information matrices)");
  if (out)
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
  FCHK(h, hipStreamSynchronize(s), "information matrices");
  for (int b = 0; b < batch; ++b) {
    if (out) {
      const IcpState& st = state[(size_t)b];
      teaser_icp_result_c& o = out[b];
      for (int k = 0; k < 16; ++k) o.transformation[k] = st.T[k];
      o.fitness = st.fitness;
      o.inlier_rmse = st.rmse;
      o.iterations = st.iterations;
      o.n_correspondences = st.count;
    }
    if (want_corr && corr[b] && n_src[b] > 0) {
      const int32_t* m = match.data() + ix.desc[(size_t)b].s_off;
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

int32_t teaser_hip_icp_information(teaser_hip_icp* h, const double* src, int32_t n_src, const double* dst,
                                   int32_t n_dst, const double* transformation, double max_correspondence_distance,
                                   double* information, teaser_icp_result_c* out, int32_t* corr) {
  int32_t* const corrs[1] = {corr};
  return teaser_hip_icp_information_batch(h, 1, &src, &n_src, &dst, &n_dst, transformation,
                                          &max_correspondence_distance, information, out, corrs);
}

}  // extern "C"
