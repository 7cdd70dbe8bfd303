// icp_outlier.hip -- host side of self k-NN and of statistical and radius outlier removal on the ICP handle
// (include/teaser_hip.h, "Self k-NN", "Outlier removal"), and the handle's options.
// Kernels: kernels_outlier.hip; design and launch count in DESIGN.md section 17.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "host_common.h"
#include "icp_host.h"
#include "icp_internal.h"
#include "teaser_hip.h"

using namespace thip;

namespace thip {

// One self k-NN stage (icp_host.h).
int32_t run_self_knn(teaser_hip_icp* h, int32_t batch, const double* const* points, const int32_t* n, const int32_t* k,
                     const double* ratio, IcpIndex& ix, KnnLayout& L) {
  std::vector<IcpKnnDesc> knn((size_t)batch);
  int top = 0;
  for (int b = 0; b < batch; ++b) {
    IcpKnnDesc& kd = knn[(size_t)b];
    memset(&kd, 0, sizeof(kd));
    kd.k = k[b];
    kd.ring_cap = h->knn_ring_cap;
    kd.out_off = L.slots;
    kd.edge = 1.0;
    kd.ratio = ratio ? ratio[b] : 0.0;
    if (n[b] > 0) {
      const int want = std::min(k[b], n[b]);
      bool rings_ok = true;
      kd.edge = knn_edge(points[b], n[b], want, &rings_ok);
      if (!rings_ok) kd.ring_cap = 0;
      top = std::max(top, want);
    }
    add_problem(ix, b, 0, n[b], points, kd.edge, (n[b] + kIcpCovBlock - 1) / kIcpCovBlock);
    L.slots += (int64_t)n[b] * k[b];
  }
  const int64_t t_off = ix.t_off;
  const int n_blk = (int)ix.blk_prob.size(), n_tblk = (int)ix.tblk_prob.size();
  // B_X: doubles first, then int32, then the mask bytes; the worklist counter is the last of the int32 (statistical
  // removal) or lies, padded to 8 bytes, between the doubles and the indices (self k-NN)
  if (ratio) {
    L.avg = 0;
    L.stats = sizeof(double) * t_off;
    L.ints = L.stats + sizeof(double) * 3 * batch;
    L.counter = L.ints + sizeof(int32_t) * batch;
    L.keep = L.counter + sizeof(int32_t);
    L.bytes = L.keep + (size_t)t_off;
  } else {
    L.d2 = 0;
    L.res = sizeof(double) * L.slots;
    L.counter = L.res + sizeof(double) * L.res_per_cloud * batch;
    L.idx = L.counter + 8;
    L.bytes = L.idx + sizeof(int32_t) * L.slots;
  }
  size_t bytes[B_COUNT] = {};
  index_bytes(ix, 0, true, bytes);
  bytes[B_STATE] = sizeof(IcpKnnDesc) * batch;
  bytes[B_X] = L.bytes;
  bytes[B_PARTIALS] = ratio || L.res_per_cloud ? sizeof(double) * n_tblk : 0;
  int32_t rc = ensure_buffers(h, bytes, "hipMalloc failed (k-NN buffers)");
  if (rc != TEASER_HIP_OK) return rc;
  hipStream_t s = h->stream;
  DevBuf* B = h->buf;
  char* out = B[B_X].as<char>();
  h->stage.resize((size_t)(3 * t_off));
  if ((rc = upload_inputs(h, ix, nullptr, points, n, knn.data(), bytes[B_STATE])) != TEASER_HIP_OK) return rc;
  // the counters: the worklist's and in front of it the kept counts (statistical removal) or the per-cloud doubles
  if (ratio)
    FCHK(h, hipMemsetAsync(out + L.ints, 0, sizeof(int32_t) * ((size_t)batch + 1), s), "hipMemsetAsync");
  else
    FCHK(h, hipMemsetAsync(out + L.res, 0, L.idx - L.res, s), "hipMemsetAsync");
  if ((rc = launch_index(h, ix)) != TEASER_HIP_OK) return rc;
  launch_icp_self_knn(s, B[B_DESC].as<IcpDesc>(), B[B_STATE].as<IcpKnnDesc>(), B[B_BLK].as<int32_t>(), n_blk, top,
                      B[B_Q].as<double>(), B[B_QS].as<double>(), B[B_QJ].as<int32_t>(), B[B_BSTART].as<int32_t>(),
                      (int32_t*)(out + L.idx), (double*)(out + L.d2), ratio ? (double*)(out + L.avg) : nullptr,
                      B[B_MATCH].as<int32_t>(), (int32_t*)(out + L.counter));
  return TEASER_HIP_OK;
}

}  // namespace thip

extern "C" {

int32_t teaser_hip_icp_set_option(teaser_hip_icp* h, const char* name, int64_t value) {
  if (!h || !name) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (strcmp(name, "knn_ring_cap") == 0) {
    if (value < 0 || value > kIcpKnnRingCapMax)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "knn_ring_cap must lie in [0, " + std::to_string(kIcpKnnRingCapMax) + "]");
    h->knn_ring_cap = (int32_t)value;
    return TEASER_HIP_OK;
  }
  if (strcmp(name, "fps_resident_max") == 0) {
    if (value < 0 || value > kFpsResidentCap)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "fps_resident_max must lie in [0, " + std::to_string(kFpsResidentCap) + "]");
    h->fps_resident_max = (int32_t)value;
    return TEASER_HIP_OK;
  }
  if (strcmp(name, "fpfh_list_bytes") == 0) {
    if (value < 1 || value > kFpfhListBytesMax)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "fpfh_list_bytes must lie in [1, " + std::to_string(kFpfhListBytesMax) + "]");
    h->fpfh_list_bytes = value;
    return TEASER_HIP_OK;
  }
  if (strcmp(name, "knn_fallbacks") == 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "knn_fallbacks is read-only");
  return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string("unknown ICP option ") + name);
}

int32_t teaser_hip_icp_get_option(teaser_hip_icp* h, const char* name, int64_t* value) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (!name || !value) return fail(h, TEASER_HIP_ERR_BAD_ARG, "name / value must not be NULL");
  if (strcmp(name, "knn_ring_cap") == 0) {
    *value = h->knn_ring_cap;
    return TEASER_HIP_OK;
  }
  if (strcmp(name, "knn_fallbacks") == 0) {
    *value = h->knn_fallbacks;
    return TEASER_HIP_OK;
  }
  if (strcmp(name, "fps_resident_max") == 0) {
    *value = h->fps_resident_max;
    return TEASER_HIP_OK;
  }
  if (strcmp(name, "fpfh_list_bytes") == 0) {
    *value = h->fpfh_list_bytes;
    return TEASER_HIP_OK;
  }
  return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string("unknown ICP option ") + name);
}

int32_t teaser_hip_icp_self_knn_batch(teaser_hip_icp* h, int32_t batch, const double* const* points, const int32_t* n,
                                      const int32_t* k, int32_t* const* idx_out, double* const* d2_out) {
  const CallStart c = begin_cloud_call(h, batch, points, n, true);
  if (c.done) return c.rc;
  int64_t slots = 0;
  if (!k) return fail(h, TEASER_HIP_ERR_BAD_ARG, "k must not be NULL");
  for (int b = 0; b < batch; ++b) {
    if (k[b] < 1 || k[b] > kIcpKnnMax)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "k must lie in [1, " + std::to_string(kIcpKnnMax) + "]" + at(b));
    if (n[b] > 0 && (!idx_out || !idx_out[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "idx_out is NULL" + at(b));
    slots += (int64_t)n[b] * k[b];
  }
  if (slots >= INT32_MAX) return fail(h, TEASER_HIP_ERR_BAD_ARG, "too many output slots (sum of n k) in one call");
  if (c.total == 0) return TEASER_HIP_OK;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  IcpIndex ix;
  KnnLayout L;
  int32_t rc = run_self_knn(h, batch, points, n, k, nullptr, ix, L);
  if (rc == TEASER_HIP_OK) rc = copy_back(h, 0, L.bytes, "self k-NN");
  if (rc != TEASER_HIP_OK) return rc;
  read_fallbacks(h, L.counter);
  const char* back = (const char*)h->back.data();
  int64_t off = 0;
  for (int b = 0; b < batch; ++b) {
    const size_t cnt = (size_t)n[b] * (size_t)k[b];
    if (cnt) memcpy(idx_out[b], back + L.idx + sizeof(int32_t) * off, sizeof(int32_t) * cnt);
    if (cnt && d2_out && d2_out[b]) memcpy(d2_out[b], back + L.d2 + sizeof(double) * off, sizeof(double) * cnt);
    off += (int64_t)cnt;
  }
  return TEASER_HIP_OK;
}

int32_t teaser_hip_icp_remove_statistical_outliers_batch(teaser_hip_icp* h, int32_t batch,
                                                         const double* const* points, const int32_t* n,
                                                         const int32_t* nb_neighbors, const double* std_ratio,
                                                         uint8_t* const* keep_out, int32_t* n_kept_out,
                                                         double* const* avg_out, double* stats_out) {
  const CallStart c = begin_cloud_call(h, batch, points, n, true);
  if (c.done) return c.rc;
  if (!nb_neighbors) return fail(h, TEASER_HIP_ERR_BAD_ARG, "nb_neighbors must not be NULL");
  if (!std_ratio) return fail(h, TEASER_HIP_ERR_BAD_ARG, "std_ratio must not be NULL");
  if (!n_kept_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_kept_out must not be NULL");
  for (int b = 0; b < batch; ++b) {
    if (nb_neighbors[b] < 1 || nb_neighbors[b] > kIcpKnnMax)
      return fail(h, TEASER_HIP_ERR_BAD_ARG,
                  "nb_neighbors must lie in [1, " + std::to_string(kIcpKnnMax) + "]" + at(b));
    if (!std::isfinite(std_ratio[b]) || !(std_ratio[b] > 0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "std_ratio must be finite and > 0" + at(b));
    if (n[b] > 0 && (!keep_out || !keep_out[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "keep_out is NULL" + at(b));
  }
  const double kNaN = std::numeric_limits<double>::quiet_NaN();
  for (int b = 0; b < batch; ++b) {  // an empty cloud: nothing kept, no statistics
    n_kept_out[b] = 0;
    if (stats_out) stats_out[3 * b] = stats_out[3 * b + 1] = stats_out[3 * b + 2] = kNaN;
  }
  if (c.total == 0) return TEASER_HIP_OK;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  IcpIndex ix;
  KnnLayout L;
  int32_t rc = run_self_knn(h, batch, points, n, nb_neighbors, std_ratio, ix, L);
  if (rc != TEASER_HIP_OK) return rc;
  DevBuf* B = h->buf;
  char* out = B[B_X].as<char>();
  launch_icp_statistical(h->stream, B[B_DESC].as<IcpDesc>(), B[B_STATE].as<IcpKnnDesc>(), B[B_TBLK].as<int32_t>(),
                         (int)ix.tblk_prob.size(), batch, (const double*)(out + L.avg), B[B_PARTIALS].as<double>(),
                         (double*)(out + L.stats), (uint8_t*)(out + L.keep), (int32_t*)(out + L.ints));
  if ((rc = copy_back(h, 0, L.bytes, "statistical outlier removal")) != TEASER_HIP_OK) return rc;
  read_fallbacks(h, L.counter);
  const char* back = (const char*)h->back.data();
  for (int b = 0; b < batch; ++b) {
    if (n[b] == 0) continue;
    const int64_t o = ix.desc[(size_t)b].t_off;
    memcpy(keep_out[b], back + L.keep + o, (size_t)n[b]);
    memcpy(&n_kept_out[b], back + L.ints + sizeof(int32_t) * b, sizeof(int32_t));
    if (avg_out && avg_out[b]) memcpy(avg_out[b], back + L.avg + sizeof(double) * o, sizeof(double) * n[b]);
    if (stats_out) memcpy(stats_out + 3 * b, back + L.stats + sizeof(double) * 3 * b, sizeof(double) * 3);
  }
  return TEASER_HIP_OK;
}

int32_t teaser_hip_icp_remove_radius_outliers_batch(teaser_hip_icp* h, int32_t batch, const double* const* points,
                                                    const int32_t* n, const int32_t* nb_points, const double* radius,
                                                    uint8_t* const* keep_out, int32_t* n_kept_out,
                                                    int32_t* const* count_out) {
  const CallStart c = begin_cloud_call(h, batch, points, n, false);
  if (c.done) return c.rc;
  if (!nb_points) return fail(h, TEASER_HIP_ERR_BAD_ARG, "nb_points must not be NULL");
  if (!radius) return fail(h, TEASER_HIP_ERR_BAD_ARG, "radius must not be NULL");
  if (!n_kept_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_kept_out must not be NULL");
  for (int b = 0; b < batch; ++b) {
    const double r = radius[b];
    if (!std::isfinite(r) || !(r > 0) || !std::isfinite(r * r) || !(r * r > 0))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "radius (and its square) must be finite and > 0" + at(b));
    if (nb_points[b] < 1) return fail(h, TEASER_HIP_ERR_BAD_ARG, "nb_points must be >= 1" + at(b));
    if (n[b] > 0 && (!keep_out || !keep_out[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "keep_out is NULL" + at(b));
  }
  for (int b = 0; b < batch; ++b) n_kept_out[b] = 0;
  if (c.total == 0) return TEASER_HIP_OK;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  IcpIndex ix;
  std::vector<IcpKnnDesc> knn((size_t)batch);
  for (int b = 0; b < batch; ++b) {
    memset(&knn[(size_t)b], 0, sizeof(IcpKnnDesc));
    knn[(size_t)b].k = nb_points[b];
    add_problem(ix, b, 0, n[b], points, radius[b], (n[b] + kIcpCovBlock - 1) / kIcpCovBlock);
  }
  const int64_t t_off = ix.t_off;
  const int n_tblk = (int)ix.tblk_prob.size();
  // B_X: the counts, the kept counts, the mask bytes
  const size_t o_kept = sizeof(int32_t) * t_off, o_keep = o_kept + sizeof(int32_t) * batch;
  const size_t out_bytes = o_keep + (size_t)t_off;
  size_t bytes[B_COUNT] = {};
  index_bytes(ix, 0, false, bytes);
  bytes[B_STATE] = sizeof(IcpKnnDesc) * batch;
  bytes[B_X] = out_bytes;
  int32_t rc = ensure_buffers(h, bytes, "hipMalloc failed (radius removal buffers)");
  if (rc != TEASER_HIP_OK) return rc;
  DevBuf* B = h->buf;
  char* out = B[B_X].as<char>();
  h->stage.resize((size_t)(3 * t_off));
  if ((rc = upload_inputs(h, ix, nullptr, points, n, knn.data(), bytes[B_STATE])) != TEASER_HIP_OK) return rc;
  FCHK(h, hipMemsetAsync(out + o_kept, 0, sizeof(int32_t) * batch, h->stream), "hipMemsetAsync");
  if ((rc = launch_index(h, ix)) != TEASER_HIP_OK) return rc;
  launch_icp_radius_count(h->stream, B[B_DESC].as<IcpDesc>(), B[B_STATE].as<IcpKnnDesc>(), B[B_TBLK].as<int32_t>(),
                          n_tblk, B[B_Q].as<double>(), B[B_QS].as<double>(), B[B_BSTART].as<int32_t>(),
                          (int32_t*)out, (uint8_t*)(out + o_keep), (int32_t*)(out + o_kept));
  if ((rc = copy_back(h, 0, out_bytes, "radius outlier removal")) != TEASER_HIP_OK) return rc;
  const char* back = (const char*)h->back.data();
  for (int b = 0; b < batch; ++b) {
    if (n[b] == 0) continue;
    const int64_t o = ix.desc[(size_t)b].t_off;
    memcpy(keep_out[b], back + o_keep + o, (size_t)n[b]);
    memcpy(&n_kept_out[b], back + o_kept + sizeof(int32_t) * b, sizeof(int32_t));
    if (count_out && count_out[b]) memcpy(count_out[b], back + sizeof(int32_t) * o, sizeof(int32_t) * n[b]);
  }
  return TEASER_HIP_OK;
}

}  // extern "C"
