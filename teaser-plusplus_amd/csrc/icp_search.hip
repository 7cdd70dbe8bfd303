// icp_search.hip -- host side of the neighbour search between two clouds on the ICP handle (include/teaser_hip.h,
// "Neighbour search"): k-NN, hybrid and uncapped radius search of a query set in a data cloud.
// Kernels: kernels_search.hip; design, launch counts and bounds in DESIGN.md section 28.
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

// n, the pointers and the coordinates of one side (`name`: "data" or "query"); *total = its number of points.
int32_t check_side(teaser_hip_icp* h, int32_t batch, const double* const* pts, const int32_t* n, const char* name,
                   int64_t* total) {
  const std::string s(name);
  *total = 0;
  if (!n) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_" + s + " must not be NULL");
  for (int b = 0; b < batch; ++b) {
    if (n[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_" + s + " must be >= 0" + at(b));
    if (n[b] > 0 && (!pts || !pts[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, s + " is NULL" + at(b));
    if (n[b] > 0 && !finite_points(pts[b], n[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, s + " has a non-finite coordinate" + at(b));
    *total += n[b];
  }
  return TEASER_HIP_OK;
}

// How a two-cloud call begins (begin_cloud_call for two sides): the handle, its cleared error and fallback count,
// batch, and both sides.  done: the entry point returns rc at once; else n_q / n_d = the number of queries / data points.
struct SearchStart {
  int32_t rc;
  bool done;
  int64_t n_q, n_d;
};
SearchStart begin_search_call(teaser_hip_icp* h, int32_t batch, const double* const* data, const int32_t* n_data,
                              const double* const* query, const int32_t* n_query) {
  if (!h) return {TEASER_HIP_ERR_BAD_ARG, true, 0, 0};
  h->err.clear();
  h->knn_fallbacks = 0;
  if (batch < 0) return {fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0"), true, 0, 0};
  if (batch == 0) return {TEASER_HIP_OK, true, 0, 0};
  SearchStart c = {TEASER_HIP_OK, false, 0, 0};
  c.rc = check_side(h, batch, data, n_data, "data", &c.n_d);
  if (c.rc == TEASER_HIP_OK) c.rc = check_side(h, batch, query, n_query, "query", &c.n_q);
  if (c.rc == TEASER_HIP_OK && c.n_d + c.n_q >= INT32_MAX / 9)
    c.rc = fail(h, TEASER_HIP_ERR_BAD_ARG, "too many points in one call");
  c.done = c.rc != TEASER_HIP_OK;
  return c;
}

bool radius_positive(double r) { return std::isfinite(r) && r > 0 && std::isfinite(r * r) && r * r > 0; }

// Buffers, uploads and the index build of one call whose problems are in ix / sd; B_X holds `x_bytes` (the packed
// queries first).  `match_bytes`: the worklist of the k-NN search.
int32_t stage_search(teaser_hip_icp* h, const IcpIndex& ix, const std::vector<IcpSearchDesc>& sd,
                     const double* const* data, const int32_t* n_data, const double* const* query, size_t x_bytes,
                     size_t match_bytes, size_t tmp_bytes, const char* oom) {
  size_t bytes[B_COUNT] = {};
  index_bytes(ix, 1, false, bytes);
  bytes[B_STATE] = sizeof(IcpSearchDesc) * sd.size();
  bytes[B_X] = x_bytes;
  bytes[B_MATCH] = match_bytes;
  bytes[B_SEARCH_TMP] = tmp_bytes;
  int32_t rc = ensure_buffers(h, bytes, oom);
  if (rc != TEASER_HIP_OK) return rc;
  h->stage.resize((size_t)(3 * (ix.s_off + ix.t_off)));
  if ((rc = upload_inputs(h, ix, query, data, n_data, sd.data(), bytes[B_STATE])) != TEASER_HIP_OK) return rc;
  return launch_index(h, ix);
}

// k-NN (radius NULL) and hybrid search share everything but the grid, the launch and the counts.
int32_t search_rows(teaser_hip_icp* h, int32_t batch, const double* const* data, const int32_t* n_data,
                    const double* const* query, const int32_t* n_query, const int32_t* k, const char* k_name,
                    const double* radius, int32_t* const* idx_out, double* const* d2_out, int32_t* const* count_out) {
  const SearchStart c = begin_search_call(h, batch, data, n_data, query, n_query);
  if (c.done) return c.rc;
  const std::string kn(k_name);
  if (!k) return fail(h, TEASER_HIP_ERR_BAD_ARG, kn + " must not be NULL");
  int64_t slots = 0;
  for (int b = 0; b < batch; ++b) {
    if (k[b] < 1 || k[b] > kIcpKnnMax)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, kn + " must lie in [1, " + std::to_string(kIcpKnnMax) + "]" + at(b));
    if (n_query[b] > 0 && (!idx_out || !idx_out[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "idx_out is NULL" + at(b));
    slots += (int64_t)n_query[b] * k[b];
  }
  if (slots >= INT32_MAX)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "too many output slots (sum of n_query " + kn + ") in one call");
  if (c.n_q == 0) return TEASER_HIP_OK;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  IcpIndex ix;
  std::vector<IcpSearchDesc> sd((size_t)batch);
  int top = 0;
  slots = 0;
  for (int b = 0; b < batch; ++b) {
    IcpSearchDesc& s = sd[(size_t)b];
    memset(&s, 0, sizeof(s));
    s.k = k[b];
    s.ring_cap = h->knn_ring_cap;
    s.out_off = slots;
    s.edge = 1.0;
    double r = radius ? radius[b] : 1.0;
    if (!radius && n_data[b] > 0) {
      bool rings_ok = true;
      r = s.edge = knn_edge(data[b], n_data[b], std::min(k[b], n_data[b]), &rings_ok);
      if (!rings_ok) s.ring_cap = 0;
    }
    top = std::max(top, radius ? k[b] : std::min(k[b], n_data[b]));
    add_problem(ix, b, n_query[b], n_data[b], data, r, (n_query[b] + kIcpCovBlock - 1) / kIcpCovBlock);
    slots += (int64_t)n_query[b] * k[b];
  }
  // B_X: the queries; then, copied back in one piece: d2, the worklist counter (padded to 8 bytes), idx, the counts
  const size_t o_d2 = sizeof(double) * 3 * (size_t)ix.s_off, o_counter = o_d2 + sizeof(double) * slots;
  const size_t o_idx = o_counter + 8, o_cnt = o_idx + sizeof(int32_t) * slots;
  const size_t end = o_cnt + (radius ? sizeof(int32_t) * (size_t)ix.s_off : 0);
  int32_t rc = stage_search(h, ix, sd, data, n_data, query, end, radius ? 0 : sizeof(int32_t) * 2 * (size_t)ix.s_off, 0,
                            "hipMalloc failed (neighbour search buffers)");
  if (rc != TEASER_HIP_OK) return rc;
  DevBuf* B = h->buf;
  char* out = B[B_X].as<char>();
  const int n_blk = (int)ix.blk_prob.size();
  if (radius) {
    launch_icp_search_hybrid(h->stream, B[B_DESC].as<IcpDesc>(), B[B_STATE].as<IcpSearchDesc>(), B[B_BLK].as<int32_t>(),
                             n_blk, top, (const double*)out, B[B_QS].as<double>(), B[B_QJ].as<int32_t>(),
                             B[B_BSTART].as<int32_t>(), (int32_t*)(out + o_idx), (double*)(out + o_d2),
                             (int32_t*)(out + o_cnt));
  } else {
    FCHK(h, hipMemsetAsync(out + o_counter, 0, 8, h->stream), "hipMemsetAsync");
    launch_icp_search_knn(h->stream, B[B_DESC].as<IcpDesc>(), B[B_STATE].as<IcpSearchDesc>(), B[B_BLK].as<int32_t>(),
                          n_blk, top, (const double*)out, B[B_Q].as<double>(), B[B_QS].as<double>(),
                          B[B_QJ].as<int32_t>(), B[B_BSTART].as<int32_t>(), (int32_t*)(out + o_idx),
                          (double*)(out + o_d2), B[B_MATCH].as<int32_t>(), (int32_t*)(out + o_counter));
  }
  if ((rc = copy_back(h, o_d2, end - o_d2, radius ? "hybrid search" : "k-NN search",
                      "kernel launch (neighbour search)")) != TEASER_HIP_OK)
    return rc;
  if (!radius) read_fallbacks(h, o_counter - o_d2);
  const char* back = (const char*)h->back.data();  // begins at o_d2 of B_X
  int64_t off = 0;
  for (int b = 0; b < batch; ++b) {
    const size_t cnt = (size_t)n_query[b] * (size_t)k[b];
    if (cnt) memcpy(idx_out[b], back + (o_idx - o_d2) + sizeof(int32_t) * off, sizeof(int32_t) * cnt);
    if (cnt && d2_out && d2_out[b]) memcpy(d2_out[b], back + sizeof(double) * off, sizeof(double) * cnt);
    if (cnt && count_out && count_out[b])
      memcpy(count_out[b], back + (o_cnt - o_d2) + sizeof(int32_t) * ix.desc[(size_t)b].s_off, sizeof(int32_t) * n_query[b]);
    off += (int64_t)cnt;
  }
  return TEASER_HIP_OK;
}

}  // namespace

extern "C" {

int32_t teaser_hip_icp_knn_search_batch(teaser_hip_icp* h, int32_t batch, const double* const* data,
                                        const int32_t* n_data, const double* const* query, const int32_t* n_query,
                                        const int32_t* k, int32_t* const* idx_out, double* const* d2_out) {
  return search_rows(h, batch, data, n_data, query, n_query, k, "k", nullptr, idx_out, d2_out, nullptr);
}

int32_t teaser_hip_icp_hybrid_search_batch(teaser_hip_icp* h, int32_t batch, const double* const* data,
                                           const int32_t* n_data, const double* const* query, const int32_t* n_query,
                                           const double* radius, const int32_t* max_nn, int32_t* const* idx_out,
                                           double* const* d2_out, int32_t* const* count_out) {
  if (h && batch > 0) {
    h->err.clear();
    if (!radius) return fail(h, TEASER_HIP_ERR_BAD_ARG, "radius must not be NULL");
    for (int b = 0; b < batch; ++b)
      if (!radius_positive(radius[b]))
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "radius (and its square) must be finite and > 0" + at(b));
  }
  return search_rows(h, batch, data, n_data, query, n_query, max_nn, "max_nn", radius, idx_out, d2_out, count_out);
}

int32_t teaser_hip_icp_radius_search_batch(teaser_hip_icp* h, int32_t batch, const double* const* data,
                                           const int32_t* n_data, const double* const* query, const int32_t* n_query,
                                           const double* radius, const int64_t* capacity, int32_t* const* count_out,
                                           int32_t* const* idx_out, double* const* d2_out, int64_t* total_out) {
  const SearchStart c = begin_search_call(h, batch, data, n_data, query, n_query);
  if (c.done) return c.rc;
  if (!radius) return fail(h, TEASER_HIP_ERR_BAD_ARG, "radius must not be NULL");
  if (!total_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "total_out must not be NULL");
  for (int b = 0; b < batch; ++b) {
    if (!radius_positive(radius[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "radius (and its square) must be finite and > 0" + at(b));
    if (n_query[b] > 0 && (!count_out || !count_out[b]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "count_out is NULL" + at(b));
    if (idx_out && idx_out[b] && !capacity)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "capacity is NULL although idx_out is given" + at(b));
    if (capacity && capacity[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "capacity must be >= 0" + at(b));
  }
  for (int b = 0; b < batch; ++b) total_out[b] = 0;
  if (c.n_q == 0) return TEASER_HIP_OK;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  IcpIndex ix;
  std::vector<IcpSearchDesc> sd((size_t)batch);
  int64_t entries = 0;  // reserved on the device: per filled problem min(capacity, n_query n_data) >= its total
  for (int b = 0; b < batch; ++b) {
    IcpSearchDesc& s = sd[(size_t)b];
    memset(&s, 0, sizeof(s));
    s.fill = idx_out && idx_out[b] ? 1 : 0;
    s.capacity = capacity ? capacity[b] : 0;
    s.out_off = entries;
    if (s.fill) entries += std::min<int64_t>(s.capacity, (int64_t)n_query[b] * n_data[b]);
    add_problem(ix, b, n_query[b], n_data[b], data, radius[b], (n_query[b] + 255) / 256);
  }
  if (entries >= ((int64_t)1 << 38))  // 12 bytes each, twice: beyond any device, and beyond the rank launch's grid
    return fail(h, TEASER_HIP_ERR_OOM, "hipMalloc failed (radius search buffers)");
  // B_X: the queries; then, copied back in one piece: d2 (entries), the totals, the counts, idx (entries); then the
  // prefix sums, which stay on the device
  const size_t o_d2 = sizeof(double) * 3 * (size_t)ix.s_off, o_total = o_d2 + sizeof(double) * entries;
  const size_t o_count = o_total + sizeof(int64_t) * batch, o_idx = o_count + sizeof(int32_t) * (size_t)ix.s_off;
  const size_t end = o_idx + sizeof(int32_t) * entries, o_prefix = (end + 7) / 8 * 8;
  const size_t x_bytes = o_prefix + sizeof(int64_t) * (size_t)ix.s_off;
  int32_t rc = stage_search(h, ix, sd, data, n_data, query, x_bytes, 0, 12 * (size_t)entries,
                            "hipMalloc failed (radius search buffers)");
  if (rc != TEASER_HIP_OK) return rc;
  DevBuf* B = h->buf;
  char* out = B[B_X].as<char>();
  double* tmp_d2 = B[B_SEARCH_TMP].as<double>();
  launch_icp_search_radius(h->stream, B[B_DESC].as<IcpDesc>(), B[B_STATE].as<IcpSearchDesc>(), B[B_BLK].as<int32_t>(),
                           (int)ix.blk_prob.size(), batch, entries, (const double*)out, B[B_QS].as<double>(),
                           B[B_QJ].as<int32_t>(), B[B_BSTART].as<int32_t>(), (int32_t*)(out + o_count),
                           (int64_t*)(out + o_prefix), (int64_t*)(out + o_total), tmp_d2,
                           entries ? (int32_t*)(tmp_d2 + entries) : nullptr, (int32_t*)(out + o_idx),
                           (double*)(out + o_d2));
  if ((rc = copy_back(h, o_d2, end - o_d2, "radius search", "kernel launch (neighbour search)")) != TEASER_HIP_OK)
    return rc;
  const char* back = (const char*)h->back.data();  // begins at o_d2 of B_X
  memcpy(total_out, back + (o_total - o_d2), sizeof(int64_t) * batch);
  for (int b = 0; b < batch; ++b) {
    const IcpSearchDesc& s = sd[(size_t)b];
    if (n_query[b])
      memcpy(count_out[b], back + (o_count - o_d2) + sizeof(int32_t) * ix.desc[(size_t)b].s_off, sizeof(int32_t) * n_query[b]);
    const int64_t tot = total_out[b];
    if (!s.fill || s.capacity < tot || tot == 0) continue;  // the count half only: the arrays are not touched
    memcpy(idx_out[b], back + (o_idx - o_d2) + sizeof(int32_t) * s.out_off, sizeof(int32_t) * tot);
    if (d2_out && d2_out[b]) memcpy(d2_out[b], back + sizeof(double) * s.out_off, sizeof(double) * tot);
  }
  return TEASER_HIP_OK;
}

}  // extern "C"
