// voxel.hip -- host side of the batched voxel down-sampling (include/teaser_hip.h, "Voxel down-sampling"): its own
// handle, argument validation with the per-problem bounds, the key layout, and the launch sequence of
// kernels_voxel.hip.
//
// The host reads every coordinate once anyway (non-finite points are refused), so the exact per-problem min / max
// comes from that same pass: the bounds decide the key layout (bits per axis, one or two sort passes) before anything
// is launched.  One call = one H2D copy per problem, the launches, one small copy of the per-problem run counts, then
// the copies of the outputs.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <climits>
#include <string>
#include <vector>

#include "host_common.h"
#include "teaser_hip.h"
#include "voxel_internal.h"

using namespace thip;

namespace {

enum { B_DESC, B_BLK, B_PTS, B_KEY_LO, B_KEY_HI, B_IOTA, B_SORTED, B_GATHERED, B_PERM1, B_PERM, B_SPTS, B_HEAD,
       B_RUN_ID, B_RUN_START, B_SUMMARY, B_MEAN, B_COUNT, B_TRACE, B_TEMP, B_COUNT_OF_BUFS };

}  // namespace

struct teaser_hip_voxel : HandleBase {
  DevBuf buf[B_COUNT_OF_BUFS];
};

namespace {

// Number of bits that hold every value in [0, v].
int bits_for(uint64_t v) {
  int b = 0;
  while (b < 64 && (v >> b) != 0) ++b;
  return b;
}

// Validates the arguments and fills lo (min_bound - v / 2) and the largest voxel index per axis of every non-empty
// problem.
int32_t validate(teaser_hip_voxel* h, int32_t batch, const double* const* pts, const int32_t* n,
                 const double* voxel_size, double* const* out, int64_t* n_out, std::vector<VoxDesc>& desc,
                 std::vector<uint64_t>& max_index) {
  if (batch < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0");
  if (batch == 0) return TEASER_HIP_OK;
  if (!n) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must not be NULL");
  if (!voxel_size) return fail(h, TEASER_HIP_ERR_BAD_ARG, "voxel_size must not be NULL");
  if (!n_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_out must not be NULL");
  desc.assign((size_t)batch, VoxDesc{});
  max_index.assign(3 * (size_t)batch, 0);
  int64_t total = 0;
  for (int b = 0; b < batch; ++b) {
    const double v = voxel_size[b];
    if (!std::isfinite(v) || !(v > 0)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "voxel_size must be finite and > 0" + at(b));
    if (n[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must be >= 0" + at(b));
    VoxDesc& d = desc[(size_t)b];
    d.off = total;
    d.n = n[b];
    d.v = v;
    total += n[b];
    if (n[b] == 0) continue;
    if (!pts || !pts[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "points is NULL" + at(b));
    if (!out || !out[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "out is NULL" + at(b));
    const double* p = pts[b];
    double mn[3], mx[3];
    for (int c = 0; c < 3; ++c) mn[c] = mx[c] = p[c];
    bool finite = true;
    for (int64_t i = 0; i < n[b]; ++i)
      for (int c = 0; c < 3; ++c) {
        const double x = p[3 * i + c];
        finite &= std::isfinite(x);
        mn[c] = std::min(mn[c], x);
        mx[c] = std::max(mx[c], x);
      }
    if (!finite) return fail(h, TEASER_HIP_ERR_BAD_ARG, "points has a non-finite coordinate" + at(b));
    // Open3D's guard: the grid must be indexable with 32-bit voxel indices
    double span = 0;
    for (int c = 0; c < 3; ++c) {
      d.lo[c] = mn[c] - 0.5 * v;
      span = std::max(span, (mx[c] + 0.5 * v) - d.lo[c]);
    }
    if (v * (double)INT_MAX < span)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "voxel_size is too small for 32-bit voxel indices" + at(b));
    for (int c = 0; c < 3; ++c) max_index[3 * (size_t)b + c] = vox_index(mx[c], d.lo[c], v);
  }
  if (total >= INT32_MAX) return fail(h, TEASER_HIP_ERR_BAD_ARG, "too many points in one call");
  return TEASER_HIP_OK;
}

}  // namespace

extern "C" {

int32_t teaser_hip_voxel_create(int32_t device, teaser_hip_voxel** out) { return open_handle(device, out); }

int32_t teaser_hip_voxel_destroy(teaser_hip_voxel* h) { return close_handle(h); }

const char* teaser_hip_voxel_last_error(const teaser_hip_voxel* h) { return h ? h->err.c_str() : ""; }

int32_t teaser_hip_voxel_fill_scratch(teaser_hip_voxel* h, int32_t byte, int64_t* bytes_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  ScratchSpan spans[B_COUNT_OF_BUFS];
  for (int k = 0; k < B_COUNT_OF_BUFS; ++k) spans[k] = span_of(h->buf[k]);
  return fill_scratch(h, byte, spans, B_COUNT_OF_BUFS, bytes_out);
}

int32_t teaser_hip_voxel_down_sample_batch(teaser_hip_voxel* h, int32_t batch, const double* const* pts,
                                           const int32_t* n, const double* voxel_size, double* const* out,
                                           int64_t* n_out, int32_t* const* counts, int32_t* const* voxel_of_point) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  std::vector<VoxDesc> desc;
  std::vector<uint64_t> max_index;
  int32_t rc = validate(h, batch, pts, n, voxel_size, out, n_out, desc, max_index);
  if (rc != TEASER_HIP_OK || batch == 0) return rc;
  for (int b = 0; b < batch; ++b) n_out[b] = 0;

  // ---- key layout: i_z at bit 0, then i_y, i_x with each problem's own widths; the problem index above the
  // widest problem ----
  std::vector<int32_t> blk_prob;
  int key_bits = 0;
  for (int b = 0; b < batch; ++b) {
    VoxDesc& d = desc[(size_t)b];
    d.blk_off = (int32_t)blk_prob.size();
    for (int k = 0; k < (d.n + kVoxBlock - 1) / kVoxBlock; ++k) blk_prob.push_back(b);
    if (d.n == 0) continue;
    const int bx = bits_for(max_index[3 * (size_t)b]), by = bits_for(max_index[3 * (size_t)b + 1]),
              bz = bits_for(max_index[3 * (size_t)b + 2]);
    d.shift[2] = 0;
    d.shift[1] = bz;
    d.shift[0] = by + bz;
    key_bits = std::max(key_bits, bx + by + bz);
  }
  const int64_t total = desc.back().off + desc.back().n;
  if (total == 0) return TEASER_HIP_OK;
  const int prob_shift = key_bits;
  const int bits = std::max(1, key_bits + bits_for((uint64_t)(batch - 1)));  // <= 3 * 32 + 31 < 128
  const bool two_words = bits > 64;
  const int n_blk = (int)blk_prob.size();

  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  const size_t N = (size_t)total;
  const size_t bytes[B_COUNT_OF_BUFS] = {
      sizeof(VoxDesc) * batch, sizeof(int32_t) * n_blk, 24 * N, 8 * N, two_words ? 8 * N : 8,
      4 * N, 8 * N, two_words ? 8 * N : 8, two_words ? 4 * N : 4, 4 * N, 24 * N, 4 * N,
      4 * N, 4 * (N + 1), 8 * (size_t)batch, 24 * N, 4 * N, 4 * N, voxel_sort_temp_bytes(total)};
  for (int k = 0; k < B_COUNT_OF_BUFS; ++k)
    if (!h->buf[k].ensure(bytes[k])) return fail(h, TEASER_HIP_ERR_OOM, "hipMalloc failed (voxel buffers)");
  hipStream_t s = h->stream;
  DevBuf* B = h->buf;

  FCHK(h, hipMemcpyAsync(B[B_DESC].p, desc.data(), bytes[B_DESC], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (descriptors)");
  FCHK(h, hipMemcpyAsync(B[B_BLK].p, blk_prob.data(), bytes[B_BLK], hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (descriptors)");
  for (int b = 0; b < batch; ++b)
    if (n[b] > 0)
      FCHK(h, hipMemcpyAsync(B[B_PTS].as<double>() + 3 * desc[(size_t)b].off, pts[b], 24 * (size_t)n[b],
                             hipMemcpyHostToDevice, s),
           "hipMemcpyAsync (points)");

  // ---- keys, sort, runs, sums ----
  launch_voxel_keys(s, B[B_DESC].as<VoxDesc>(), B[B_BLK].as<int32_t>(), n_blk, B[B_PTS].as<double>(), prob_shift,
                    B[B_KEY_LO].as<uint64_t>(), two_words ? B[B_KEY_HI].as<uint64_t>() : nullptr,
                    B[B_IOTA].as<int32_t>());
  FCHK(h, launch_voxel_sort(s, B[B_TEMP].p, bytes[B_TEMP], total, bits, B[B_KEY_LO].as<uint64_t>(),
                            B[B_KEY_HI].as<uint64_t>(), B[B_IOTA].as<int32_t>(), B[B_SORTED].as<uint64_t>(),
                            B[B_GATHERED].as<uint64_t>(), B[B_PERM1].as<int32_t>(), B[B_PERM].as<int32_t>()),
       "voxel sort");
  FCHK(h, launch_voxel_runs(s, B[B_TEMP].p, bytes[B_TEMP], total, two_words, B[B_PTS].as<double>(),
                            B[B_KEY_LO].as<uint64_t>(), B[B_KEY_HI].as<uint64_t>(), B[B_PERM].as<int32_t>(),
                            B[B_SPTS].as<double>(), B[B_HEAD].as<int32_t>(), B[B_RUN_ID].as<int32_t>(),
                            B[B_RUN_START].as<int32_t>()),
       "voxel runs");
  launch_voxel_reduce(s, B[B_DESC].as<VoxDesc>(), batch, total, B[B_RUN_ID].as<int32_t>(),
                      B[B_RUN_START].as<int32_t>(), B[B_SPTS].as<double>(), B[B_SUMMARY].as<int32_t>(),
                      B[B_MEAN].as<double>(), B[B_COUNT].as<int32_t>());
  bool want_trace = false, want_counts = false;
  for (int b = 0; b < batch; ++b) {
    want_trace |= voxel_of_point && voxel_of_point[b] && n[b] > 0;
    want_counts |= counts && counts[b] && n[b] > 0;
  }
  if (want_trace)
    launch_voxel_trace(s, B[B_DESC].as<VoxDesc>(), B[B_BLK].as<int32_t>(), n_blk, B[B_PERM].as<int32_t>(),
                       B[B_RUN_ID].as<int32_t>(), B[B_SUMMARY].as<int32_t>(), B[B_TRACE].as<int32_t>());
  FCHK(h, hipGetLastError(), "voxel kernel launch");

  // ---- results: run counts first, then exactly the voxels ----
  std::vector<int32_t> summary(2 * (size_t)batch);
  FCHK(h, hipMemcpyAsync(summary.data(), B[B_SUMMARY].p, bytes[B_SUMMARY], hipMemcpyDeviceToHost, s),
       "voxel run counts");
  FCHK(h, hipStreamSynchronize(s), "voxel run counts");
  int64_t runs = 0;
  for (int b = 0; b < batch; ++b) runs += summary[2 * (size_t)b + 1];
  std::vector<double> mean(3 * (size_t)runs);
  std::vector<int32_t> count(want_counts ? (size_t)runs : 0), trace(want_trace ? N : 0);
  FCHK(h, hipMemcpyAsync(mean.data(), B[B_MEAN].p, 24 * (size_t)runs, hipMemcpyDeviceToHost, s),
       "hipMemcpyAsync (voxels)");
  if (want_counts)
    FCHK(h, hipMemcpyAsync(count.data(), B[B_COUNT].p, 4 * (size_t)runs, hipMemcpyDeviceToHost, s),
         "hipMemcpyAsync (counts)");
  if (want_trace)
    FCHK(h, hipMemcpyAsync(trace.data(), B[B_TRACE].p, 4 * N, hipMemcpyDeviceToHost, s),
         "hipMemcpyAsync (voxel_of_point)");
  FCHK(h, hipStreamSynchronize(s), "voxel results");
  for (int b = 0; b < batch; ++b) {
    const int64_t first = summary[2 * (size_t)b], m = summary[2 * (size_t)b + 1];
    n_out[b] = m;
    if (m > 0) memcpy(out[b], mean.data() + 3 * first, 24 * (size_t)m);
    if (want_counts && counts[b] && m > 0) memcpy(counts[b], count.data() + first, 4 * (size_t)m);
    if (want_trace && voxel_of_point[b] && n[b] > 0)
      memcpy(voxel_of_point[b], trace.data() + desc[(size_t)b].off, 4 * (size_t)n[b]);
  }
  return TEASER_HIP_OK;
}

int32_t teaser_hip_voxel_down_sample(teaser_hip_voxel* h, const double* pts, int32_t n, double voxel_size,
                                     double* out, int64_t* n_out, int32_t* counts, int32_t* voxel_of_point) {
  double* const outs[1] = {out};
  int32_t* const cs[1] = {counts};
  int32_t* const vs[1] = {voxel_of_point};
  return teaser_hip_voxel_down_sample_batch(h, 1, &pts, &n, &voxel_size, outs, n_out, cs, vs);
}

}  // extern "C"
