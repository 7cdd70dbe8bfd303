// features.hip -- host side of the correspondence front-end (include/teaser_hip.h, "Batched correspondence
// front-end"): its own handle, argument validation, the descriptor tables and the launch sequence of the kernels of
// kernels_features.hip.  The only one: teaser_hip_compute_fpfh and teaser_hip_match_features (solver.hip) come here
// with a batch of one.
//
// FPFH of a batch of clouds.  The points of all clouds are packed one after the other; every radius block and every
// point finds its cloud through a block -> cloud / point -> cloud map and the descriptor table.
//   1. count pass for BOTH radii over the whole batch, one scan workgroup per cloud and radius, then ONE small copy of
//      {list total, longest list} per cloud and radius and the first host synchronisation;
//   2. the host cuts the clouds into waves whose lists fit the list budget (one wave, normally), sizes the list buffer
//      once, uploads the list base of every cloud and turns the cloud-local offsets into 64-bit offsets into the
//      wave's list;
//   3. per wave, stream-ordered and without a host round trip: fill + sort of the normal-radius lists, normals; then
//      per wave fill + sort of the FPFH-radius lists, SPFH, FPFH;
//   4. the copies of the outputs and the second (last) synchronisation.
// Matching a batch of feature pairs: two 1-nearest searches per pair, the searches of all pairs in one launch sequence
// (run_knn with k = 1), the results of all searches in one copy, one synchronisation, then the O(n) index bookkeeping
// per pair on the host.  A call therefore waits for the stream (hipStreamSynchronize) 2 times (FPFH, clouds ->
// correspondences) or once (matching), whatever the batch and the number of waves.  The k-NN calls (knn_batch,
// match_knn_batch, correspondences_knn_batch) keep that contract: the searches of all problems through the same
// run_knn, the device-side mutual filter, one copy of the lists and the keep mask, one synchronisation, then the
// O(n k) pair writing on the host.  Features and normals the caller asked
// for, and the features the matching calls take from the host, are copied per problem between the device and the
// caller's own (pageable) arrays: those copies are additional.
#include <math.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <climits>
#include <string>
#include <vector>

#include "features_internal.h"
#include "host_common.h"
#include "internal.h"
#include "teaser_hip.h"

using namespace thip;

namespace {

// Neighbour lists (8 bytes per neighbour) of one wave of clouds; a wave always holds at least one cloud.  The rank
// sort of lists longer than the LDS sort's capacity needs a scratch copy of the same size when it is used.
constexpr int64_t kFeatListBudgetBytes = (int64_t)4 << 30;
// Partial results (8 bytes per query, data chunk and list slot) of one wave of searches.
constexpr int64_t kFeatPartBudgetBytes = (int64_t)1 << 30;

enum { B_DESC, B_BLK, B_PT_CLOUD, B_PTS, B_COUNTS, B_OFFSETS, B_CURSOR, B_META, B_BASE, B_LIST, B_LIST2, B_NORMALS,
       B_SPFH, B_FEAT, B_SEARCH, B_SBLK, B_PART_D, B_PART_I, B_MFEAT, B_KNN_I, B_KNN_D, B_KNN_KEEP,
       B_TUPLE_DESC, B_TUPLE_BLK, B_TUPLE_PAIRS, B_TUPLE_KEEP, B_COUNT_OF_BUFS };
enum { H_PTS, H_META, H_KNN_I, H_KNN_D, H_KNN_KEEP, H_TUPLE_PAIRS, H_TUPLE_KEEP, H_COUNT_OF_BUFS };

struct Wave {
  int c0, c1;  // clouds (or searches) [c0, c1)
};

// One nearest-neighbour search of a call: both sides non-empty, rows of the packed feature array.
struct KnnSearch {
  int64_t data_row, query_row;
  int32_t nd, nq;
};

}  // namespace

struct teaser_hip_features : HandleBase {
  DevBuf buf[B_COUNT_OF_BUFS];
  HostBuf host[H_COUNT_OF_BUFS];  // the packed points going in, the small data-dependent results coming back
  int64_t list_budget = kFeatListBudgetBytes;
  int64_t part_budget = kFeatPartBudgetBytes;
  // host tables of the call in flight (kept here so that they outlive their asynchronous uploads)
  std::vector<FeatCloudDesc> desc;
  std::vector<int32_t> blk_cloud, pt_cloud, blk_search;
  std::vector<int64_t> base;
  std::vector<FeatSearchDesc> search;
  std::vector<FeatTupleDesc> tuple;
  std::vector<int32_t> blk_tuple;
};

namespace {

#define FENSURE(h, b, bytes) \
  do {                       \
    if (!(b).ensure(bytes)) return fail((h), TEASER_HIP_ERR_OOM, "allocation failed (front-end buffers)"); \
  } while (0)

// The batched entry points' rule for the radii of `batch` problems: finite, > 0, and the float square the kernels
// compare with neither 0 nor inf.  (Not in validate_clouds: teaser_hip_compute_fpfh keeps its older rule, > 0.)
int32_t check_radii(teaser_hip_features* h, int32_t batch, const double* normal_radius, const double* fpfh_radius) {
  if (!normal_radius) return fail(h, TEASER_HIP_ERR_BAD_ARG, "normal_radius must not be NULL");
  if (!fpfh_radius) return fail(h, TEASER_HIP_ERR_BAD_ARG, "fpfh_radius must not be NULL");
  for (int b = 0; b < batch; ++b)
    for (int w = 0; w < 2; ++w) {
      const double v = (w ? fpfh_radius : normal_radius)[b];
      const float r2 = (float)(v * v);
      if (!std::isfinite(v) || !(v > 0) || !std::isfinite(r2) || !(r2 > 0))
        return fail(h, TEASER_HIP_ERR_BAD_ARG,
                    std::string(w ? "fpfh_radius" : "normal_radius") + " must be finite and > 0" + at(b));
    }
  return TEASER_HIP_OK;
}

// Checks `nc` clouds (problem index reported = c / per_problem) and builds the descriptor tables.
int32_t validate_clouds(teaser_hip_features* h, int nc, int per_problem, const float* const* cloud, const char* const* names,
                        const int32_t* const* n, const double* normal_radius, const double* fpfh_radius) {
  h->desc.assign((size_t)nc, FeatCloudDesc{});
  int64_t total = 0, blocks = 0;
  const int chunk = feat_radius_chunk();
  for (int c = 0; c < nc; ++c) {
    const int b = c / per_problem, side = c % per_problem;
    const int32_t nb = n[side][b];
    if (nb < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string("n must be >= 0 for ") + names[side] + at(b));
    if (nb > 0 && (!cloud || !cloud[c]))
      return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string(names[side]) + " is NULL" + at(b));
    FeatCloudDesc& d = h->desc[(size_t)c];
    d.off = total;
    d.n = nb;
    d.blk_off = (int32_t)blocks;
    d.qblocks = (nb + 63) / 64;
    d.r2[0] = (float)(normal_radius[b] * normal_radius[b]);  // pcl::KdTreeFLANN::radiusSearch: static_cast<float>(r * r)
    d.r2[1] = (float)(fpfh_radius[b] * fpfh_radius[b]);
    total += nb;
    blocks += (int64_t)d.qblocks * ((nb + chunk - 1) / chunk);
    if (total >= INT32_MAX || blocks >= INT32_MAX)
      return fail(h, TEASER_HIP_ERR_UNSUPPORTED, "too many points in one call" + at(b));
  }
  return TEASER_HIP_OK;
}

int64_t cloud_blocks(const FeatCloudDesc& d) {
  const int chunk = feat_radius_chunk();
  return (int64_t)d.qblocks * ((d.n + chunk - 1) / chunk);
}

// FPFH of the clouds described by h->desc (cloud[c]: n x 3 floats): features in B_FEAT, normals in B_NORMALS, packed.
// One host synchronisation; everything after it is only enqueued.
int32_t run_fpfh(teaser_hip_features* h, const float* const* cloud) {
  const int nc = (int)h->desc.size();
  const int64_t T = nc ? h->desc.back().off + h->desc.back().n : 0;
  if (T == 0) return TEASER_HIP_OK;
  const int n_blk = (int)(h->desc.back().blk_off + cloud_blocks(h->desc.back()));
  hipStream_t s = h->stream;
  DevBuf* B = h->buf;

  h->blk_cloud.resize((size_t)n_blk);
  h->pt_cloud.resize((size_t)T);
  for (int c = 0; c < nc; ++c) {
    const FeatCloudDesc& d = h->desc[(size_t)c];
    std::fill_n(h->blk_cloud.begin() + d.blk_off, cloud_blocks(d), c);
    std::fill_n(h->pt_cloud.begin() + d.off, d.n, c);
  }
  FENSURE(h, B[B_DESC], sizeof(FeatCloudDesc) * (size_t)nc);
  FENSURE(h, B[B_BLK], 4 * (size_t)n_blk);
  FENSURE(h, B[B_PT_CLOUD], 4 * (size_t)T);
  FENSURE(h, B[B_PTS], 12 * (size_t)T);
  FENSURE(h, B[B_COUNTS], 2 * 4 * (size_t)T);
  FENSURE(h, B[B_OFFSETS], 2 * 8 * (size_t)T);
  FENSURE(h, B[B_CURSOR], 4 * (size_t)T);
  FENSURE(h, B[B_META], 2 * 16 * (size_t)nc);
  FENSURE(h, B[B_BASE], 2 * 8 * (size_t)nc);
  FENSURE(h, B[B_NORMALS], 12 * (size_t)T);
  FENSURE(h, B[B_SPFH], 33 * 4 * (size_t)T);
  FENSURE(h, B[B_FEAT], 33 * 4 * (size_t)T);
  FENSURE(h, h->host[H_PTS], 12 * (size_t)T);
  FENSURE(h, h->host[H_META], 2 * 16 * (size_t)nc);

  for (int c = 0; c < nc; ++c) {
    const FeatCloudDesc& d = h->desc[(size_t)c];
    if (d.n > 0) memcpy(h->host[H_PTS].as<float>() + 3 * d.off, cloud[c], 12 * (size_t)d.n);
  }
  const FeatCloudDesc* d_desc = B[B_DESC].as<FeatCloudDesc>();
  const int32_t* d_blk = B[B_BLK].as<int32_t>();
  const int32_t* d_ptc = B[B_PT_CLOUD].as<int32_t>();
  const float* d_pts = B[B_PTS].as<float>();
  FCHK(h, hipMemcpyAsync(B[B_DESC].p, h->desc.data(), sizeof(FeatCloudDesc) * (size_t)nc, hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (descriptors)");
  FCHK(h, hipMemcpyAsync(B[B_BLK].p, h->blk_cloud.data(), 4 * (size_t)n_blk, hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (block map)");
  FCHK(h, hipMemcpyAsync(B[B_PT_CLOUD].p, h->pt_cloud.data(), 4 * (size_t)T, hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (point map)");
  FCHK(h, hipMemcpyAsync(B[B_PTS].p, h->host[H_PTS].p, 12 * (size_t)T, hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (points)");

  // ---- 1. counts and scans for both radii, one copy of the totals ----
  FCHK(h, hipMemsetAsync(B[B_COUNTS].p, 0, 2 * 4 * (size_t)T, s), "hipMemsetAsync (counts)");
  for (int w = 0; w < 2; ++w) {
    launch_feat_radius_count_batch(s, d_desc, d_blk, 0, n_blk, w, d_pts, B[B_COUNTS].as<int32_t>() + w * T);
    launch_feat_scan_batch(s, d_desc, nc, B[B_COUNTS].as<int32_t>() + w * T, B[B_OFFSETS].as<int64_t>() + w * T,
                           B[B_META].as<int64_t>() + (size_t)w * 2 * nc);
  }
  FCHK(h, hipGetLastError(), "front-end kernel launch (counts)");
  const int64_t* meta = h->host[H_META].as<int64_t>();
  FCHK(h, hipMemcpyAsync(h->host[H_META].p, B[B_META].p, 2 * 16 * (size_t)nc, hipMemcpyDeviceToHost, s),
       "hipMemcpyAsync (list totals)");
  FCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize (list totals)");

  // ---- 2. waves of clouds per radius, list bases, one allocation ----
  const int64_t budget = h->list_budget / feat_nbr_bytes();
  std::vector<Wave> waves[2];
  std::vector<char> wave_long[2];
  h->base.assign(2 * (size_t)nc, 0);
  int64_t list_cap = 1;
  bool any_long = false;
  for (int w = 0; w < 2; ++w) {
    int c0 = 0;
    int64_t acc = 0;
    bool lng = false;
    for (int c = 0; c < nc; ++c) {
      const int64_t tot = meta[(size_t)w * 2 * nc + 2 * c], mx = meta[(size_t)w * 2 * nc + 2 * c + 1];
      if (c > c0 && acc + tot > budget) {
        waves[w].push_back(Wave{c0, c});
        wave_long[w].push_back(lng);
        c0 = c;
        acc = 0;
        lng = false;
      }
      h->base[(size_t)w * nc + c] = acc;
      acc += tot;
      lng |= mx > feat_sort_capacity();
      list_cap = std::max(list_cap, acc);
    }
    waves[w].push_back(Wave{c0, nc});
    wave_long[w].push_back(lng);
    for (char l : wave_long[w]) any_long |= l != 0;
  }
  FENSURE(h, B[B_LIST], (size_t)list_cap * (size_t)feat_nbr_bytes());
  if (any_long) FENSURE(h, B[B_LIST2], (size_t)list_cap * (size_t)feat_nbr_bytes());
  FCHK(h, hipMemcpyAsync(B[B_BASE].p, h->base.data(), 2 * 8 * (size_t)nc, hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (list bases)");
  for (int w = 0; w < 2; ++w)
    launch_feat_rebase(s, d_ptc, B[B_BASE].as<int64_t>() + (size_t)w * nc, T, B[B_OFFSETS].as<int64_t>() + w * T);

  // ---- 3. per radius and wave: lists, then what consumes them ----
  for (int w = 0; w < 2; ++w) {
    FCHK(h, hipMemsetAsync(B[B_CURSOR].p, 0, 4 * (size_t)T, s), "hipMemsetAsync (cursor)");
    const int32_t* counts = B[B_COUNTS].as<int32_t>() + w * T;
    const int64_t* offsets = B[B_OFFSETS].as<int64_t>() + w * T;
    for (size_t k = 0; k < waves[w].size(); ++k) {
      const FeatCloudDesc& first = h->desc[(size_t)waves[w][k].c0];
      const FeatCloudDesc& last = h->desc[(size_t)waves[w][k].c1 - 1];
      const int blk0 = first.blk_off, blk1 = (int)(last.blk_off + cloud_blocks(last));
      const int64_t pt0 = first.off, pt1 = last.off + last.n;
      launch_feat_lists_batch(s, d_desc, d_blk, blk0, blk1 - blk0, w, pt0, pt1, d_pts, counts,
                              B[B_CURSOR].as<int32_t>(), offsets, B[B_LIST].p,
                              wave_long[w][k] ? B[B_LIST2].p : nullptr);
      if (w == 0)
        launch_feat_normals_batch(s, d_desc, d_ptc, pt0, pt1, d_pts, offsets, counts, B[B_LIST].p,
                                  B[B_NORMALS].as<float>());
      else
        launch_feat_fpfh_batch(s, d_desc, d_ptc, pt0, pt1, d_pts, B[B_NORMALS].as<float>(), offsets, counts,
                               B[B_LIST].p, B[B_SPFH].as<float>(), B[B_FEAT].as<float>());
    }
  }
  FCHK(h, hipGetLastError(), "front-end kernel launch (features)");
  return TEASER_HIP_OK;
}

// Enqueues the copy of a packed per-point device array (`width` floats per point) into the per-cloud host arrays.
int32_t copy_out(teaser_hip_features* h, const float* d_packed, int width, float* const* out, int first, int stride) {
  if (!out) return TEASER_HIP_OK;
  for (size_t c = (size_t)first, b = 0; c < h->desc.size(); c += (size_t)stride, ++b) {
    const FeatCloudDesc& d = h->desc[c];
    if (d.n > 0 && out[b])
      FCHK(h, hipMemcpyAsync(out[b], d_packed + (size_t)width * d.off, 4 * (size_t)width * d.n, hipMemcpyDeviceToHost,
                             h->stream),
           "hipMemcpyAsync (outputs)");
  }
  return TEASER_HIP_OK;
}

int32_t validate_match_outputs(teaser_hip_features* h, int32_t batch, int32_t* const* pairs, const int64_t* pair_cap,
                               int64_t* n_pairs) {
  if (!pair_cap) return fail(h, TEASER_HIP_ERR_BAD_ARG, "pair_cap must not be NULL");
  if (!n_pairs) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_pairs must not be NULL");
  for (int b = 0; b < batch; ++b) {
    if (pair_cap[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "pair_cap must be >= 0" + at(b));
    if (pair_cap[b] > 0 && (!pairs || !pairs[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "pairs is NULL" + at(b));
  }
  return TEASER_HIP_OK;
}

// The k-NN searches `in` over rows of d_feat, enqueued: row q of search number x in B_KNN_I (and B_KNN_D when
// want_dist) at h->search[x].nn_off = k slots, the k nearest in (d, index) order, then -1 / +inf.  No synchronisation.
// The partial lists (8 bytes per query, data chunk and list slot of the kernel serving k) of one wave of searches fit
// the partial-result budget; a wave always holds at least one search.  *total = result slots of all searches.
int32_t run_knn(teaser_hip_features* h, const std::vector<KnnSearch>& in, const std::vector<int>& problem_of,
                const float* d_feat, int dim, int k, bool want_dist, int64_t* total) {
  hipStream_t s = h->stream;
  DevBuf* B = h->buf;
  h->search.clear();
  *total = 0;
  if (in.empty()) return TEASER_HIP_OK;
  const int slots = feat_knn_slots(k);
  const int64_t part_budget = h->part_budget / 8;
  std::vector<Wave> waves;
  std::vector<int> wave_blk0;
  int64_t blocks = 0, part_acc = 0, part_cap = 1;
  int q0 = 0;
  for (int q = 0; q < (int)in.size(); ++q) {
    const KnnSearch& x = in[(size_t)q];
    const int64_t part = (int64_t)feat_nn_chunks(x.nd) * slots * x.nq;
    if (q > q0 && part_acc + part > part_budget) {
      waves.push_back(Wave{q0, q});
      q0 = q;
      part_acc = 0;
    }
    if (q == q0) wave_blk0.push_back((int)blocks);
    const FeatSearchDesc d{x.data_row, x.query_row, part_acc, *total, x.nd, x.nq, (int32_t)blocks, (x.nq + 63) / 64};
    blocks += (int64_t)d.qblocks * feat_nn_chunks(x.nd);
    if (blocks >= INT32_MAX)
      return fail(h, TEASER_HIP_ERR_UNSUPPORTED, "too many features in one call" + at(problem_of[(size_t)q]));
    part_acc += part;
    part_cap = std::max(part_cap, part_acc);
    *total += (int64_t)x.nq * k;
    h->search.push_back(d);
  }
  waves.push_back(Wave{q0, (int)in.size()});
  h->blk_search.resize((size_t)blocks);
  for (size_t q = 0; q < h->search.size(); ++q) {
    const int32_t end = q + 1 < h->search.size() ? h->search[q + 1].blk_off : (int32_t)blocks;
    std::fill(h->blk_search.begin() + h->search[q].blk_off, h->blk_search.begin() + end, (int32_t)q);
  }
  FENSURE(h, B[B_SEARCH], sizeof(FeatSearchDesc) * h->search.size());
  FENSURE(h, B[B_SBLK], 4 * (size_t)blocks);
  FENSURE(h, B[B_PART_D], 4 * (size_t)part_cap);
  FENSURE(h, B[B_PART_I], 4 * (size_t)part_cap);
  FENSURE(h, B[B_KNN_I], 4 * (size_t)*total);
  if (want_dist) FENSURE(h, B[B_KNN_D], 4 * (size_t)*total);
  FCHK(h, hipMemcpyAsync(B[B_SEARCH].p, h->search.data(), sizeof(FeatSearchDesc) * h->search.size(),
                         hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (search descriptors)");
  FCHK(h, hipMemcpyAsync(B[B_SBLK].p, h->blk_search.data(), 4 * (size_t)blocks, hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (search block map)");
  for (size_t w = 0; w < waves.size(); ++w) {
    const int s0 = waves[w].c0, s1 = waves[w].c1;
    const int blk0 = wave_blk0[w], blk1 = s1 < (int)h->search.size() ? h->search[(size_t)s1].blk_off : (int)blocks;
    int max_nq = 0;
    for (int q = s0; q < s1; ++q) max_nq = std::max(max_nq, h->search[(size_t)q].nq);
    launch_feat_knn_batch(s, B[B_SEARCH].as<FeatSearchDesc>(), B[B_SBLK].as<int32_t>(), blk0, blk1 - blk0, s0, s1,
                          max_nq, d_feat, dim, k, B[B_PART_D].as<float>(), B[B_PART_I].as<int32_t>(),
                          B[B_KNN_I].as<int32_t>(), want_dist ? B[B_KNN_D].as<float>() : nullptr);
  }
  FCHK(h, hipGetLastError(), "front-end kernel launch (k-NN)");
  return TEASER_HIP_OK;
}

// The end of the matching calls: too_small = the first problem whose pairs did not fit its pair_cap, -1 if all did.
int32_t check_pair_caps(teaser_hip_features* h, int too_small, const int64_t* n_pairs) {
  if (too_small < 0) return TEASER_HIP_OK;
  return fail(h, TEASER_HIP_ERR_BAD_ARG,
              "pair_cap is too small: " + std::to_string(n_pairs[too_small]) + " pairs needed" + at(too_small));
}

// Matches `batch` pairs whose features are rows of d_feat (src_row[b], dst_row[b] = first row of each side): two
// 1-nearest searches per pair through run_knn, the indices copied back, ONE synchronisation, then the pair lists.
int32_t run_match(teaser_hip_features* h, int32_t batch, const float* d_feat, const int64_t* src_row,
                  const int64_t* dst_row, const int32_t* n_src, const int32_t* n_dst, int dim, bool use_crosscheck,
                  int32_t* const* pairs, const int64_t* pair_cap, int64_t* n_pairs) {
  hipStream_t s = h->stream;
  for (int b = 0; b < batch; ++b) n_pairs[b] = 0;
  // two searches per pair with both sides non-empty (matcher.cc:123-133: i = the larger cloud, j = the smaller one):
  // search 2k: for every j its nearest i (:162);  search 2k + 1: for every i its nearest j (:165)
  std::vector<KnnSearch> in;
  std::vector<int> problem_of;  // pair index of searches 2k, 2k + 1
  for (int b = 0; b < batch; ++b) {
    if (n_src[b] == 0 || n_dst[b] == 0) continue;
    const bool swapped = n_dst[b] > n_src[b];
    const int ni = swapped ? n_dst[b] : n_src[b], nj = swapped ? n_src[b] : n_dst[b];
    const int64_t ri = swapped ? dst_row[b] : src_row[b], rj = swapped ? src_row[b] : dst_row[b];
    in.push_back(KnnSearch{ri, rj, ni, nj});
    in.push_back(KnnSearch{rj, ri, nj, ni});
    problem_of.insert(problem_of.end(), 2, b);
  }
  int64_t total = 0;
  const int32_t rc = run_knn(h, in, problem_of, d_feat, dim, 1, false, &total);
  if (rc != TEASER_HIP_OK) return rc;
  if (total > 0) {
    FENSURE(h, h->host[H_KNN_I], 4 * (size_t)total);
    FCHK(h, hipMemcpyAsync(h->host[H_KNN_I].p, h->buf[B_KNN_I].p, 4 * (size_t)total, hipMemcpyDeviceToHost, s),
         "hipMemcpyAsync (nearest neighbours)");
  }
  FCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize (results)");

  int too_small = -1;
  for (size_t x = 0; x < in.size(); x += 2) {
    const int b = problem_of[x];
    const FeatSearchDesc& a = h->search[x];
    const int ni = a.nd, nj = a.nq;
    const int32_t* j_to_i = h->host[H_KNN_I].as<int32_t>() + a.nn_off;  // (k = 1: a search's results are its nq rows)
    const int32_t* i_nn = j_to_i + nj;
    // A query whose distances are all NaN / +inf (non-finite features) has no nearest neighbour: the kernel reports
    // -1.  FLANN would return garbage there; an error is the honest answer.
    bool ok = true;
    for (int j = 0; j < nj; ++j) ok &= j_to_i[j] >= 0 && j_to_i[j] < ni;
    for (int i = 0; i < ni; ++i) ok &= i_nn[i] >= 0 && i_nn[i] < nj;
    if (!ok)
      return fail(h, TEASER_HIP_ERR_BAD_ARG, "non-finite feature values (no nearest neighbour for a point)" + at(b));
    const auto corres = feat_match_pairs(j_to_i, nj, i_nn, ni, n_dst[b] > n_src[b], use_crosscheck);
    n_pairs[b] = (int64_t)corres.size();
    if ((int64_t)corres.size() > pair_cap[b]) {
      if (too_small < 0) too_small = b;
      continue;
    }
    for (size_t q = 0; q < corres.size(); ++q) {
      pairs[b][2 * q] = corres[q].first;
      pairs[b][2 * q + 1] = corres[q].second;
    }
  }
  return check_pair_caps(h, too_small, n_pairs);
}

// Whether every row of an nq x k list holds its k_eff = min(k, nd) entries (sorted: the last of them decides).
bool knn_rows_full(const int32_t* idx, int nq, int nd, int k) {
  const int k_eff = std::min(k, nd);
  bool ok = true;
  for (int q = 0; q < nq; ++q) ok &= idx[(size_t)q * k + k_eff - 1] >= 0;
  return ok;
}

// k-NN matching of `batch` pairs whose features are rows of d_feat: F[i] for every source row, with mutual also B[j]
// for every target row and the device-side filter; lists and keep mask come back in one copy phase, ONE
// synchronisation, then the pairs are written row by row, a row's kept targets in ascending order.
int32_t run_match_knn(teaser_hip_features* h, int32_t batch, const float* d_feat, const int64_t* src_row,
                      const int64_t* dst_row, const int32_t* n_src, const int32_t* n_dst, int dim, int k, bool mutual,
                      int32_t* const* pairs, const int64_t* pair_cap, int64_t* n_pairs) {
  hipStream_t s = h->stream;
  DevBuf* B = h->buf;
  for (int b = 0; b < batch; ++b) n_pairs[b] = 0;
  std::vector<KnnSearch> in;
  std::vector<int> problem_of, pair_of;
  int64_t max_entries = 0;
  for (int b = 0; b < batch; ++b) {
    if (n_src[b] == 0 || n_dst[b] == 0) continue;
    in.push_back(KnnSearch{dst_row[b], src_row[b], n_dst[b], n_src[b]});  // F: source rows ask the target
    problem_of.push_back(b);
    if (mutual) {
      in.push_back(KnnSearch{src_row[b], dst_row[b], n_src[b], n_dst[b]});  // B: target rows ask the source
      problem_of.push_back(b);
    }
    pair_of.push_back(b);
    max_entries = std::max(max_entries, (int64_t)n_src[b] * k);
  }
  int64_t total = 0;
  const int32_t rc = run_knn(h, in, problem_of, d_feat, dim, k, false, &total);
  if (rc != TEASER_HIP_OK) return rc;
  const int per_pair = mutual ? 2 : 1;
  if (total > 0) {
    FENSURE(h, h->host[H_KNN_I], 4 * (size_t)total);
    if (mutual) {
      FENSURE(h, B[B_KNN_KEEP], (size_t)total);
      FENSURE(h, h->host[H_KNN_KEEP], (size_t)total);
      launch_feat_knn_mutual_batch(s, B[B_SEARCH].as<FeatSearchDesc>(), (int)pair_of.size(), max_entries, k,
                                   B[B_KNN_I].as<int32_t>(), B[B_KNN_KEEP].as<uint8_t>());
      FCHK(h, hipGetLastError(), "front-end kernel launch (mutual filter)");
      FCHK(h, hipMemcpyAsync(h->host[H_KNN_KEEP].p, B[B_KNN_KEEP].p, (size_t)total, hipMemcpyDeviceToHost, s),
           "hipMemcpyAsync (keep mask)");
    }
    FCHK(h, hipMemcpyAsync(h->host[H_KNN_I].p, B[B_KNN_I].p, 4 * (size_t)total, hipMemcpyDeviceToHost, s),
         "hipMemcpyAsync (nearest neighbours)");
  }
  FCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize (results)");

  int too_small = -1;
  std::vector<int32_t> row;
  for (size_t p = 0; p < pair_of.size(); ++p) {
    const int b = pair_of[p];
    const FeatSearchDesc& f = h->search[per_pair * p];
    const int32_t* F = h->host[H_KNN_I].as<int32_t>() + f.nn_off;
    const uint8_t* keep = mutual ? h->host[H_KNN_KEEP].as<uint8_t>() + f.nn_off : nullptr;
    bool ok = knn_rows_full(F, f.nq, f.nd, k);
    if (mutual) {
      const FeatSearchDesc& r = h->search[per_pair * p + 1];
      ok = ok && knn_rows_full(h->host[H_KNN_I].as<int32_t>() + r.nn_off, r.nq, r.nd, k);
    }
    if (!ok)
      return fail(h, TEASER_HIP_ERR_BAD_ARG,
                  "non-finite feature values (fewer than min(k, n) neighbours for a point)" + at(b));
    const int k_eff = std::min(k, f.nd);
    int64_t count = 0;
    for (int i = 0; i < f.nq; ++i)
      for (int q = 0; q < k_eff; ++q) count += !keep || keep[(size_t)i * k + q];
    n_pairs[b] = count;
    if (count > pair_cap[b]) {
      if (too_small < 0) too_small = b;
      continue;
    }
    int32_t* out = pairs[b];
    for (int i = 0; i < f.nq; ++i) {
      row.clear();
      for (int q = 0; q < k_eff; ++q)
        if (!keep || keep[(size_t)i * k + q]) row.push_back(F[(size_t)i * k + q]);
      std::sort(row.begin(), row.end());
      for (int32_t j : row) {
        *out++ = i;
        *out++ = j;
      }
    }
  }
  return check_pair_caps(h, too_small, n_pairs);
}

// The two feature sets of every problem (a[b]: n_a[b] x dim, b[b]: n_b[b] x dim), checked and copied one after the
// other into B_MFEAT; a problem with an empty side is not read.  a_row / b_row = first row of each side.
int32_t upload_feature_pairs(teaser_hip_features* h, int32_t batch, const float* const* a, const char* a_name,
                             const int32_t* n_a, const float* const* b, const char* b_name, const int32_t* n_b,
                             const char* n_names, int dim, std::vector<int64_t>* a_row, std::vector<int64_t>* b_row,
                             float** d_feat) {
  a_row->assign((size_t)batch, 0);
  b_row->assign((size_t)batch, 0);
  int64_t rows = 0;
  for (int p = 0; p < batch; ++p) {
    if (n_a[p] < 0 || n_b[p] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string(n_names) + " must be >= 0" + at(p));
    const bool both = n_a[p] > 0 && n_b[p] > 0;
    if (both && (!a || !a[p])) return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string(a_name) + " is NULL" + at(p));
    if (both && (!b || !b[p])) return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string(b_name) + " is NULL" + at(p));
    (*a_row)[(size_t)p] = rows;
    rows += both ? n_a[p] : 0;
    (*b_row)[(size_t)p] = rows;
    rows += both ? n_b[p] : 0;
    if (rows >= INT32_MAX) return fail(h, TEASER_HIP_ERR_UNSUPPORTED, "too many features in one call" + at(p));
  }
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  FENSURE(h, h->buf[B_MFEAT], 4 * (size_t)std::max<int64_t>(rows, 1) * (size_t)dim);
  *d_feat = h->buf[B_MFEAT].as<float>();
  for (int p = 0; p < batch; ++p) {
    if (n_a[p] == 0 || n_b[p] == 0) continue;
    FCHK(h, hipMemcpyAsync(*d_feat + (size_t)(*a_row)[(size_t)p] * dim, a[p], 4 * (size_t)n_a[p] * dim,
                           hipMemcpyHostToDevice, h->stream),
         "hipMemcpyAsync (features)");
    FCHK(h, hipMemcpyAsync(*d_feat + (size_t)(*b_row)[(size_t)p] * dim, b[p], 4 * (size_t)n_b[p] * dim,
                           hipMemcpyHostToDevice, h->stream),
         "hipMemcpyAsync (features)");
  }
  return TEASER_HIP_OK;
}

// FPFH of both clouds of every pair (cloud 2 b = source of pair b, cloud 2 b + 1 = its target), the copies of the
// features / normals the caller asked for enqueued; src_row / dst_row = first row of each side in B_FEAT.
int32_t run_pair_fpfh(teaser_hip_features* h, int32_t batch, const float* const* src_xyz, const int32_t* n_src,
                      const float* const* dst_xyz, const int32_t* n_dst, const double* normal_radius,
                      const double* fpfh_radius, float* const* src_feat_out, float* const* dst_feat_out,
                      float* const* src_normals_out, float* const* dst_normals_out, std::vector<int64_t>* src_row,
                      std::vector<int64_t>* dst_row) {
  std::vector<const float*> cloud(2 * (size_t)batch);
  for (int b = 0; b < batch; ++b) {
    cloud[2 * (size_t)b] = src_xyz ? src_xyz[b] : nullptr;
    cloud[2 * (size_t)b + 1] = dst_xyz ? dst_xyz[b] : nullptr;
  }
  const char* names[2] = {"src_xyz", "dst_xyz"};
  const int32_t* ns[2] = {n_src, n_dst};
  int32_t rc = validate_clouds(h, 2 * batch, 2, cloud.data(), names, ns, normal_radius, fpfh_radius);
  if (rc != TEASER_HIP_OK) return rc;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  if ((rc = run_fpfh(h, cloud.data())) != TEASER_HIP_OK) return rc;
  if (h->desc.back().off + h->desc.back().n > 0) {  // (features leave the device only where the caller asked)
    if ((rc = copy_out(h, h->buf[B_FEAT].as<float>(), 33, src_feat_out, 0, 2)) != TEASER_HIP_OK) return rc;
    if ((rc = copy_out(h, h->buf[B_FEAT].as<float>(), 33, dst_feat_out, 1, 2)) != TEASER_HIP_OK) return rc;
    if ((rc = copy_out(h, h->buf[B_NORMALS].as<float>(), 3, src_normals_out, 0, 2)) != TEASER_HIP_OK) return rc;
    if ((rc = copy_out(h, h->buf[B_NORMALS].as<float>(), 3, dst_normals_out, 1, 2)) != TEASER_HIP_OK) return rc;
  }
  src_row->resize((size_t)batch);
  dst_row->resize((size_t)batch);
  for (int b = 0; b < batch; ++b) {
    (*src_row)[(size_t)b] = h->desc[2 * (size_t)b].off;
    (*dst_row)[(size_t)b] = h->desc[2 * (size_t)b + 1].off;
  }
  return TEASER_HIP_OK;
}

int32_t check_knn_args(teaser_hip_features* h, int32_t batch, int32_t dim, int32_t k) {
  if (batch < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0");
  if (dim <= 0 || dim > feat_nn_max_dim())
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "dim must be in [1, " + std::to_string(feat_nn_max_dim()) + "]");
  if (k < 1 || k > TEASER_HIP_FEATURES_KNN_MAX)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "k must be in [1, " + std::to_string(TEASER_HIP_FEATURES_KNN_MAX) + "]");
  return TEASER_HIP_OK;
}

}  // namespace

int32_t thip::features_fpfh_batch(teaser_hip_features* h, int32_t batch, const float* const* cloud, const int32_t* n,
                                  const double* normal_radius, const double* fpfh_radius, float* const* fpfh_out,
                                  float* const* normals_out) {
  h->err.clear();
  if (!n) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n must not be NULL");
  const char* names[1] = {"cloud"};
  const int32_t* ns[1] = {n};
  int32_t rc = validate_clouds(h, batch, 1, cloud, names, ns, normal_radius, fpfh_radius);
  if (rc != TEASER_HIP_OK) return rc;
  for (int b = 0; b < batch; ++b)
    if (n[b] > 0 && (!fpfh_out || !fpfh_out[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "fpfh_out is NULL" + at(b));
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  if ((rc = run_fpfh(h, cloud)) != TEASER_HIP_OK) return rc;
  if (h->desc.back().off + h->desc.back().n == 0) return TEASER_HIP_OK;
  if ((rc = copy_out(h, h->buf[B_FEAT].as<float>(), 33, fpfh_out, 0, 1)) != TEASER_HIP_OK) return rc;
  if ((rc = copy_out(h, h->buf[B_NORMALS].as<float>(), 3, normals_out, 0, 1)) != TEASER_HIP_OK) return rc;
  FCHK(h, hipStreamSynchronize(h->stream), "hipStreamSynchronize (results)");
  return TEASER_HIP_OK;
}

extern "C" {

int32_t teaser_hip_features_create(int32_t device, teaser_hip_features** out) { return open_handle(device, out); }

int32_t teaser_hip_features_destroy(teaser_hip_features* h) { return close_handle(h); }

const char* teaser_hip_features_last_error(const teaser_hip_features* h) { return h ? h->err.c_str() : ""; }

int32_t teaser_hip_features_fill_scratch(teaser_hip_features* h, int32_t byte, int64_t* bytes_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  ScratchSpan spans[B_COUNT_OF_BUFS + H_COUNT_OF_BUFS];
  for (int k = 0; k < B_COUNT_OF_BUFS; ++k) spans[k] = span_of(h->buf[k]);
  for (int k = 0; k < H_COUNT_OF_BUFS; ++k) spans[B_COUNT_OF_BUFS + k] = span_of(h->host[k]);
  return fill_scratch(h, byte, spans, B_COUNT_OF_BUFS + H_COUNT_OF_BUFS, bytes_out);
}

int32_t teaser_hip_features_set_budgets(teaser_hip_features* h, int64_t list_bytes, int64_t part_bytes) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->list_budget = list_bytes > 0 ? list_bytes : kFeatListBudgetBytes;
  h->part_budget = part_bytes > 0 ? part_bytes : kFeatPartBudgetBytes;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_features_fpfh_batch(teaser_hip_features* h, int32_t batch, const float* const* cloud,
                                       const int32_t* n, const double* normal_radius, const double* fpfh_radius,
                                       float* const* fpfh_out, float* const* normals_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (batch < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0");
  if (batch == 0) return TEASER_HIP_OK;
  const int32_t rc = check_radii(h, batch, normal_radius, fpfh_radius);
  if (rc != TEASER_HIP_OK) return rc;
  return features_fpfh_batch(h, batch, cloud, n, normal_radius, fpfh_radius, fpfh_out, normals_out);
}

int32_t teaser_hip_features_match_batch(teaser_hip_features* h, int32_t batch, const float* const* src_feat,
                                        const int32_t* n_src, const float* const* dst_feat, const int32_t* n_dst,
                                        int32_t dim, int32_t use_crosscheck, int32_t* const* pairs,
                                        const int64_t* pair_cap, int64_t* n_pairs) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (batch < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0");
  if (dim <= 0 || dim > feat_nn_max_dim())
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "dim must be in [1, " + std::to_string(feat_nn_max_dim()) + "]");
  if (batch == 0) return TEASER_HIP_OK;
  if (!n_src || !n_dst) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src / n_dst must not be NULL");
  int32_t rc = validate_match_outputs(h, batch, pairs, pair_cap, n_pairs);
  if (rc != TEASER_HIP_OK) return rc;
  std::vector<int64_t> src_row, dst_row;
  float* d_feat = nullptr;
  rc = upload_feature_pairs(h, batch, src_feat, "src_feat", n_src, dst_feat, "dst_feat", n_dst, "n_src / n_dst", dim,
                            &src_row, &dst_row, &d_feat);
  if (rc != TEASER_HIP_OK) return rc;
  return run_match(h, batch, d_feat, src_row.data(), dst_row.data(), n_src, n_dst, dim, use_crosscheck != 0, pairs,
                   pair_cap, n_pairs);
}

int32_t teaser_hip_features_correspondences_batch(teaser_hip_features* h, int32_t batch, const float* const* src_xyz,
                                                  const int32_t* n_src, const float* const* dst_xyz,
                                                  const int32_t* n_dst, const double* normal_radius,
                                                  const double* fpfh_radius, int32_t use_crosscheck,
                                                  int32_t* const* pairs, const int64_t* pair_cap, int64_t* n_pairs,
                                                  float* const* src_feat_out, float* const* dst_feat_out,
                                                  float* const* src_normals_out, float* const* dst_normals_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (batch < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0");
  if (batch == 0) return TEASER_HIP_OK;
  if (!n_src || !n_dst) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src / n_dst must not be NULL");
  int32_t rc = check_radii(h, batch, normal_radius, fpfh_radius);
  if (rc != TEASER_HIP_OK) return rc;
  rc = validate_match_outputs(h, batch, pairs, pair_cap, n_pairs);
  if (rc != TEASER_HIP_OK) return rc;
  std::vector<int64_t> src_row, dst_row;
  rc = run_pair_fpfh(h, batch, src_xyz, n_src, dst_xyz, n_dst, normal_radius, fpfh_radius, src_feat_out, dst_feat_out,
                     src_normals_out, dst_normals_out, &src_row, &dst_row);
  if (rc != TEASER_HIP_OK) return rc;
  return run_match(h, batch, h->buf[B_FEAT].as<float>(), src_row.data(), dst_row.data(), n_src, n_dst, 33,
                   use_crosscheck != 0, pairs, pair_cap, n_pairs);
}

int32_t teaser_hip_features_knn_batch(teaser_hip_features* h, int32_t batch, const float* const* data_feat,
                                      const int32_t* n_data, const float* const* query_feat, const int32_t* n_query,
                                      int32_t dim, int32_t k, int32_t* const* idx, float* const* dist) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  int32_t rc = check_knn_args(h, batch, dim, k);
  if (rc != TEASER_HIP_OK) return rc;
  if (batch == 0) return TEASER_HIP_OK;
  if (!n_data || !n_query) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_data / n_query must not be NULL");
  for (int b = 0; b < batch; ++b)
    if (n_query[b] > 0 && (!idx || !idx[b])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "idx is NULL" + at(b));
  std::vector<int64_t> data_row, query_row;
  float* d_feat = nullptr;
  rc = upload_feature_pairs(h, batch, data_feat, "data_feat", n_data, query_feat, "query_feat", n_query,
                            "n_data / n_query", dim, &data_row, &query_row, &d_feat);
  if (rc != TEASER_HIP_OK) return rc;
  std::vector<KnnSearch> in;
  std::vector<int> problem_of;
  for (int b = 0; b < batch; ++b) {
    if (n_data[b] == 0 || n_query[b] == 0) continue;
    in.push_back(KnnSearch{data_row[(size_t)b], query_row[(size_t)b], n_data[b], n_query[b]});
    problem_of.push_back(b);
  }
  int64_t total = 0;
  if ((rc = run_knn(h, in, problem_of, d_feat, dim, k, dist != nullptr, &total)) != TEASER_HIP_OK) return rc;
  if (total > 0) {
    FENSURE(h, h->host[H_KNN_I], 4 * (size_t)total);
    FCHK(h, hipMemcpyAsync(h->host[H_KNN_I].p, h->buf[B_KNN_I].p, 4 * (size_t)total, hipMemcpyDeviceToHost, h->stream),
         "hipMemcpyAsync (nearest neighbours)");
    if (dist) {
      FENSURE(h, h->host[H_KNN_D], 4 * (size_t)total);
      FCHK(h, hipMemcpyAsync(h->host[H_KNN_D].p, h->buf[B_KNN_D].p, 4 * (size_t)total, hipMemcpyDeviceToHost,
                             h->stream),
           "hipMemcpyAsync (distances)");
    }
  }
  FCHK(h, hipStreamSynchronize(h->stream), "hipStreamSynchronize (results)");
  int bad = -1;
  size_t x = 0;
  for (int b = 0; b < batch; ++b) {
    const size_t slots = (size_t)n_query[b] * (size_t)k;
    if (slots == 0) continue;
    float* db = dist ? dist[b] : nullptr;
    if (n_data[b] == 0) {  // nothing to find: k_eff = 0
      std::fill_n(idx[b], slots, -1);
      if (db) std::fill_n(db, slots, (float)INFINITY);
      continue;
    }
    const FeatSearchDesc& d = h->search[x++];
    memcpy(idx[b], h->host[H_KNN_I].as<int32_t>() + d.nn_off, 4 * slots);
    if (db) memcpy(db, h->host[H_KNN_D].as<float>() + d.nn_off, 4 * slots);
    if (bad < 0 && !knn_rows_full(idx[b], d.nq, d.nd, k)) bad = b;
  }
  if (bad >= 0)
    return fail(h, TEASER_HIP_ERR_BAD_ARG,
                "non-finite feature values (fewer than min(k, n) neighbours for a point)" + at(bad));
  return TEASER_HIP_OK;
}

int32_t teaser_hip_features_match_knn_batch(teaser_hip_features* h, int32_t batch, const float* const* src_feat,
                                            const int32_t* n_src, const float* const* dst_feat, const int32_t* n_dst,
                                            int32_t dim, int32_t k, int32_t mutual, int32_t* const* pairs,
                                            const int64_t* pair_cap, int64_t* n_pairs) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  int32_t rc = check_knn_args(h, batch, dim, k);
  if (rc != TEASER_HIP_OK) return rc;
  if (batch == 0) return TEASER_HIP_OK;
  if (!n_src || !n_dst) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src / n_dst must not be NULL");
  if ((rc = validate_match_outputs(h, batch, pairs, pair_cap, n_pairs)) != TEASER_HIP_OK) return rc;
  std::vector<int64_t> src_row, dst_row;
  float* d_feat = nullptr;
  rc = upload_feature_pairs(h, batch, src_feat, "src_feat", n_src, dst_feat, "dst_feat", n_dst, "n_src / n_dst", dim,
                            &src_row, &dst_row, &d_feat);
  if (rc != TEASER_HIP_OK) return rc;
  return run_match_knn(h, batch, d_feat, src_row.data(), dst_row.data(), n_src, n_dst, dim, k, mutual != 0, pairs,
                       pair_cap, n_pairs);
}

int32_t teaser_hip_features_correspondences_knn_batch(
    teaser_hip_features* h, int32_t batch, const float* const* src_xyz, const int32_t* n_src,
    const float* const* dst_xyz, const int32_t* n_dst, const double* normal_radius, const double* fpfh_radius,
    int32_t k, int32_t mutual, int32_t* const* pairs, const int64_t* pair_cap, int64_t* n_pairs,
    float* const* src_feat_out, float* const* dst_feat_out, float* const* src_normals_out,
    float* const* dst_normals_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  int32_t rc = check_knn_args(h, batch, 33, k);
  if (rc != TEASER_HIP_OK) return rc;
  if (batch == 0) return TEASER_HIP_OK;
  if (!n_src || !n_dst) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src / n_dst must not be NULL");
  if ((rc = check_radii(h, batch, normal_radius, fpfh_radius)) != TEASER_HIP_OK) return rc;
  if ((rc = validate_match_outputs(h, batch, pairs, pair_cap, n_pairs)) != TEASER_HIP_OK) return rc;
  std::vector<int64_t> src_row, dst_row;
  rc = run_pair_fpfh(h, batch, src_xyz, n_src, dst_xyz, n_dst, normal_radius, fpfh_radius, src_feat_out, dst_feat_out,
                     src_normals_out, dst_normals_out, &src_row, &dst_row);
  if (rc != TEASER_HIP_OK) return rc;
  return run_match_knn(h, batch, h->buf[B_FEAT].as<float>(), src_row.data(), dst_row.data(), n_src, n_dst, 33, k,
                       mutual != 0, pairs, pair_cap, n_pairs);
}

int32_t teaser_hip_features_tuple_test_batch(teaser_hip_features* h, int32_t batch, const float* const* src_xyz,
                                             const int32_t* n_src, const float* const* dst_xyz, const int32_t* n_dst,
                                             const float* tuple_scale, const uint64_t* seed, int32_t* const* pairs,
                                             int64_t* n_pairs) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (batch < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0");
  if (batch == 0) return TEASER_HIP_OK;
  if (!n_src || !n_dst) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src / n_dst must not be NULL");
  if (!tuple_scale) return fail(h, TEASER_HIP_ERR_BAD_ARG, "tuple_scale must not be NULL");
  if (!seed) return fail(h, TEASER_HIP_ERR_BAD_ARG, "seed must not be NULL");
  if (!n_pairs) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_pairs must not be NULL");

  // ---- everything that can be refused is refused here, before anything is launched or written ----
  // The problems the test applies to (teaser_hip_tuple_test returns the others untouched), cut into waves whose pairs
  // (8 bytes each) fit the partial-result budget; a wave always holds at least one problem.
  const int64_t pair_budget = h->part_budget / 8;
  h->tuple.clear();
  std::vector<int> problem_of;
  std::vector<Wave> waves;            // in units of active problems
  std::vector<int64_t> wave_pair0;    // first pair of each wave in the host's packed arrays
  int64_t n_pts = 0, blocks = 0, pair_acc = 0, pair_cap = 0, pair_total = 0;
  int a0 = 0;
  bool clock_seed = false;
  for (int b = 0; b < batch; ++b) {
    if (n_src[b] < 0 || n_dst[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_src / n_dst must be >= 0" + at(b));
    if (n_pairs[b] < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_pairs must be >= 0" + at(b));
    if (n_pairs[b] == 0) continue;
    if (!pairs || !pairs[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "pairs is NULL" + at(b));
    if (!src_xyz || !src_xyz[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "src_xyz is NULL" + at(b));
    if (!dst_xyz || !dst_xyz[b]) return fail(h, TEASER_HIP_ERR_BAD_ARG, "dst_xyz is NULL" + at(b));
    if (!(tuple_scale[b] > 0.0f)) continue;  // matcher.cc:223: skipped for tuple_scale == 0
    const int64_t ncorr = n_pairs[b];
    for (int64_t k = 0; k < ncorr; ++k)
      if (pairs[b][2 * k] < 0 || pairs[b][2 * k] >= n_src[b] || pairs[b][2 * k + 1] < 0 ||
          pairs[b][2 * k + 1] >= n_dst[b])
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "a pair's index lies outside its cloud" + at(b));
    const int a = (int)problem_of.size();
    if (a > a0 && pair_acc + ncorr > pair_budget) {
      waves.push_back(Wave{a0, a});
      a0 = a;
      pair_acc = 0;
    }
    if (a == a0) wave_pair0.push_back(pair_total);
    const int64_t nb = feat_tuple_blocks(ncorr);
    h->tuple.push_back(FeatTupleDesc{pair_acc, ncorr, n_pts, n_pts + n_src[b], seed[b], tuple_scale[b], (int32_t)blocks,
                                     (int32_t)nb, 0});
    blocks += nb;
    if (blocks >= INT32_MAX) return fail(h, TEASER_HIP_ERR_UNSUPPORTED, "too many pairs in one call" + at(b));
    n_pts += (int64_t)n_src[b] + n_dst[b];
    pair_acc += ncorr;
    pair_total += ncorr;
    pair_cap = std::max(pair_cap, pair_acc);
    clock_seed |= seed[b] == 0;
    problem_of.push_back(b);
  }
  const int na = (int)problem_of.size();
  if (na == 0) return TEASER_HIP_OK;
  waves.push_back(Wave{a0, na});
  if (clock_seed) {  // "from the clock": one reading for the call
    const uint64_t now = (uint64_t)time(nullptr);
    for (FeatTupleDesc& d : h->tuple)
      if (d.seed == 0) d.seed = now;
  }
  h->blk_tuple.resize((size_t)blocks);
  for (int a = 0; a < na; ++a)
    std::fill_n(h->blk_tuple.begin() + h->tuple[(size_t)a].blk_off, h->tuple[(size_t)a].n_blk, a);

  // ---- one upload: descriptors, block map, the packed points (source then target of every problem) and pairs ----
  hipStream_t s = h->stream;
  DevBuf* B = h->buf;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  FENSURE(h, B[B_TUPLE_DESC], sizeof(FeatTupleDesc) * (size_t)na);
  FENSURE(h, B[B_TUPLE_BLK], 4 * (size_t)blocks);
  FENSURE(h, B[B_PTS], 12 * (size_t)std::max<int64_t>(n_pts, 1));
  FENSURE(h, B[B_TUPLE_PAIRS], 8 * (size_t)pair_cap);
  FENSURE(h, B[B_TUPLE_KEEP], (size_t)pair_cap);
  FENSURE(h, h->host[H_PTS], 12 * (size_t)std::max<int64_t>(n_pts, 1));
  FENSURE(h, h->host[H_TUPLE_PAIRS], 8 * (size_t)pair_total);
  FENSURE(h, h->host[H_TUPLE_KEEP], (size_t)pair_total);
  {
    int32_t* hp = h->host[H_TUPLE_PAIRS].as<int32_t>();
    for (int a = 0; a < na; ++a) {
      const int b = problem_of[(size_t)a];
      const FeatTupleDesc& d = h->tuple[(size_t)a];
      float* pts = h->host[H_PTS].as<float>();
      if (n_src[b] > 0) memcpy(pts + 3 * d.src_off, src_xyz[b], 12 * (size_t)n_src[b]);
      if (n_dst[b] > 0) memcpy(pts + 3 * d.dst_off, dst_xyz[b], 12 * (size_t)n_dst[b]);
      memcpy(hp, pairs[b], 8 * (size_t)d.ncorr);
      hp += 2 * d.ncorr;
    }
  }
  FCHK(h, hipMemcpyAsync(B[B_TUPLE_DESC].p, h->tuple.data(), sizeof(FeatTupleDesc) * (size_t)na, hipMemcpyHostToDevice,
                         s),
       "hipMemcpyAsync (tuple descriptors)");
  FCHK(h, hipMemcpyAsync(B[B_TUPLE_BLK].p, h->blk_tuple.data(), 4 * (size_t)blocks, hipMemcpyHostToDevice, s),
       "hipMemcpyAsync (tuple block map)");
  if (n_pts > 0)
    FCHK(h, hipMemcpyAsync(B[B_PTS].p, h->host[H_PTS].p, 12 * (size_t)n_pts, hipMemcpyHostToDevice, s),
         "hipMemcpyAsync (points)");
  // ---- per wave (one, normally), stream-ordered: its pairs, the launch, its keep flags back ----
  for (size_t w = 0; w < waves.size(); ++w) {
    const FeatTupleDesc& first = h->tuple[(size_t)waves[w].c0];
    const FeatTupleDesc& last = h->tuple[(size_t)waves[w].c1 - 1];
    const int64_t n_wave = last.pair_off + last.ncorr;
    FCHK(h, hipMemcpyAsync(B[B_TUPLE_PAIRS].p, h->host[H_TUPLE_PAIRS].as<int32_t>() + 2 * wave_pair0[w],
                           8 * (size_t)n_wave, hipMemcpyHostToDevice, s),
         "hipMemcpyAsync (pairs)");
    FCHK(h, hipMemsetAsync(B[B_TUPLE_KEEP].p, 0, (size_t)n_wave, s), "hipMemsetAsync (keep flags)");
    launch_feat_tuple_batch(s, B[B_TUPLE_DESC].as<FeatTupleDesc>(), B[B_TUPLE_BLK].as<int32_t>(), first.blk_off,
                            last.blk_off + last.n_blk - first.blk_off, B[B_PTS].as<float>(),
                            B[B_TUPLE_PAIRS].as<int32_t>(), B[B_TUPLE_KEEP].as<uint8_t>());
    FCHK(h, hipGetLastError(), "front-end kernel launch (tuple test)");
    FCHK(h, hipMemcpyAsync(h->host[H_TUPLE_KEEP].as<uint8_t>() + wave_pair0[w], B[B_TUPLE_KEEP].p, (size_t)n_wave,
                           hipMemcpyDeviceToHost, s),
         "hipMemcpyAsync (keep flags)");
  }
  FCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize (results)");

  // ---- the survivors of every problem, sorted and unique (matcher.cc:299-300) ----
  const uint8_t* keep = h->host[H_TUPLE_KEEP].as<uint8_t>();
  std::vector<std::pair<int32_t, int32_t>> kept;
  for (int a = 0; a < na; ++a) {
    const int b = problem_of[(size_t)a];
    const int64_t ncorr = h->tuple[(size_t)a].ncorr;
    kept.clear();
    for (int64_t k = 0; k < ncorr; ++k)
      if (keep[k]) kept.emplace_back(pairs[b][2 * k], pairs[b][2 * k + 1]);
    keep += ncorr;
    std::sort(kept.begin(), kept.end());
    kept.erase(std::unique(kept.begin(), kept.end()), kept.end());
    for (size_t k = 0; k < kept.size(); ++k) {
      pairs[b][2 * k] = kept[k].first;
      pairs[b][2 * k + 1] = kept[k].second;
    }
    n_pairs[b] = (int64_t)kept.size();
  }
  return TEASER_HIP_OK;
}

}  // extern "C"
