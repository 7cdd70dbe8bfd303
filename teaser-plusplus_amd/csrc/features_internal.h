// features_internal.h -- structures shared by the correspondence front-end's host code (features.hip) and its gfx950
// kernels (kernels_features.hip), their launchers, and the matcher's host-side index bookkeeping.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace thip {

// One cloud of a batch (host-built, read-only on the device).  Its points occupy [off, off + n) of every packed
// per-point array (points, normals, counts, offsets, SPFH, features); neighbour indices are local to the cloud.
struct FeatCloudDesc {
  int64_t off;
  int32_t n;
  int32_t blk_off;  // first radius block of this cloud in the block -> cloud map
  int32_t qblocks;  // query blocks of 64 points; the cloud's radius blocks are (chunk, qblock) = (l / qblocks, l % qblocks)
  float r2[2];      // squared search radius in float: [0] normals, [1] FPFH
  int32_t pad;
};

// One nearest-neighbour search of a batch: for each of nq query rows its nearest of nd data rows.  Rows are rows of
// the packed feature array; partial results occupy part[part_off .. part_off + chunks * slots * nq), results
// nn[nn_off .. nn_off + nq * k): for each query row its k nearest (feat_knn_slots, launch_feat_knn_batch below).
struct FeatSearchDesc {
  int64_t data_row, query_row, part_off, nn_off;
  int32_t nd, nq;
  int32_t blk_off;  // first block of this search in the block -> search map
  int32_t qblocks;  // query blocks of 64 rows; blocks are (chunk, qblock) = (l / qblocks, l % qblocks)
};

// One problem of a batched tuple test (include/teaser_hip.h, "tuple_test_batch"): its ncorr pairs occupy
// [pair_off, pair_off + ncorr) of the wave's packed pair array (two int32 each) and keep flags, its clouds start at
// points src_off / dst_off of the packed point array, its trials are spread over blocks [blk_off, blk_off + n_blk) of
// the block -> problem map.
struct FeatTupleDesc {
  int64_t pair_off, ncorr, src_off, dst_off;
  uint64_t seed;  // never 0 here: the host has replaced "from the clock" by the call's clock value
  float scale;
  int32_t blk_off, n_blk;
  int32_t pad;
};

int feat_radius_chunk();  // data points per radius block (kFeatChunk)

// counts[which][g] of every point of the clouds whose blocks are [blk_base, blk_base + n_blk) (counts zeroed first)
void launch_feat_radius_count_batch(hipStream_t s, const FeatCloudDesc* d_desc, const int32_t* d_blk_cloud, int blk_base,
                                    int n_blk, int which, const float* d_pts, int32_t* d_counts);
// per cloud: exclusive scan of its counts into offsets (local to the cloud), {total, longest list} into d_meta[2 c]
void launch_feat_scan_batch(hipStream_t s, const FeatCloudDesc* d_desc, int batch, const int32_t* d_counts,
                            int64_t* d_offsets, int64_t* d_meta);
// offsets[g] += base[cloud of g]: the cloud-local offsets become 64-bit offsets into the wave's list
void launch_feat_rebase(hipStream_t s, const int32_t* d_pt_cloud, const int64_t* d_base, int64_t n_pts,
                        int64_t* d_offsets);
// fill + LDS sort (+ rank sort of the lists longer than feat_sort_capacity() when d_scratch != nullptr) of the lists of
// points [pt0, pt1) = the clouds whose blocks are [blk_base, blk_base + n_blk); d_cursor zeroed by the caller
void launch_feat_lists_batch(hipStream_t s, const FeatCloudDesc* d_desc, const int32_t* d_blk_cloud, int blk_base,
                             int n_blk, int which, int64_t pt0, int64_t pt1, const float* d_pts,
                             const int32_t* d_counts, int32_t* d_cursor, const int64_t* d_offsets, void* d_list,
                             void* d_scratch);
void launch_feat_normals_batch(hipStream_t s, const FeatCloudDesc* d_desc, const int32_t* d_pt_cloud, int64_t pt0,
                               int64_t pt1, const float* d_pts, const int64_t* d_offsets, const int32_t* d_counts,
                               const void* d_list, float* d_normals);
void launch_feat_fpfh_batch(hipStream_t s, const FeatCloudDesc* d_desc, const int32_t* d_pt_cloud, int64_t pt0,
                            int64_t pt1, const float* d_pts, const float* d_normals, const int64_t* d_offsets,
                            const int32_t* d_counts, const void* d_list, float* d_spfh, float* d_out);
// k-NN (include/teaser_hip.h, "k nearest"; k = 1 is the matcher's pair of searches).  The searches use FeatSearchDesc
// and a block -> search map, with part_off counting the chunks x feat_knn_slots(k) x nq partial entries and nn_off the
// nq x k result slots of the searches before.
int feat_knn_slots(int k);  // list slots of the kernel instantiation that serves k (1, 2, 4, 8 or 16)
// searches [s0, s1), whose blocks are [blk_base, blk_base + n_blk); max_nq = the largest nq among them.
// Row q of d_idx / d_dist (d_dist may be nullptr) = the k nearest in (d, index) order, then -1 / +inf
void launch_feat_knn_batch(hipStream_t s, const FeatSearchDesc* d_search, const int32_t* d_blk_search, int blk_base,
                           int n_blk, int s0, int s1, int max_nq, const float* d_feat, int dim, int k, float* d_part_d,
                           int32_t* d_part_i, int32_t* d_idx, float* d_dist);
// pairs p < n_pairs with searches 2 p (forward) and 2 p + 1 (backward): d_keep[nn_off of 2 p + i k + slot] = whether
// source row i is among the k nearest of its neighbour F[i][slot]; max_entries = the largest nq x k of a forward search
void launch_feat_knn_mutual_batch(hipStream_t s, const FeatSearchDesc* d_search, int n_pairs, int64_t max_entries,
                                  int k, const int32_t* d_idx, uint8_t* d_keep);

// The tuple constraint.  feat_tuple_blocks: blocks of 256 lanes a problem of ncorr pairs gets (one trial per lane, the
// remaining trials by a grid stride inside the problem).  The launch: the problems whose blocks are [blk_base,
// blk_base + n_blk); d_keep[pair] (zeroed by the caller) becomes 1 for every pair of a passing trial.
int64_t feat_tuple_blocks(int64_t ncorr);
void launch_feat_tuple_batch(hipStream_t s, const FeatTupleDesc* d_desc, const int32_t* d_blk_problem, int blk_base,
                             int n_blk, const float* d_pts, const int32_t* d_pairs, uint8_t* d_keep);

// Index bookkeeping of Matcher::advancedMatching (reference matcher.cc:155-233, 281-296) after the two searches:
// i = the larger cloud, j = the smaller one, j_to_i[j] = nearest i of j, i_nn[i] = nearest j of i (both valid
// indices).  Returns the sorted unique (src, dst) pairs.
inline std::vector<std::pair<int32_t, int32_t>> feat_match_pairs(const int32_t* j_to_i, int nj, const int32_t* i_nn,
                                                                 int ni, bool swapped, bool use_crosscheck) {
  std::vector<int32_t> i_to_j((size_t)ni, -1);
  for (int j = 0; j < nj; ++j) {
    const int i = j_to_i[(size_t)j];
    if (i_to_j[(size_t)i] == -1) i_to_j[(size_t)i] = i_nn[(size_t)i];
  }
  std::vector<std::pair<int32_t, int32_t>> corres;
  if (use_crosscheck) {
    for (int i = 0; i < ni; ++i) {
      const int j = i_to_j[(size_t)i];
      if (j >= 0 && j_to_i[(size_t)j] == i) corres.emplace_back(i, j);
    }
  } else {
    for (int i = 0; i < ni; ++i)
      if (i_to_j[(size_t)i] != -1) corres.emplace_back(i, i_to_j[(size_t)i]);
    for (int j = 0; j < nj; ++j) corres.emplace_back(j_to_i[(size_t)j], j);
  }
  if (swapped)
    for (auto& c : corres) std::swap(c.first, c.second);
  std::sort(corres.begin(), corres.end());
  corres.erase(std::unique(corres.begin(), corres.end()), corres.end());
  return corres;
}

}  // namespace thip
