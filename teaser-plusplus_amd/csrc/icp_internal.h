// icp_internal.h -- structures shared by the ICP host code (icp.hip) and its gfx950 kernels (kernels_icp.hip).
// Kept apart from internal.h: the ICP handle shares nothing with teaser_hip_solver.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace thip {

constexpr int kIcpBlock = 256;   // source points per correspondence block (the chunking depends on n_s alone)
constexpr int kIcpSums = 17;     // {count, sum d2, sum p' (3), sum q' (3), sum p' q'^T (9)} of one block
constexpr int kIcpPlaneSums = 29;  // point-to-plane: {count, sum d2, upper triangle of A by rows (21), g (6)}
constexpr int kIcpInfoSums = 21;   // information matrix: the upper triangle of the 6 x 6 by rows
constexpr int kIcpScanThreads = 1024;
constexpr int kIcpCovBlock = 64;   // points per covariance block: one wave, one point per lane
constexpr int kIcpCovMaxNN = 100;  // K of the contract: the largest max_nn of covariance estimation
constexpr int kIcpCovSmallNN = 32; // capacity of the small instantiation's per-lane neighbour list
constexpr int kIcpKnnMax = 100;    // the largest k of self k-NN and nb_neighbors of statistical outlier removal
constexpr int kIcpKnnSmall = 32;   // capacity of the small instantiation's per-lane list
constexpr int kIcpKnnRingCap = 4;  // default number of rings searched on the grid before the whole-cloud route
constexpr int kIcpKnnRingCapMax = 16;
constexpr int kIcpKnnScanBlocks = 2048;  // waves of the whole-cloud route (each loops over the worklist)
constexpr int kIcpSearchR0Max = 16;      // two-cloud k-NN: a query more cells than this outside the grid skips the rings
constexpr int kFpsResidentCap = 10240;   // farthest-point down-sampling: the resident route's compiled capacity
constexpr int64_t kFpfhListBytes = (int64_t)512 << 20;  // Open3D-form FPFH: default bound of the neighbour-list scratch
constexpr int64_t kFpfhListBytesMax = (int64_t)1 << 40;

// IcpDesc::method / IcpDesc::kernel: the values of teaser_icp_estimation_c (include/teaser_hip.h)
enum { kIcpMethodPoint = 0, kIcpMethodPlane = 1, kIcpMethodGicp = 2, kIcpMethodColor = 3 };
enum { kIcpKernelL2 = 0, kIcpKernelHuber = 1, kIcpKernelCauchy = 2, kIcpKernelGM = 3, kIcpKernelTukey = 4 };

// One problem of a batch (host-built, read-only on the device).  Cell coordinates of a point x are
// floor((x - origin) * inv_h) per axis, clamped to [-2, 2^40] (monotone, so neighbouring cells stay neighbours).
struct IcpDesc {
  int32_t n_s, n_t;
  int64_t s_off;      // first source point in the packed X / match arrays
  int64_t t_off;      // first target point in the packed target arrays
  int64_t b_off;      // first entry of this problem's bucket-start table (tb + 1 entries)
  int64_t tb_mask;    // bucket table size - 1 (power of two >= 2 n_t); unused when n_t = 0
  int32_t blk_off;    // first correspondence block of this problem
  int32_t nblk;       // ceil(n_s / kIcpBlock)
  int64_t cmax[3];    // largest target cell coordinate per axis
  double origin[3];   // target bounding-box minimum
  double inv_h;       // 1 / cell edge (cell edge = r (1 + 1e-6) + 1e-12 max |bbox coordinate|)
  double centre[3];   // target bounding-box centre: the fixed point the sums are centred on
  double r2;          // r * r
  double rel_fitness, rel_rmse;
  int32_t max_iteration;
  int32_t tblk_off;   // first target block of this problem (index build)
  int32_t method;     // kIcpMethodPoint / kIcpMethodPlane / kIcpMethodGicp
  int32_t kernel;     // robust kernel of a point-to-plane problem (kIcpKernelL2 ...)
  double kernel_k;    // its parameter; unused for L2
};

// Mutable per-problem state.
struct IcpState {
  double T[16];       // accumulated transform, row-major 4x4
  double U[12];       // rows 0..2 of the transform the next correspondence launch applies to X
  double fitness, rmse;
  int32_t iterations; // loop bodies executed
  int32_t count;      // |C| of the current result
  int32_t phase;      // 0: the first correspondence pass has not been finalized yet
  int32_t done;       // 1: converged or out of iterations -- every later launch returns at once
};

// One cloud of a covariance-estimation call, beside its IcpDesc (the cloud is the "target" of that descriptor: n_t,
// t_off, the grid and r2 = radius^2; blk_off / nblk count its blocks of kIcpCovBlock points).
struct IcpCovDesc {
  int32_t max_nn;     // 3 .. kIcpCovMaxNN
  int32_t pad;
  double eps;         // the eigenvalue given to the normal direction
};

// One cloud of a self k-NN / outlier-removal call, beside its IcpDesc (the cloud is the descriptor's "target", as in
// covariance estimation; blk_off / nblk count its blocks of kIcpCovBlock points, tblk_off its blocks of 256).
struct IcpKnnDesc {
  int32_t k;          // neighbours asked for (self k-NN: k; statistical removal: nb_neighbors; radius removal: nb_points)
  int32_t ring_cap;   // rings 0 .. ring_cap - 1 are searched on the grid; 0: every query takes the whole-cloud route
  int64_t out_off;    // first slot of this cloud in the packed n x k outputs (self k-NN)
  double edge;        // h: the grid's cell edge is at least h (1 + 1e-6), the margin of set_grid
  double ratio;       // std_ratio (statistical removal)
};

// One problem of a two-cloud neighbour search (kernels_search.hip), beside its IcpDesc: the data cloud is the
// descriptor's "target" (n_t, t_off, the grid), the query set its "source" (n_s, s_off in the packed queries); blk_off /
// nblk count the blocks of queries (kIcpCovBlock per block for k-NN and hybrid, 256 for the radius search).
struct IcpSearchDesc {
  int32_t k;          // k (k-NN) or max_nn (hybrid)
  int32_t ring_cap;   // k-NN: rings r0 .. r0 + ring_cap - 1 are searched on the grid; 0: every query is scanned
  int32_t fill;       // radius: 1 when the caller gave arrays for this problem
  int32_t pad;
  int64_t out_off;    // k-NN, hybrid: first slot of the packed n_query x k outputs; radius: first entry of the problem
  int64_t capacity;   // radius: entries the caller's arrays hold; the problem is filled iff fill && capacity >= total
  double edge;        // k-NN: h of IcpKnnDesc::edge
};

// One cloud of a normal-estimation call, beside its IcpDesc (the cloud is the descriptor's "target"; hybrid search: the
// grid and r2 of the radius, as in covariance estimation; k-NN search: an IcpKnnDesc with k = max_nn beside it).  Offsets
// count rows (points) of the packed outputs.
struct IcpNormalDesc {
  int32_t max_nn;     // 3 .. kIcpCovMaxNN
  int32_t orient;     // 0 none, 1 towards the point ref, 2 along the direction ref
  int64_t nrm_off;    // first row of this cloud's normals
  int64_t cov_off;    // first row of its raw covariances, -1: not asked for
  int64_t eig_off;    // first row of its eigenvalues, -1: not asked for
  double ref[3];
};

// One piece of a boundary-point call (kernels_boundary.hip), beside its IcpDesc and IcpSearchDesc.
struct IcpBoundaryDesc {
  double threshold;   // (angle_threshold pi) / 180.0
  int32_t cloud;      // the cloud of the piece: its entry of the n_boundary counters
  int32_t pad;
};

// One cloud of a colour-gradient pass, beside its IcpDesc (the cloud is the descriptor's "target": the grid and r2 of the
// gradient radius; blk_off / nblk count its blocks of kIcpCovBlock points).
struct IcpGradDesc {
  int32_t max_nn;     // 4 .. kIcpCovMaxNN
  int32_t pad;
};

// One problem of a call that holds a Colored-ICP problem, beside its IcpDesc; read for method 3 only.
struct IcpColorDesc {
  double sg, sp;      // sqrt(lambda_geometric), sqrt(1 - lambda_geometric)
};

// What the mode-3 correspondence kernel gathers from besides the arrays of the other modes (kernel argument, by value).
struct IcpColorArgs {
  const IcpColorDesc* cd;  // one per problem
  const double* rec_t;     // 4 doubles per target point at t_off: the colour gradient, then the intensity
  const double* int_s;     // one intensity per source point at s_off
};

// Grid cell of one coordinate; host (descriptor set-up) and device (index build, search) run the same expression.
__host__ __device__ inline int64_t icp_cell(double x, double origin, double inv_h) {
  double v = floor((x - origin) * inv_h);
  v = v < -2.0 ? -2.0 : (v > 1099511627776.0 ? 1099511627776.0 : v);
  return (int64_t)v;
}

__host__ __device__ inline int64_t icp_bucket(int64_t cx, int64_t cy, int64_t cz, int64_t mask) {
  uint64_t k = (uint64_t)cx * 0x9E3779B97F4A7C15ull ^ (uint64_t)cy * 0xC2B2AE3D27D4EB4Full ^
               (uint64_t)cz * 0x165667B19E3779F9ull;
  k ^= k >> 31;
  k *= 0xD6E8FEB86659FD93ull;
  k ^= k >> 32;
  return (int64_t)(k & (uint64_t)mask);
}

#if defined(__HIPCC__)
// The point of this thread's map block in a launch over list pieces (kernels_fpfh.hip, kernels_boundary.hip: n_hyb blocks
// of hybrid pieces, then the blocks of the k-NN pieces, each kind counting blk_off from its own start): the piece p and
// the first point i0 of the block inside it.
__device__ __forceinline__ int list_block_piece(const IcpDesc* __restrict__ descs, const int32_t* __restrict__ blk_prob,
                                                int n_hyb, int64_t* i0) {
  const int blk = (int)blockIdx.x;
  const int p = blk_prob[blk];
  const int rel = blk < n_hyb ? blk : blk - n_hyb;
  *i0 = (int64_t)(rel - descs[p].blk_off) * kIcpCovBlock;
  return p;
}
#endif

void launch_icp_index(hipStream_t s, const IcpDesc* d_desc, const int32_t* d_tblk_prob, int n_tblk, int batch,
                      const double* d_q, int32_t* d_tbucket, int32_t* d_bcount, int32_t* d_bstart,
                      int32_t* d_cursor, double* d_qs, int32_t* d_qj);
void launch_icp_iteration(hipStream_t s, const IcpDesc* d_desc, IcpState* d_state, const int32_t* d_blk_prob,
                          int n_blk, int batch, double* d_x, const double* d_qs, const int32_t* d_qj,
                          const int32_t* d_bstart, const double* d_normals, const double* d_cov_s,
                          const double* d_cov_t, int mode, int32_t* d_match, double* d_partials);
// One iteration of a call that holds a Colored-ICP problem (mode 3; kernels_icp.hip): launch_icp_iteration's arguments
// and what the coloured branch gathers from.
void launch_icp_iteration_color(hipStream_t s, const IcpDesc* d_desc, IcpState* d_state, const int32_t* d_blk_prob,
                                int n_blk, int batch, double* d_x, const double* d_qs, const int32_t* d_qj,
                                const int32_t* d_bstart, const double* d_normals, const double* d_cov_s,
                                const double* d_cov_t, int32_t* d_match, double* d_partials, const IcpColorArgs& col);
// Colour gradients of the indexed clouds (the Colored-ICP contract of include/teaser_hip.h): point i of a cloud reads its
// normal at d_normals[3 (t_off + i)] and the intensities at d_rec[4 (t_off + .) + 3], and writes d_rec[4 (t_off + i) + 0..2].
void launch_icp_color_gradients(hipStream_t s, const IcpDesc* d_desc, const IcpGradDesc* d_gd, const int32_t* d_blk_prob,
                                int n_blk, int max_nn, const double* d_q, const double* d_qs, const int32_t* d_qj,
                                const int32_t* d_bstart, const double* d_normals, double* d_rec);
void launch_icp_covariances(hipStream_t s, const IcpDesc* d_desc, const IcpCovDesc* d_cov, const int32_t* d_blk_prob,
                            int n_blk, int max_nn, const double* d_q, const double* d_qs, const int32_t* d_qj,
                            const int32_t* d_bstart, double* d_out);
// Self k-NN on the indexed clouds.  avg == nullptr: idx / d2 (n x k per cloud at IcpKnnDesc::out_off) are written;
// otherwise avg[t_off + i] (statistical removal's mean distance).  work: 2 int32 per point; work_count: one int32,
// cleared by the caller, holds the number of queries the whole-cloud route served when the launches have run.
void launch_icp_self_knn(hipStream_t s, const IcpDesc* d_desc, const IcpKnnDesc* d_knn, const int32_t* d_blk_prob,
                         int n_blk, int top_k, const double* d_q, const double* d_qs, const int32_t* d_qj,
                         const int32_t* d_bstart, int32_t* d_idx, double* d_d2, double* d_avg, int32_t* d_work,
                         int32_t* d_work_count);
// Normal estimation on the indexed clouds (the normals contract of include/teaser_hip.h): the normals at
// IcpNormalDesc::nrm_off of d_nrm, the raw covariances / ascending eigenvalues of the clouds that ask for them at
// cov_off / eig_off of d_cov / d_eig.  Hybrid search: one launch over n_blk blocks of kIcpCovBlock points.  k-NN search:
// the ring and scan launches of self k-NN with the covariance consumer (work / work_count as there).
void launch_icp_normals_hybrid(hipStream_t s, const IcpDesc* d_desc, const IcpNormalDesc* d_nd,
                               const int32_t* d_blk_prob, int n_blk, int max_nn, const double* d_q, const double* d_qs,
                               const int32_t* d_qj, const int32_t* d_bstart, double* d_nrm, double* d_cov,
                               double* d_eig);
void launch_icp_normals_knn(hipStream_t s, const IcpDesc* d_desc, const IcpKnnDesc* d_knn, const IcpNormalDesc* d_nd,
                            const int32_t* d_blk_prob, int n_blk, int top_k, const double* d_q, const double* d_qs,
                            const int32_t* d_qj, const int32_t* d_bstart, double* d_nrm, double* d_cov, double* d_eig,
                            int32_t* d_work, int32_t* d_work_count);
// mean, std, threshold (stats: 3 doubles per cloud) from avg, then the mask and the kept count (cleared by the caller)
void launch_icp_statistical(hipStream_t s, const IcpDesc* d_desc, const IcpKnnDesc* d_knn,
                            const int32_t* d_tblk_prob, int n_tblk, int batch, const double* d_avg,
                            double* d_partials, double* d_stats, uint8_t* d_keep, int32_t* d_kept);
// count of points with d2 < r2 (27 cells of the grid built for r), the mask and the kept count (cleared by the caller)
void launch_icp_radius_count(hipStream_t s, const IcpDesc* d_desc, const IcpKnnDesc* d_knn,
                             const int32_t* d_tblk_prob, int n_tblk, const double* d_q, const double* d_qs,
                             const int32_t* d_bstart, int32_t* d_count, uint8_t* d_keep, int32_t* d_kept);
// Neighbour search between two clouds (kernels_search.hip; the contract "Neighbour search" of include/teaser_hip.h).
// d_x: the packed queries (IcpDesc::s_off), the data clouds are indexed.  k-NN: n_query x k slots per problem at
// IcpSearchDesc::out_off of d_idx / d_d2; work: 2 int32 per query, work_count as for self k-NN.
void launch_icp_search_knn(hipStream_t s, const IcpDesc* d_desc, const IcpSearchDesc* d_sd, const int32_t* d_blk_prob,
                           int n_blk, int top_k, const double* d_x, const double* d_q, const double* d_qs,
                           const int32_t* d_qj, const int32_t* d_bstart, int32_t* d_idx, double* d_d2, int32_t* d_work,
                           int32_t* d_work_count);
// Hybrid: the rows as above and d_cnt[s_off + i] = the number written.
void launch_icp_search_hybrid(hipStream_t s, const IcpDesc* d_desc, const IcpSearchDesc* d_sd,
                              const int32_t* d_blk_prob, int n_blk, int top_nn, const double* d_x, const double* d_qs,
                              const int32_t* d_qj, const int32_t* d_bstart, int32_t* d_idx, double* d_d2,
                              int32_t* d_cnt);
// Radius: d_count / d_prefix per query at s_off (the count and its exclusive sum over the problem), d_total per problem;
// the problems that are filled get their rows in ascending (d2, j) at out_off + prefix of d_idx / d_d2, through the
// unordered d_tmp_d2 / d_tmp_j.  entries: the sum of the entries reserved (0: the count half only, no array is touched).
void launch_icp_search_radius(hipStream_t s, const IcpDesc* d_desc, const IcpSearchDesc* d_sd,
                              const int32_t* d_blk_prob, int n_blk, int batch, int64_t entries, const double* d_x,
                              const double* d_qs, const int32_t* d_qj, const int32_t* d_bstart, int32_t* d_count,
                              int64_t* d_prefix, int64_t* d_total, double* d_tmp_d2, int32_t* d_tmp_j, int32_t* d_idx,
                              double* d_d2);
// The Open3D-form FPFH (kernels_fpfh.hip; the contract "FPFH (Open3D form)" of include/teaser_hip.h).  The descriptors
// are those of the PIECES of the clouds (n_s points from s_off of d_q; the cloud itself at t_off), the block map holds
// n_hyb blocks of hybrid pieces, then n_knn blocks of k-NN pieces, each kind counting blk_off from its own start; the
// lists (k slots per point at IcpSearchDesc::out_off, index -1 behind the valid entries) are the search launchers'.
// SPFH: row s_off + i of d_spfh from the points and normals of the cloud.  FPFH: row s_off + i of d_fpfh from the SPFH
// rows of the whole cloud, which must be complete.
void launch_icp_fpfh_spfh(hipStream_t s, const IcpDesc* d_desc, const IcpSearchDesc* d_sd, const int32_t* d_blk_prob,
                          int n_hyb, int n_knn, const double* d_q, const double* d_normals, const int32_t* d_list_idx,
                          double* d_spfh);
void launch_icp_fpfh(hipStream_t s, const IcpDesc* d_desc, const IcpSearchDesc* d_sd, const int32_t* d_blk_prob,
                     int n_hyb, int n_knn, const int32_t* d_list_idx, const double* d_list_d2, const double* d_spfh,
                     double* d_fpfh);
// Boundary points (kernels_boundary.hip; the contract "Boundary points" of include/teaser_hip.h) over the pieces and
// lists of the FPFH launches above, with an IcpBoundaryDesc per piece: for point s_off + i the byte d_mask, and where the
// arrays are not NULL its max_gap and its list length m; the boundary points of cloud c are ADDED to d_n_boundary[c].
void launch_icp_boundary(hipStream_t s, const IcpDesc* d_desc, const IcpSearchDesc* d_sd, const IcpBoundaryDesc* d_bd,
                         const int32_t* d_blk_prob, int n_hyb, int n_knn, const double* d_q, const double* d_normals,
                         const int32_t* d_list_idx, uint8_t* d_mask, double* d_max_gap, int32_t* d_count,
                         int32_t* d_n_boundary);
// Depth frames (kernels_rgbd.hip; the contract "Depth frames" of include/teaser_hip.h; the records are those of
// icp_rgbd_device.h).  Unprojection: three launches over the n_tiles tiles of all frames (d_tile_frame: the frame of
// every tile) -- the rows of every tile into d_tile_count, their exclusive sums per frame into d_tile_start and the
// frames' counts into d_count, then the rows themselves at the frames' offsets of d_points / d_colors / d_pixels.
struct IcpFrameDesc;
struct IcpProjDesc;
void launch_icp_rgbd_unproject(hipStream_t s, const IcpFrameDesc* d_frames, const int32_t* d_tile_frame, int n_tiles,
                               int batch, const unsigned char* d_in, int32_t* d_tile_count, int32_t* d_tile_start,
                               int32_t* d_count, double* d_points, double* d_colors, int32_t* d_pixels);
// Projection: the scatter over n_blk blocks of points into the key image (filled with ones by the caller), then the
// resolve over n_tiles blocks of pixels: depth, and where a problem asks for them colour and index; the non-empty pixels
// of problem b are ADDED to d_n_hit[b].
void launch_icp_rgbd_project(hipStream_t s, const IcpProjDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                             const int32_t* d_tile_prob, int n_tiles, const double* d_points, const double* d_colors,
                             uint64_t* d_keys, float* d_depth, float* d_color_img, int32_t* d_index_img,
                             int32_t* d_n_hit);
// The information matrices of the problems whose matches (d_match, written by the mode-0 correspondence pass over the
// same block map) and targets as given (d_q) are on the device: d_partials takes kIcpInfoSums doubles per block,
// d_info 36 per problem (row-major 6 x 6).  kernels_icp_information.hip.
void launch_icp_information(hipStream_t s, const IcpDesc* d_desc, const int32_t* d_blk_prob, int n_blk, int batch,
                            const double* d_q, const int32_t* d_match, double* d_partials, double* d_info);
void launch_icp_live(hipStream_t s, const IcpState* d_state, int batch, int32_t* d_live);

}  // namespace thip
