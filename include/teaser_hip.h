/*
 * teaser_hip.h -- C ABI of the MI355X-native TEASER++ registration hot path.
 *
 * This is the drop-in boundary for teaser::RobustRegistrationSolver::solve() and nothing else
 * (TIM build + scale pruning -> inlier graph -> maximum clique -> GNC-TLS rotation -> TLS
 * translation).  Plain pointers and sizes only; no C++/torch/Eigen types.  The reference has no
 * FFI layer of its own: its boundary is the C++ class in teaser/include/teaser/registration.h,
 * which pybind11 (python/teaserpp_python/teaserpp_python.cc:82-177) and MEX
 * (matlab/teaser_mex.cc:207-218) wrap.  Each entry point below cites the reference interface it
 * replaces (paths relative to the reference checkout).  INTEGRATION.md shows the bindings.
 *
 * Layout conventions
 *   - point clouds: `3 x N` column-major doubles, i.e. x0 y0 z0 x1 y1 z1 ... -- exactly
 *     Eigen::Matrix<double,3,Eigen::Dynamic>::data() (registration.h:576-577), zero-copy.
 *   - rotation: 9 doubles, ROW-major (R(r,c) = rotation[3*r+c]).
 *   - index lists: int32, ascending, in the reference's meaning (see each getter).
 *   - adjacency bitmap: n rows of W = (n+63)/64 uint64 words, bit j of row i = edge (i,j).
 *
 * Threading: one handle = one device + one HIP stream; a handle is NOT re-entrant, distinct
 * handles are independent (same contract as one RobustRegistrationSolver object).  Unlike the
 * reference object (registration.cc:702-704 mutates the rotation solver), a handle is reusable.
 *
 * Errors: every call returns a teaser_hip_status; solve never throws.  A valid==0 solution with
 * status OK is the reference's soft failure (clique size <= 1, registration.cc:643-647).
 *
 * Problem-size limits.  The routes follow the largest problem of a
 * batch (max_n): above 65536 correspondences the inlier graph is built by the all-FP64 K1 kernel
 * and a separate degree pass instead of the matrix-core filter, the degree closure is off, and the
 * colouring bound uses the vertex-centric rounds only; every problem of such a batch takes these
 * routes, with the same results.  Refused with TEASER_HIP_ERR_UNSUPPORTED (the handle stays usable):
 *   - inlier_selection_mode = KCORE_HEU when max_n > 65536 (solve and teaser_hip_max_clique;
 *     before any work);
 *   - estimate_scaling when n > 46341 (the reference's own `int` limit, registration.cc:47);
 *   - rotation_tim_graph = COMPLETE when sum over the batch of n(n-1)/2 + 2 > 2^31 (before any
 *     work).  This is stricter than the reference, which builds COMPLETE TIMs over the maximum
 *     clique only (registration.cc:690-693); here they are sized for all n points.
 */
#ifndef TEASER_HIP_H_
#define TEASER_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEASER_HIP_ABI_VERSION 1

#if defined(__GNUC__)
#define TEASER_HIP_API __attribute__((visibility("default")))
#else
#define TEASER_HIP_API
#endif

typedef enum teaser_hip_status {
  TEASER_HIP_OK = 0,
  TEASER_HIP_ERR_BAD_ARG = 1,
  TEASER_HIP_ERR_HIP = 2,          /* a HIP runtime call failed: teaser_hip_last_error() */
  TEASER_HIP_ERR_NO_DEVICE = 3,    /* no gfx950 device visible: the product never falls back to CPU */
  TEASER_HIP_ERR_UNSUPPORTED = 4,  /* parameter value outside the reference's own domain */
  TEASER_HIP_ERR_TIME_LIMIT = 5,   /* max_clique_time_limit hit; incumbent returned (graph.cc:44) */
  TEASER_HIP_ERR_SCRATCH = 6,      /* exact clique search ran out of device scratch */
  TEASER_HIP_ERR_OOM = 7,
  TEASER_HIP_ERR_BUSY = 8          /* every lane holds a submitted batch: teaser_hip_wait first */
} teaser_hip_status;

/* enums: registration.h:382-412 (same numeric values) */
enum { TEASER_ROT_GNC_TLS = 0, TEASER_ROT_FGR = 1, TEASER_ROT_QUATRO = 2 };
enum { TEASER_INLIER_PMC_EXACT = 0, TEASER_INLIER_PMC_HEU = 1, TEASER_INLIER_KCORE_HEU = 2,
       TEASER_INLIER_NONE = 3 };
enum { TEASER_TIM_CHAIN = 0, TEASER_TIM_COMPLETE = 1 };

/* POD mirror of teaser::RobustRegistrationSolver::Params (registration.h:419-514): same fields,
 * same order, same defaults (teaser_hip_params_default). */
typedef struct teaser_params_c {
  double noise_bound;                    /* 0.01 */
  double cbar2;                          /* 1 */
  int32_t estimate_scaling;              /* 1 */
  int32_t rotation_estimation_algorithm; /* TEASER_ROT_GNC_TLS */
  double rotation_gnc_factor;            /* 1.4 */
  int64_t rotation_max_iterations;       /* 100 */
  double rotation_cost_threshold;        /* 1e-6 */
  int32_t rotation_tim_graph;            /* TEASER_TIM_CHAIN */
  int32_t inlier_selection_mode;         /* TEASER_INLIER_PMC_EXACT */
  double kcore_heuristic_threshold;      /* 0.5 */
  int32_t use_max_clique;                /* deprecated, 1 */
  int32_t max_clique_exact_solution;     /* deprecated, 1 */
  double max_clique_time_limit;          /* 3600 s */
  int32_t max_clique_num_threads;        /* accepted, ignored on the GPU */
} teaser_params_c;

/* teaser::RegistrationSolution (registration.h:32-39) + the scalars behind the getters. */
typedef struct teaser_solution_c {
  int32_t valid;                 /* RegistrationSolution::valid */
  int32_t status;                /* teaser_hip_status of this problem */
  double scale;
  double rotation[9];            /* row-major */
  double translation[3];
  int32_t n;                     /* correspondences of this problem */
  int32_t clique_size;           /* getInlierMaxClique().size() */
  int32_t n_rotation_inliers;    /* getRotationInliers().size() */
  int32_t n_translation_inliers; /* getTranslationInliers().size() */
  double gnc_cost;               /* getGNCRotationCostAtTermination(), registration.h:609-611 */
  int32_t gnc_iterations;
  int32_t clique_exact_run;      /* 1 iff the device B&B had to run (bounds did not close) */
  int32_t heuristic_size;        /* lower bound found by the greedy stage */
  int32_t colour_uncoloured;     /* global colouring bound: survivors left without one of the
                                    heuristic_size colours (0: greedy clique proven maximum without
                                    search; > 0: they were the only B&B roots; -1: stage not run;
                                    -2: the degree closure decided the problem -- lb = ub from the vertex
                                    degrees, graph.cc:83-102 -- before any heuristic ran; -3: the same, and
                                    the maximum clique it returns is proven maximum but not the only one) */
  int64_t num_edges;             /* edges of the inlier graph */
} teaser_solution_c;

/* Per-stage device time of the last solve call (HIP events on the stream the kernels run on),
 * enabled by teaser_hip_set_profiling(h, level): 1 = every stage, 2 = K1 only (the kernel itself,
 * and its pre-pass / fix-up: three event pairs per solve, what bench.py keeps on inside its timed
 * region).  Milliseconds, summed over the
 * launches of that stage. */
typedef struct teaser_profile_c {
  float h2d_ms;
  float tim_graph_ms;    /* K1 main kernel only: TIM norms + prune + adjacency bitmap */
  int32_t tim_graph_launches;
  float degree_ms;
  float heuristic_ms;
  float peel_ms;
  float exact_ms;
  float rotation_ms;
  float translation_ms;
  float d2h_ms;
  float total_ms;
  int64_t tim_graph_pairs; /* unordered pairs evaluated by K1 in the last call */
  int64_t tim_graph_bytes; /* algorithmic bytes of K1: 48 n + 8 n ceil(n/64), summed over problems */
  float colour_ms;         /* global colouring bound (only for problems the peel did not close) */
  float tim_aux_ms;        /* K1 pre-pass (bbox, operand packing) + FP64 fix-up + overflow clear */
} teaser_profile_c;

typedef struct teaser_hip_solver teaser_hip_solver;

/* Fills the defaults of registration.h:419-514. */
TEASER_HIP_API int32_t teaser_hip_params_default(teaser_params_c* params);

/* RobustRegistrationSolver(const Params&) (registration.h:548, registration.cc:507-510).
 * device < 0: current device.  Fails with TEASER_HIP_ERR_NO_DEVICE when no GPU is visible. */
TEASER_HIP_API int32_t teaser_hip_solver_create(const teaser_params_c* params, int32_t device,
                                 teaser_hip_solver** out);
TEASER_HIP_API int32_t teaser_hip_solver_destroy(teaser_hip_solver* h);

/* reset(const Params&) (registration.h:891) / getParams() (registration.h:914). */
TEASER_HIP_API int32_t teaser_hip_solver_reset(teaser_hip_solver* h, const teaser_params_c* params);
TEASER_HIP_API int32_t teaser_hip_solver_get_params(const teaser_hip_solver* h, teaser_params_c* params);

/* RegistrationSolution solve(const Matrix<double,3,Dyn>& src, const Matrix<double,3,Dyn>& dst)
 * (registration.h:576-577, registration.cc:568-737).  src/dst are HOST pointers, 3 x n
 * column-major; borrowed for the duration of the call.  n < 2 gives valid = 0. */
TEASER_HIP_API int32_t teaser_hip_solve(teaser_hip_solver* h, const double* src, const double* dst, int32_t n,
                         teaser_solution_c* out);

/* Same contract with DEVICE pointers (inputs already resident in HBM, on h's device). */
TEASER_HIP_API int32_t teaser_hip_solve_device(teaser_hip_solver* h, const double* d_src, const double* d_dst,
                                int32_t n, teaser_solution_c* out);

/* solve(const PointCloud&, const PointCloud&, std::vector<std::pair<int,int>>)
 * (registration.h:567-569, registration.cc:553-566): float xyz clouds (geometry.h:15-23) and
 * index pairs; gathers with float -> double widening, then solves. */
TEASER_HIP_API int32_t teaser_hip_solve_correspondences(teaser_hip_solver* h, const float* src_cloud_xyz,
                                         int32_t n_src, const float* dst_cloud_xyz, int32_t n_dst,
                                         const int32_t* corr_pairs /* 2*C: src_idx,dst_idx */,
                                         int32_t n_corr, teaser_solution_c* out);

/* Batched mode (no reference equivalent; the reference solves one problem per object):
 * `batch` independent problems, problem b has n[b] correspondences.  Host pointers per problem. */
TEASER_HIP_API int32_t teaser_hip_solve_batch(teaser_hip_solver* h, const double* const* src,
                               const double* const* dst, const int32_t* n, int32_t batch,
                               teaser_solution_c* out /* [batch] */);

/* Batched, inputs packed and device-resident: problem b occupies points
 * [offset[b], offset[b]+n[b]) of d_src/d_dst (3 doubles per point); offsets are HOST arrays. */
TEASER_HIP_API int32_t teaser_hip_solve_batch_device(teaser_hip_solver* h, const double* d_src,
                                      const double* d_dst, const int64_t* point_offset,
                                      const int32_t* n, int32_t batch, teaser_solution_c* out);

/* Asynchronous batches (no reference equivalent).  submit enqueues everything of a batched solve
 * that needs no host sync on one of the handle's LANES (child contexts with their own HIP stream
 * and arenas, used round-robin; teaser_hip_set_pipeline_depth, default 2) and returns a ticket;
 * wait blocks on that lane's one host sync, finishes the rare bound-closing work and writes the
 * solutions.  With 2 batches in flight the host enqueues batch k+1 while the GPU runs batch k,
 * and the latency-bound tail of batch k (clique, GNC, TLS: one workgroup per problem) shares the GPU
 * with batch k+1's K1.  Results are identical to teaser_hip_solve_batch_device (same kernels).
 * Since round 4 the second half of a batch (the lane's host sync and, when the peel left problems open, the
 * colouring bound / exact search with their own syncs) runs on an INTERNAL finisher thread of the lane as soon
 * as the batch is enqueued; wait collects its result.  The caller's contract is unchanged: ONE calling thread,
 * tickets in any order; the threads are joined by teaser_hip_solver_destroy / teaser_hip_set_pipeline_depth.
 * Lanes want one hardware queue each.  HIP multiplexes its streams onto GPU_MAX_HW_QUEUES hardware queues (default
 * 4) and reads that variable ONCE, at the process's first HIP call: a C / C++ caller that wants more than four
 * batches in flight exports GPU_MAX_HW_QUEUES (8 is enough for depth <= 7) before that call -- the library never
 * modifies the environment (the Python package sets it as a default before it loads the library).  With fewer
 * queues than lanes the results are the same; lanes then share queues and overlap less (a one-time note on stderr).
 *   flags = TEASER_HIP_INPUT_DEVICE: src/dst are packed DEVICE arrays (as solve_batch_device), which
 *           must stay valid and unmodified until the matching wait;
 *   flags = TEASER_HIP_INPUT_HOST:   src/dst are packed HOST arrays of the same layout (problem b =
 *           points [offset[b], offset[b]+n[b])); page-locked memory (teaser_hip_host_alloc: memory pinned by
 *           ANOTHER HIP runtime in the process is pageable to this one) is copied asynchronously at PCIe speed
 *           on a stream of the handle that is otherwise idle, and
 *           must stay valid until wait.  ONE host batch beyond the lanes is accepted (depth + 1 in
 *           flight): its copy starts at once, hidden behind the kernels of the batches on the lanes,
 *           and it is enqueued on the first lane that frees up, at the next submit / wait call --
 *           a throughput caller keeps depth + 1 host batches outstanding and pays no PCIe time.
 * point_offset / n are host arrays, copied at submit.  Tickets may be waited for in any order
 * (a batch still staged behind the lanes answers TEASER_HIP_ERR_BUSY until an earlier ticket has been
 * waited for), each exactly once; after wait the getters address that batch until the next submit /
 * wait / solve.  TEASER_HIP_ERR_BUSY: all lanes are in flight (and, for host inputs, one batch is staged). */
enum { TEASER_HIP_INPUT_DEVICE = 0, TEASER_HIP_INPUT_HOST = 1 };
TEASER_HIP_API int32_t teaser_hip_submit_batch(teaser_hip_solver* h, const double* src, const double* dst,
                                const int64_t* point_offset, const int32_t* n, int32_t batch,
                                int32_t flags, int32_t* ticket);
TEASER_HIP_API int32_t teaser_hip_wait(teaser_hip_solver* h, int32_t ticket, teaser_solution_c* out /* [batch] */);
TEASER_HIP_API int32_t teaser_hip_set_pipeline_depth(teaser_hip_solver* h, int32_t depth /* 1..16 */);

/* One process, several devices ("a batch call may fan out across all visible
 * devices"): a multi-solver owns one handle per listed device (a device may be listed twice) and one
 * host thread per handle; solve_batch cuts the batch into contiguous blocks, one per handle, and
 * runs them concurrently (host pointers per problem, as teaser_hip_solve_batch).  No collective:
 * the problems are independent and the solutions land in the caller's array.  The getters of
 * problem p are reached through teaser_hip_multi_route(mh, p, &h, &local) -> h's getters with `local`. */
typedef struct teaser_hip_multi teaser_hip_multi;
TEASER_HIP_API int32_t teaser_hip_multi_create(const teaser_params_c* params, const int32_t* devices,
                                int32_t n_devices /* 0: every visible device */, teaser_hip_multi** out);
TEASER_HIP_API int32_t teaser_hip_multi_destroy(teaser_hip_multi* mh);
TEASER_HIP_API int32_t teaser_hip_multi_solve_batch(teaser_hip_multi* mh, const double* const* src,
                                     const double* const* dst, const int32_t* n, int32_t batch,
                                     teaser_solution_c* out /* [batch] */);
TEASER_HIP_API int32_t teaser_hip_multi_route(teaser_hip_multi* mh, int32_t problem, teaser_hip_solver** h,
                               int32_t* local_problem);
TEASER_HIP_API int32_t teaser_hip_multi_device_count(const teaser_hip_multi* mh);

/* Rank mode: one PROCESS per GPU, the problems of a job cut into contiguous shards, every rank
 * solving its shard with teaser_hip_solve_batch on its own handle, and ONE all-gather of the fixed-size solution
 * records over RCCL (xGMI inside a node) -- the compiled-caller counterpart of the Python host's
 * batched.solve_sharded (torch.distributed).  The reference has no multi-process mode (one problem per
 * RobustRegistrationSolver object, registration.cc:568-737); there is no data-path collective.
 *   comm_shard      rank r of `world` owns problems [first, last): contiguous, balanced (the first total % world
 *                   ranks own one more)
 *   comm_unique_id  rank 0 makes the RCCL id (TEASER_HIP_COMM_ID_BYTES bytes) and hands it to the other ranks by
 *                   whatever the job already has (MPI_Bcast, a file, a socket).  The calling process hosts RCCL's
 *                   bootstrap root: it must stay alive until every rank's comm_create has returned
 *   comm_last_error(NULL) = why the last failed comm_create of this process failed
 *   comm_create     collective over all ranks; device < 0: the current device
 *   comm_gather_solutions  collective: `local` = this rank's records in shard order (n_local = last - first),
 *                   `all` [total] receives every rank's records in problem order, the same on every rank
 * librccl is loaded on first use: TEASER_HIP_ERR_UNSUPPORTED when it is absent. */
#define TEASER_HIP_COMM_ID_BYTES 128
typedef struct teaser_hip_comm teaser_hip_comm;
TEASER_HIP_API int32_t teaser_hip_comm_shard(int64_t total, int32_t rank, int32_t world, int64_t* first, int64_t* last);
TEASER_HIP_API int32_t teaser_hip_comm_unique_id(uint8_t* id /* [TEASER_HIP_COMM_ID_BYTES] */);
TEASER_HIP_API int32_t teaser_hip_comm_create(const uint8_t* id, int32_t rank, int32_t world, int32_t device,
                               teaser_hip_comm** out);
TEASER_HIP_API int32_t teaser_hip_comm_destroy(teaser_hip_comm* c);
TEASER_HIP_API int32_t teaser_hip_comm_gather_solutions(teaser_hip_comm* c, const teaser_solution_c* local,
                                         int64_t n_local, int64_t total, teaser_solution_c* all /* [total] */);
/* collective: the INDEX SETS behind the parity bar -- getInlierMaxClique, getRotationInliers, getTranslationInliers
 * (registration.h:770, 713, 744) -- of every problem on every rank, in ONE all-gather of padded int32 blocks.
 * `h` is the solver whose last solve_batch produced this rank's n_local problems (the lists are read through the
 * getters below); k_max >= the longest list of ANY problem, the same on every rank (take it from the gathered
 * solution records: max over clique_size, n_rotation_inliers, n_translation_inliers).  lens [total][3] receives
 * the list lengths, indices [total][3][k_max] the lists in that order, padded with -1.  A rank holding a list
 * longer than k_max still takes part (zeroed block) and returns BAD_ARG afterwards. */
TEASER_HIP_API int32_t teaser_hip_comm_gather_indices(teaser_hip_comm* c, teaser_hip_solver* h, int64_t n_local,
                                       int64_t total, int32_t k_max, int32_t* lens, int32_t* indices);
TEASER_HIP_API const char* teaser_hip_comm_last_error(const teaser_hip_comm* c);

/* Getters on the last solve call; `problem` indexes the batch (0 for single solves).  Each copies
 * into buf when buf != NULL and *len (capacity in elements on entry) suffices, and always writes
 * the required length to *len.
 *   max_clique           getInlierMaxClique()        (registration.h:770)  sorted input indices
 *   rotation_inliers     getRotationInliers()        (registration.h:713)  indices of rotation TIMs
 *   translation_inliers  getTranslationInliers()     (registration.h:744)  positions in the clique
 *   input_ordered_translation_inliers  getInputOrderedTranslationInliers() (registration.h:752-763)
 *   inlier_graph_bitmap  the adjacency behind getInlierGraph() (registration.h:772), as bitmap
 *   degrees              vertex degrees of the inlier graph */
TEASER_HIP_API int32_t teaser_hip_get_max_clique(teaser_hip_solver* h, int32_t problem, int32_t* buf, int64_t* len);
TEASER_HIP_API int32_t teaser_hip_get_rotation_inliers(teaser_hip_solver* h, int32_t problem, int32_t* buf,
                                        int64_t* len);
TEASER_HIP_API int32_t teaser_hip_get_translation_inliers(teaser_hip_solver* h, int32_t problem, int32_t* buf,
                                           int64_t* len);
TEASER_HIP_API int32_t teaser_hip_get_input_ordered_translation_inliers(teaser_hip_solver* h, int32_t problem,
                                                         int32_t* buf, int64_t* len);
TEASER_HIP_API int32_t teaser_hip_get_inlier_graph_bitmap(teaser_hip_solver* h, int32_t problem, uint64_t* buf,
                                           int64_t* len /* words */);
TEASER_HIP_API int32_t teaser_hip_get_degrees(teaser_hip_solver* h, int32_t problem, int32_t* buf, int64_t* len);
/* DIAGNOSTIC (tests), on no hot path: the rows of a problem's graph as the device arena holds them -- n rows on a
 * stride of *stride_words words (ceil(n / 64) rounded up to a multiple of 8: 64 bytes), len = n x stride.  The words
 * ceil(n / 64) .. stride - 1 of a row are padding and zero.  Unlike teaser_hip_get_inlier_graph_bitmap the call
 * mirrors nothing: behind a solve that stored the upper triangle only, the words of row r in front of r / 64 are
 * whatever an earlier solve left there.  Behind a solve whose K1 stored no row at all (teaser_hip_get_graph_route: 2)
 * it does what that getter does: every row of the batch is rebuilt first, once, both halves and the padding.
 * Both getters rebuild from the handle's own arenas: the caller's point arrays are not read again and need not
 * outlive the solve. */
TEASER_HIP_API int32_t teaser_hip_get_inlier_graph_rows(teaser_hip_solver* h, int32_t problem, uint64_t* buf,
                                         int64_t* len /* words */, int32_t* stride_words);
/* DIAGNOSTIC (tests): how the last solve's K1 stored the graph of the batch `problem` belongs to -- 0: both halves,
 * 1: the upper triangle (the lower one is mirrored on demand), 2: nothing (the degree closure worked from the points;
 * rows are rebuilt on demand) -- and how many problems rebuilds have covered since that solve.  Which route a solve
 * takes is not observable in any result.  Either pointer may be NULL. */
TEASER_HIP_API int32_t teaser_hip_get_graph_route(teaser_hip_solver* h, int32_t problem, int32_t* route, int64_t* rebuilt);

/* Stage entry points (registration.h:584-601), host pointers, 3 x K column-major TIMs/points:
 *   solveForRotation   -> GNCTLSRotationSolver::solveForRotation (registration.cc:764-866);
 *                         noise_bound is the value the rotation solver holds.
 *   solveForTranslation-> TLSTranslationSolver::solveForTranslation (registration.cc:445-471)
 *   scalar TLS         -> ScalarTLSEstimator::estimate (registration.cc:21-88)
 * inlier masks are one byte per element (0/1); may be NULL. */
TEASER_HIP_API int32_t teaser_hip_solve_for_rotation(teaser_hip_solver* h, const double* src, const double* dst,
                                      int32_t k, double noise_bound, double* rotation_rowmajor,
                                      uint8_t* inlier_mask, double* cost, int32_t* iterations);
TEASER_HIP_API int32_t teaser_hip_solve_for_translation(teaser_hip_solver* h, const double* src,
                                         const double* dst, int32_t k, double* translation,
                                         uint8_t* inlier_mask);
TEASER_HIP_API int32_t teaser_hip_scalar_tls(teaser_hip_solver* h, const double* x, const double* ranges,
                              int32_t n, double* estimate, uint8_t* inlier_mask);
/*   solveForScale      -> the scale solver the Params select (registration.h:584, :847-853):
 *                         TLSScaleSolver::solveForScale (registration.cc:410-425) when estimate_scaling,
 *                         else ScaleInliersSelector::solveForScale (registration.cc:427-443, scale = 1),
 *                         on caller-supplied TIMs v1, v2 (3 x m column-major). */
TEASER_HIP_API int32_t teaser_hip_solve_for_scale(teaser_hip_solver* h, const double* v1, const double* v2,
                                   int64_t m, double* scale, uint8_t* inlier_mask);

/* Correspondence front-end (the stage BEFORE solve()).
 *   compute_fpfh   -> teaser::FPFHEstimation::computeFPFHFeatures (teaser/src/fpfh.cc:15-43,
 *                     teaser/include/teaser/fpfh.h:40-42): PCL-semantics normals (radius search, viewpoint
 *                     0,0,0) and 33-bin FPFH descriptors.  cloud_xyz: n x 3 floats (teaser::PointXYZ);
 *                     fpfh_out: n x 33 floats (pcl::FPFHSignature33::histogram); normals_out: n x 3 or NULL
 *                     (FPFHEstimation::getNormals, fpfh.h:56).
 *   match_features -> teaser::Matcher::calculateCorrespondences (teaser/src/matcher.cc:21-301,
 *                     matcher.h:40-44) for use_tuple_test = false: exact L2 nearest neighbours both ways,
 *                     optional cross check, sorted unique (src, dst) pairs.  pairs: room for *n_pairs
 *                     pairs on entry (n_src + n_dst always suffices), count on return.
 *   tuple_test     -> the tuple constraint of the same function (matcher.cc:223-283, use_tuple_test = true with
 *                     tuple_scale != 0), applied to the pairs match_features returned: 100 x n_pairs random
 *                     triples of correspondences, a triple is kept when its three side lengths in the source
 *                     cloud and in the target cloud agree within the factor tuple_scale (l_i s < l_j < l_i / s);
 *                     the correspondences of the kept triples, sorted and unique, replace the list (host
 *                     arithmetic in float like the reference; no device needed, `h` may be NULL).  The reference
 *                     draws from rand() seeded with time(NULL), i.e. its result is not reproducible; here
 *                     seed = 0 means "seed from the clock" (the reference's behaviour), any other value gives a
 *                     reproducible draw (splitmix64).  The reference's normalizePoints (matcher.cc:57-116) moves
 *                     and scales both clouds alike, which the ratio test cannot see: not needed.
 *                     tuple_scale <= 0: nothing to do (the reference skips the test for tuple_scale == 0). */
TEASER_HIP_API int32_t teaser_hip_compute_fpfh(teaser_hip_solver* h, const float* cloud_xyz, int32_t n,
                                double normal_radius, double fpfh_radius, float* fpfh_out,
                                float* normals_out);
TEASER_HIP_API int32_t teaser_hip_match_features(teaser_hip_solver* h, const float* src_feat, int32_t n_src,
                                  const float* dst_feat, int32_t n_dst, int32_t dim, int32_t use_crosscheck,
                                  int32_t* pairs, int64_t* n_pairs);
TEASER_HIP_API int32_t teaser_hip_tuple_test(teaser_hip_solver* h, const float* src_xyz, int32_t n_src,
                              const float* dst_xyz, int32_t n_dst, float tuple_scale, uint64_t seed,
                              int32_t* pairs /* in / out */, int64_t* n_pairs /* in / out */);
/*   tuple_test_batch -> the same constraint for a BATCH of problems on the GPU (teaser_hip_features_tuple_test_batch,
 *                     declared with the batched front-end below).  teaser_hip_tuple_test stays the host form and the
 *                     specification: for every problem and every non-zero seed the batched call returns exactly
 *                     what it returns.  The contract, per problem, with ncorr = n_pairs input pairs (src, dst), the
 *                     float clouds, float s = tuple_scale and the uint64 seed; all counters are 64-bit:
 *                       for i = 0 .. 100 ncorr - 1 and k = 0, 1, 2:
 *                         z = seed + (3 i + k + 1) 0x9E3779B97F4A7C15            (wrapping: splitmix64's state after
 *                         z = (z ^ z >> 30) 0xBF58476D1CE4E5B9                    3 i + k + 1 draws, so a trial is a
 *                         z = (z ^ z >> 27) 0x94D049BB133111EB;  z ^= z >> 31     function of (seed, i) alone)
 *                         r_k = z mod ncorr                                       (the exact 64-bit remainder)
 *                       with (i_k, j_k) = input pair r_k, in float, every operation rounded and nothing fused:
 *                         |a - b| = sqrt(dx dx + dy dy + dz dz), summed in that order, sqrt correctly rounded
 *                         li0 = |p_i0 - p_i1|, li1 = |p_i1 - p_i2|, li2 = |p_i2 - p_i0| in the source cloud,
 *                         lj0, lj1, lj2 likewise in the target cloud
 *                       trial i passes when li s < lj and lj < li / s (a correctly rounded division) for all three
 *                       sides.  Result: the input pairs that occur in at least one passing trial, sorted by
 *                       (src, dst), unique.
 *                     Edge cases as the host function: a problem with !(tuple_scale > 0) or ncorr = 0 is returned
 *                     untouched (neither sorted nor made unique); input pairs may be unsorted and may repeat, and
 *                     repeats count towards ncorr; an index outside its cloud is TEASER_HIP_ERR_BAD_ARG naming the
 *                     problem, found on the host before anything is launched or written; seed = 0 means "from the
 *                     clock": the call reads time(NULL) once and uses that value for every problem whose seed is 0. */

/* DRS rotation certifier: teaser::DRSCertifier::certify(R, src, dst, theta) (teaser/src/certification.cc:39-190,
 * teaser/include/teaser/certification.h:53-239).  Parameters as DRSCertifier::Params (certification.h:71-104;
 * eig_decomposition_solver: the dense solver is always used -- Spectra is an un-vendored dependency).
 * R: 3 x 3 row-major; src / dst: the 3 x N column-major matrices of the reference (N points, xyz interleaved);
 * theta: N entries, +1 inlier / -1 outlier (certification.h:133-140).  traj: capacity traj_cap doubles
 * (max_iterations always suffices) or NULL; out->iterations = length of the sub-optimality trajectory.
 * TEASER_HIP_ERR_UNSUPPORTED when rocSOLVER / rocBLAS (the symmetric eigensolver) cannot be loaded. */
typedef struct teaser_certifier_params_c {
  double noise_bound;     /* 0.01 */
  double cbar2;           /* 1 */
  double sub_optimality;  /* 1e-3 */
  double max_iterations;  /* 2e2 (a double in the reference, too) */
  double gamma_tau;       /* 1.999999 */
} teaser_certifier_params_c;
typedef struct teaser_certification_c {
  int32_t is_optimal;          /* CertificationResult::is_optimal */
  int32_t iterations;          /* suboptimality_traj.size() */
  double best_suboptimality;   /* CertificationResult::best_suboptimality */
} teaser_certification_c;
TEASER_HIP_API int32_t teaser_hip_certifier_params_default(teaser_certifier_params_c* p);
/* The certifier's cold start: the first rocBLAS handle and rocSOLVER call of a process load those libraries'
 * gfx950 code objects (about 110 s on ROCm 7.2, host-side).  certifier_warmup starts ONE background thread per
 * process that does this (and a small eigendecomposition + GEMM) and returns at once; teaser_hip_certify joins it.
 * Call it when the application starts (or right after creating the solver) to take the load off the first
 * certify().  device < 0: the current device. */
TEASER_HIP_API int32_t teaser_hip_certifier_warmup(int32_t device);
TEASER_HIP_API int32_t teaser_hip_certify(teaser_hip_solver* h, const teaser_certifier_params_c* p, const double* R,
                           const double* src, const double* dst, const double* theta, int32_t n,
                           teaser_certification_c* out, double* traj, int32_t traj_cap);
/* The certifier's projection onto the affine dual subspace alone: DRSCertifier::getOptimalDualProjection
 * (certification.cc:323-452), by the kernel launches the loop of teaser_hip_certify itself makes.  W, W_dual: (4n + 4)^2
 * doubles, column-major (host); theta: n entries, each +1 or -1; 1 <= n <= 8000.  Uses neither rocSOLVER nor rocBLAS and
 * does not wait for their warm-up. */
TEASER_HIP_API int32_t teaser_hip_certify_dual_projection(teaser_hip_solver* h, const double* W, const double* theta,
                                                          int32_t n, double* W_dual);
/* teaser_hip_certify, which also copies out the matrices of the 0-based `iteration` of its loop, from the buffers the loop
 * works on: stages = 6 (4n + 4)^2 doubles (host), column-major, in this order: M entering the iteration, M_psd, W, W_dual,
 * M_affine, M leaving it (= M entering where the loop stopped at that iteration).  The run is the one teaser_hip_certify
 * makes: same launches, same trajectory.  TEASER_HIP_ERR_BAD_ARG (the message names `iteration`) when the run ends before
 * that iteration; out / traj are filled as by teaser_hip_certify then, too. */
TEASER_HIP_API int32_t teaser_hip_certify_stages(teaser_hip_solver* h, const teaser_certifier_params_c* p, const double* R,
                                                 const double* src, const double* dst, const double* theta, int32_t n,
                                                 int32_t iteration, double* stages, double* traj, int32_t traj_cap,
                                                 teaser_certification_c* out);

/* MaxCliqueSolver::findMaxClique (graph.cc:12-125) on a caller-supplied adjacency bitmap
 * (host pointer, n rows of (n+63)/64 words).  clique: capacity n; sorted on return. */
TEASER_HIP_API int32_t teaser_hip_max_clique(teaser_hip_solver* h, const uint64_t* bitmap, int32_t n,
                              int32_t* clique, int32_t* clique_size, int32_t* exact_run);

/* Profiling / diagnostics. */
TEASER_HIP_API int32_t teaser_hip_set_profiling(teaser_hip_solver* h, int32_t level /* 0, 1, 2 */);
/* Route switches among EQUIVALENT paths and tuning knobs of the implementation (no counterpart in the reference;
 * process-wide, `h` may be NULL).  No value of a route option changes a result: the GPU suite compares the routes
 * with each other and with the oracle (tests/test_gpu_route_switches.py).  Names (defaults; ranges and meanings in
 * INTEGRATION.md's settings table): "k1_fp64" (0; 1 = the all-FP64 K1 instead of the matrix-core filter),
 * "fused_estimators" (1), "scale_sort64" (0), "scale_batch" (1), "scale_mid_batch" (1), "spec_bounds" (1),
 * "finisher" (1), "copy_stream" (0), "h2d_kernel" (0), "depth" (2; lanes of handles created afterwards), "stagger"
 * (1), "k1_stream" (0), "tail_cus" (0), "tail_cu_block" (0), "k4_lds_stack" (16384), "k4_donate" (1),
 * "k4_donate_after" / "k4_hungry" / "k4_expand" (-1 = built-in), "heu_blocks" (0 = built-in), "greedy_threads"
 * (0 = built-in), "fixup_wgs" (0 = built-in), "k4_waves" (0 = built-in: 4096), "deg_closure" (1), "greedy_small"
 * (1), "deg_closure_wgs" (0 = built-in), "scale_hull" (60), "scale_hull_sync" (1), "colour_persistent" (0),
 * "heu_skip_closed" (0), "colour_mis" (8192), "colour_mis_any" (0).
 * DIAGNOSTIC options, which may change results: "k4_debug" (0; stderr diagnostics), "k4_lb_bonus" (0; the exact
 * search starts above the incumbent), "tail_skip" (0; timing probes: stages left out, results wrong by design),
 * "reference_snapshot_semantics" (0; handles created or reset afterwards behave like the reference snapshot's
 * binary).  Each option also has an environment variable that is read ONCE per process; the
 * library never calls getenv on a solve path and never modifies the environment.
 * Returns BAD_ARG for an unknown name or a value outside the option's range. */
TEASER_HIP_API int32_t teaser_hip_set_option(teaser_hip_solver* h, const char* name, int64_t value);
/* The current value of a teaser_hip_set_option name (its default, the environment's value, or the last value set),
 * so a caller can restore it.  Returns BAD_ARG for an unknown name or a NULL pointer. */
TEASER_HIP_API int32_t teaser_hip_get_option(const char* name, int64_t* value);
TEASER_HIP_API int32_t teaser_hip_get_profile(const teaser_hip_solver* h, teaser_profile_c* out);
/* The HIP stream (hipStream_t) all kernels of this handle are launched on. */
TEASER_HIP_API void* teaser_hip_get_stream(teaser_hip_solver* h);
TEASER_HIP_API const char* teaser_hip_last_error(const teaser_hip_solver* h);
TEASER_HIP_API int32_t teaser_hip_abi_version(void);
TEASER_HIP_API int32_t teaser_hip_device_count(void);

/* ICP refinement (the reference's 3DMatch tutorial, examples/teaser_python_fpfh_icp/example.py:66-71, refines the
 * TEASER++ pose with Open3D's registration_icp + TransformationEstimationPointToPoint(with_scaling=False)): batched
 * point-to-point ICP with Open3D's semantics, on its OWN handle (nothing is shared with teaser_hip_solver).
 * Per problem: source P (n_s points) and target Q (n_t points), xyz interleaved doubles (the layout of solve()'s
 * 3 x N column-major input); r = max_correspondence_distance; init 4 x 4 row-major, last row 0 0 0 1.
 *   apply(T, p)_row = ((T[row][0] x + T[row][1] y) + T[row][2] z) + T[row][3]      (no fused operations)
 *   corr(X): for each source point i, the lexicographic minimum of (d2, j) over the target points j with
 *            d2 = ((dx dx + dy dy) + dz dz) < r r, dx = X.x - Q.x: ties go to the smaller target index, a point at
 *            exactly r is not a match.  fitness = |C| / n_s, inlier_rmse = sqrt(sum d2 / |C|), both 0 when C = {}.
 *   loop:    X = apply(init, P), T = init, res = corr(X); for it = 1 .. max_iteration:
 *            U = umeyama(X[C.src], Q[C.dst]) (identity when C is empty), T = U T, X = apply(U, X), prev = res,
 *            res = corr(X), stop when |prev.fitness - res.fitness| < relative_fitness AND
 *            |prev.inlier_rmse - res.inlier_rmse| < relative_rmse -- ABSOLUTE differences, despite Open3D's names.
 *   umeyama: R = V diag(1,1,s) U^T from the SVD U S V^T of H = sum (p - mu_P)(q - mu_Q)^T, s = -1 iff
 *            det(U) det(V) < 0, t = mu_Q - R mu_P (no scaling).  The sums are centred on a fixed point of each
 *            problem (its target's bounding-box centre), so clouds far from the origin keep their precision.
 *            Where the best fit is not unique -- a cross-covariance H of rank <= 1 (one correspondence, collinear
 *            matches, every source matched to one target point) -- U is a maximiser of tr(R H) among the proper
 *            rotations (R^T R = I, det R = +1, R H symmetric, t = mu_Q - R mu_P), not a specified one; H = 0 gives
 *            R = the identity exactly.  Rank 2 (coplanar matches) and det(H) < 0 with s1 > s2 have a unique answer.
 * Output: T, fitness and inlier_rmse of the final res, iterations = loop bodies executed (max_iteration = 0
 * returns init and corr(apply(init, P))), and the correspondence set sorted by source index.  n_s = 0 or n_t = 0
 * is valid (no correspondences, fitness 0, rmse 0).  TEASER_HIP_ERR_BAD_ARG (teaser_hip_icp_last_error names the
 * argument) for a non-finite or non-positive r, a negative max_iteration, negative or non-finite criteria, a
 * non-finite init or one whose last row is not 0 0 0 1, non-finite points, a NULL pointer where n > 0.
 * Results are deterministic: the same bits run to run, and for a problem alone or inside any batch.  An ICP handle is
 * not re-entrant (one call at a time; distinct handles are independent), like a solver handle. */
typedef struct teaser_icp_params_c {
  double max_correspondence_distance; /* r; no default (Open3D's argument is required) */
  int32_t max_iteration;              /* 30 */
  double relative_fitness;            /* 1e-6 */
  double relative_rmse;               /* 1e-6 */
} teaser_icp_params_c;
typedef struct teaser_icp_result_c {
  double transformation[16]; /* row-major 4 x 4 */
  double fitness;
  double inlier_rmse;
  int32_t iterations;
  int32_t n_correspondences;
} teaser_icp_result_c;
typedef struct teaser_hip_icp teaser_hip_icp;
/* Open3D's ICPConvergenceCriteria defaults; max_correspondence_distance is set to 0 (invalid until given). */
TEASER_HIP_API int32_t teaser_hip_icp_params_default(teaser_icp_params_c* params);
/* device < 0: the current device.  TEASER_HIP_ERR_NO_DEVICE without a GPU: there is no CPU path. */
TEASER_HIP_API int32_t teaser_hip_icp_create(int32_t device, teaser_hip_icp** out);
TEASER_HIP_API int32_t teaser_hip_icp_destroy(teaser_hip_icp* icp);
TEASER_HIP_API const char* teaser_hip_icp_last_error(const teaser_hip_icp* icp);
/* DIAGNOSTIC, on no hot path; it never changes a result.  Every handle but the solver's keeps grow-only scratch
 * buffers between its calls, and a call may assume nothing about what they hold.  teaser_hip_<kind>_fill_scratch
 * (icp, voxel, features, posegraph, ransac, fgr, plane, tsdf) sets every byte of every device scratch buffer and of
 * every page-locked staging buffer of the handle, up to the buffer's CAPACITY (not the last call's size), to `byte`
 * (0 .. 255, anything else is TEASER_HIP_ERR_BAD_ARG), on the handle's stream, and synchronises; the ICP handle's
 * pageable staging is filled up to its current size.  *bytes_out = the device bytes filled: 0 for a handle that has
 * served no call, and unchanged by a call that grew no buffer.  It allocates nothing, frees nothing and leaves what is
 * state alone: options, the fallback count of the last call, the TSDF volume, the stream.  A test that calls it
 * between two calls and still finds the second equal to its restatement has shown that the second read nothing the
 * first one left (tests/test_gpu_scratch_independence.py). */
TEASER_HIP_API int32_t teaser_hip_icp_fill_scratch(teaser_hip_icp* icp, int32_t byte, int64_t* bytes_out);
/* `batch` independent problems, HOST pointers per problem, borrowed for the call.  init: batch x 16 row-major
 * or NULL (identity for every problem); params: one per problem; out: [batch]; corr: NULL, or per problem NULL or
 * room for n_src[b] x 2 int32 (source index, target index), ascending source index, out[b].n_correspondences
 * pairs written.  Problems of mixed sizes share the launches. */
TEASER_HIP_API int32_t teaser_hip_icp_batch(teaser_hip_icp* icp, int32_t batch, const double* const* src,
                                            const int32_t* n_src, const double* const* dst, const int32_t* n_dst,
                                            const double* init, const teaser_icp_params_c* params,
                                            teaser_icp_result_c* out, int32_t* const* corr);
/* One problem: teaser_hip_icp_batch with batch = 1.  init may be NULL (identity); corr NULL or room for n_src x 2. */
TEASER_HIP_API int32_t teaser_hip_icp_solve(teaser_hip_icp* icp, const double* src, int32_t n_src,
                                            const double* dst, int32_t n_dst, const double* init,
                                            const teaser_icp_params_c* params, teaser_icp_result_c* out,
                                            int32_t* corr);

/* ICP refinement: point-to-plane (Open3D's TransformationEstimationPointToPlane with an optional RobustKernel), a
 * second estimation method of the same batched ICP: same handle, search, stop rule and determinism guarantees,
 * selectable per problem and mixed freely with point-to-point problems in one batch.
 * Additional input per point-to-plane problem: the target normals N, n_t x 3 doubles, one per target point, used as
 * given (not normalised, like Open3D).  A zero normal is legal and contributes nothing to the step.
 * The loop, apply, corr, fitness, inlier_rmse (EUCLIDEAN, as above: Open3D's registration_icp reports that one for
 * every estimation method), T = U T, the iteration count and the stop rule are exactly those written out above.
 * Only U differs.  With c = the problem's target bounding-box centre and, for every correspondence (i, j) of C in
 * ascending i, x = the current moved source point, q = Q[j], n = N[j]:
 *   x' = x - c,  q' = q - c,  e = x' - q'
 *   r  = (e0 n0 + e1 n1) + e2 n2                        residual, no fused operations
 *   w  = kernel(r)                                      weight, table below
 *   J  = [ x' x n ; n ]                                 6-vector (cross product, then the normal)
 *   A  = sum w J J^T  (6 x 6, symmetric),  g = sum w r J
 *   solve A xi = -g in FP64 by LDL^T without pivoting;  xi = (alpha, beta, gamma, t'x, t'y, t'z)
 *   R  = Rz(gamma) Ry(beta) Rx(alpha)                   Open3D's TransformVector6dToMatrix4d
 *   U  = [ R | t' + c - R c ]                           the step expressed in the problem's own coordinates
 * U is the identity when C is empty, when the factorisation meets a pivot that is not finite or not positive, or when
 * xi is not finite (Open3D returns the identity when its solve fails).  An exactly singular system gives the identity:
 * parallel normals on a planar target, all normals zero, a single correspondence, every pair of a Generalized-ICP
 * problem left out -- whenever the FP64 factorisation of the FP64 sums meets a pivot that is exactly zero or negative.
 * When a pivot is zero only up to rounding (A singular in exact arithmetic, its FP64 pivot a few ulps either side of
 * 0), either outcome -- the identity or the step the tiny pivot gives -- is conforming, and it is always a rigid
 * transform: finite, R a proper rotation, last row 0 0 0 1.  Solving in the frame centred on c is the ONE
 * deliberate difference from Open3D, which linearises about the origin: the two steps differ at second order in the
 * step's rotation and have the same fixed point, and the centred form makes the result independent of where the pair
 * sits in space (up to the coordinates' own rounding), as the point-to-point sums already are.
 * Robust kernels, Open3D's RobustKernel::Weight(r) with its parameter k:
 *   L2 (default)  1
 *   Huber         1 if |r| <= k, else k / |r|
 *   Cauchy        1 / (1 + (r / k)^2)
 *   GM            k / (k + r^2)^2
 *   Tukey         (1 - (r / k)^2)^2 if |r| <= k, else 0
 * Open3D's L1Loss (w = 1 / |r|, unbounded at r = 0) is not offered.  Open3D applies no kernel to point-to-point;
 * neither does this.  TEASER_HIP_ERR_BAD_ARG (argument named) in addition to the list above: an unknown method or
 * kernel, a kernel other than L2 with point-to-point, a kernel_k that is not finite and > 0 (ignored for L2),
 * point-to-plane with n_t > 0 and no dst_normals, non-finite dst_normals.  Point-to-point problems give the same bits
 * through the _ex entry points as through the ones above, alone or mixed with point-to-plane problems. */
typedef struct teaser_icp_estimation_c {
  int32_t method;  /* 0 point-to-point (default), 1 point-to-plane, 2 Generalized ICP (_cov entry points and later),
                      3 Colored ICP (_color entry points only) */
  int32_t kernel;  /* 0 L2 (default), 1 Huber, 2 Cauchy, 3 GM, 4 Tukey */
  double kernel_k; /* 1.0 (Open3D's default); ignored for L2 */
} teaser_icp_estimation_c;
TEASER_HIP_API int32_t teaser_hip_icp_estimation_default(teaser_icp_estimation_c* est);
/* teaser_hip_icp_batch plus dst_normals (NULL, or per problem NULL for point-to-point, else n_dst[b] x 3 doubles,
 * borrowed for the call) and est (NULL = every problem point-to-point, else one per problem). */
TEASER_HIP_API int32_t teaser_hip_icp_batch_ex(teaser_hip_icp* icp, int32_t batch, const double* const* src,
                                               const int32_t* n_src, const double* const* dst,
                                               const int32_t* n_dst, const double* init,
                                               const teaser_icp_params_c* params, teaser_icp_result_c* out,
                                               int32_t* const* corr, const double* const* dst_normals,
                                               const teaser_icp_estimation_c* est);
/* One problem: teaser_hip_icp_batch_ex with batch = 1. */
TEASER_HIP_API int32_t teaser_hip_icp_solve_ex(teaser_hip_icp* icp, const double* src, int32_t n_src,
                                               const double* dst, int32_t n_dst, const double* init,
                                               const teaser_icp_params_c* params, teaser_icp_result_c* out,
                                               int32_t* corr, const double* dst_normals,
                                               const teaser_icp_estimation_c* est);

/* ICP refinement: Generalized ICP (plane-to-plane; Segal, Haehnel, Thrun, "Generalized-ICP", RSS 2009; the formulation
 * of Open3D's registration_generalized_icp / TransformationEstimationForGeneralizedICP), a third estimation method
 * (method = 2) of the same batched ICP: same handle, search, stop rule and determinism guarantees, selectable per
 * problem and mixed freely with methods 0 and 1 in one batch.
 * The loop, apply, corr (the lexicographic minimum of (d2, j), strict d2 < r r), fitness, the EUCLIDEAN inlier_rmse,
 * T = U T, the iteration count, the stop rule on absolute differences, max_iteration = 0, empty clouds and the corr
 * output are exactly those written out above.  Only U differs.
 * Additional input per Generalized-ICP problem: source covariances Cs (n_s x 9 doubles) and target covariances Ct
 * (n_t x 9), one row-major 3 x 3 per point.  ONLY THE UPPER TRIANGLE (entries 0, 1, 2, 4, 5, 8) IS READ; the matrix is
 * taken as symmetric.  With c = the problem's target bounding-box centre, Rk = the rotation block of the accumulated T
 * that the current moved points X correspond to (init for the first step, then U T), and for every correspondence
 * (i, j) of C in ascending i, x = X[i], q = Q[j]:
 *   x' = x - c,  q' = q - c,  e = x' - q'
 *   B  = Rk Cs[i]                B[r][c] = (Rk[r][0] Cs[0][c] + Rk[r][1] Cs[1][c]) + Rk[r][2] Cs[2][c]
 *   M  = Ct[j] + B Rk^T          M[r][c] = Ct[r][c] + ((B[r][0] Rk[c][0] + B[r][1] Rk[c][1]) + B[r][2] Rk[c][2]), c >= r
 *                                (symmetric 3 x 3, FP64, no fused operations)
 *   adj: a00 = M11 M22 - M12 M12,  a01 = M02 M12 - M01 M22,  a02 = M01 M12 - M02 M11,
 *        a11 = M00 M22 - M02 M02,  a12 = M01 M02 - M00 M12,  a22 = M00 M11 - M01 M01
 *   det = (M00 a00 + M01 a01) + M02 a02,   W = adj / det (each entry one division)
 *        The correspondence contributes NOTHING to A and g when det is not finite or not > 0.  It still counts for
 *        fitness and inlier_rmse.
 *   J  = [ -[x']x | I3 ]                                3 x 6: e(xi) ~ e + J xi, xi = (alpha, beta, gamma, t'x, t'y, t'z)
 *   A  = sum J^T W J  (6 x 6, symmetric),  g = sum J^T W e
 *        with G = [x']x W (column k of G = x' x column k of W):  A = [ rows (x' x row r of G) | G ; . | W ],
 *        W e = per row (W[r][0] e0 + W[r][1] e1) + W[r][2] e2,  g = [ x' x (W e) ; W e ]
 *   solve A xi = -g by the LDL^T of point-to-plane;  R = Rz(gamma) Ry(beta) Rx(alpha);  U = [ R | t' + c - R c ]
 * U is the identity in the cases point-to-plane names: C empty, a pivot that is not finite or not positive (which
 * includes every correspondence having been left out), xi not finite.  With W = n n^T this is the point-to-plane step
 * (J^T n = [x' x n ; n]).
 * Robust kernels: L2 ONLY.  Open3D weights each row of the whitened residual M^(-1/2) e, which needs a 3 x 3 matrix
 * square root per correspondence and iteration; a different weighting under the same names would mislead, so a
 * Generalized-ICP problem with kernel != 0 is refused (TEASER_HIP_ERR_BAD_ARG, "kernel" in the message).
 * Differences from Open3D (this states the FORMULATION; bit parity with Open3D is not claimed and was not measured):
 *   - the step is linearised in the frame centred on c, as for point-to-plane;
 *   - Rk Cs Rk^T is formed each iteration from the caller's Cs and the accumulated T, not by transforming stored
 *     covariances step after step;
 *   - L2 only.
 * Methods 0, 1 and 2 go through the _cov entry points below; the older entry points keep refusing method 2 ("method").
 * Point-to-point and point-to-plane problems give the same bits through the _cov entry points as through their own,
 * alone or mixed.  TEASER_HIP_ERR_BAD_ARG (argument and problem named) in addition to the lists above: method 2 with
 * n_src > 0 and no src_cov or n_dst > 0 and no dst_cov, a non-finite entry among the six read of any covariance,
 * kernel != 0 with method 2.
 * src_cov / dst_cov: NULL, or per problem NULL (methods 0 and 1) or n x 9 doubles, borrowed for the call. */
TEASER_HIP_API int32_t teaser_hip_icp_batch_cov(teaser_hip_icp* icp, int32_t batch, const double* const* src,
                                                const int32_t* n_src, const double* const* dst,
                                                const int32_t* n_dst, const double* init,
                                                const teaser_icp_params_c* params, teaser_icp_result_c* out,
                                                int32_t* const* corr, const double* const* dst_normals,
                                                const teaser_icp_estimation_c* est, const double* const* src_cov,
                                                const double* const* dst_cov);
/* One problem: teaser_hip_icp_batch_cov with batch = 1. */
TEASER_HIP_API int32_t teaser_hip_icp_solve_cov(teaser_hip_icp* icp, const double* src, int32_t n_src,
                                                const double* dst, int32_t n_dst, const double* init,
                                                const teaser_icp_params_c* params, teaser_icp_result_c* out,
                                                int32_t* corr, const double* dst_normals,
                                                const teaser_icp_estimation_c* est, const double* src_cov,
                                                const double* dst_cov);
/* Covariance estimation for Generalized ICP, on the ICP handle: a batch of clouds (n x 3 doubles each) with a radius, a
 * max_nn in [3, TEASER_HIP_ICP_COV_MAX_NN] and an epsilon (NULL = 1e-3 for every cloud) per cloud.  Per point i:
 *   neighbourhood: the points j (i itself included) with d2 = ((dx dx + dy dy) + dz dz) < radius radius,
 *                  dx = P[i].x - P[j].x (the expression of corr); when there are more than max_nn, the max_nn smallest
 *                  by (d2, j).  m = their number.
 *   m < 3:         C = the identity.
 *   otherwise:     o = P[j] - P[i];  S1 = sum o,  S2 = sum o o^T (upper triangle), both added one neighbour at a time in
 *                  ascending (d2, j) from 0, so the bits depend on neither bucket order, batch nor run;
 *                  cov[a][b] = (S2[a][b] - (S1[a] S1[b]) / m) / (m - 1)
 *                  cyclic Jacobi in FP64 on cov with V = I: at most 16 sweeps over the pairs (0,1), (0,2), (1,2); a pair
 *                  is skipped when a_pq = 0 or |a_pq| <= 1e-17 (|a_pp| + |a_qq|), a sweep that rotates nothing ends
 *                  the iteration; theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(1 + theta^2))
 *                  (sign(0) = +1), cs = 1 / sqrt(1 + t^2), sn = t cs; a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0,
 *                  (a_op, a_oq) = (cs a_op - sn a_oq, sn a_op + cs a_oq) for the third index o, and the columns p, q
 *                  of V likewise
 *                  n^ = the column of V of the smallest diagonal entry (the first on a tie), divided by its length
 *                  C = I - ((1 - epsilon) n^) n^^T, that is V diag(epsilon, 1, 1) V^T; the sign of n^ cannot matter.
 * out[b]: n[b] x 9 doubles, row-major symmetric 3 x 3 per point.  TEASER_HIP_ERR_BAD_ARG (argument and cloud named):
 * non-finite points, a radius (or its square) or epsilon that is not finite and > 0, max_nn outside its range, NULL
 * where n > 0.  Deterministic like every call on this handle.  Performance only: a call whose largest max_nn exceeds
 * 32 runs every cloud of the call through the kernel with the longer neighbour list (lower occupancy). */
#define TEASER_HIP_ICP_COV_MAX_NN 100
TEASER_HIP_API int32_t teaser_hip_icp_covariances_batch(teaser_hip_icp* icp, int32_t batch,
                                                        const double* const* points, const int32_t* n,
                                                        const double* radius, const int32_t* max_nn,
                                                        const double* epsilon, double* const* out);

/* Normal estimation (Open3D's estimate_normals with KDTreeSearchParamHybrid or KDTreeSearchParamKNN, plus
 * estimate_covariances and the two orient_normals_* calls), on the ICP handle: a batch of clouds (n x 3 doubles each)
 * with one search record per cloud.  Per point i:
 *   neighbourhood, search 0 (hybrid): exactly the covariance contract's above -- d2 < radius radius, i itself
 *                  included, the max_nn smallest by (d2, j).  m = their number.
 *   neighbourhood, search 1 (k-NN):   the m = min(max_nn, n) first of self k-NN's order (d2, j) below; no radius.
 *   m >= 3:        S1, S2, cov and the cyclic Jacobi are those of the covariance contract above, word for word.
 *                  cov_out = that cov (the RAW sample covariance before the Jacobi), the full symmetric matrix, the
 *                            lower triangle mirrored;
 *                  eig_out = the three diagonal entries after the Jacobi, ascending;
 *                  n^      = the column of V of the smallest diagonal entry (the first on a tie), divided by its length.
 *   m < 3:         n^ = 0, cov_out = the zero matrix, eig_out = 0 (hybrid search, or k-NN search on a cloud with n < 3);
 *                  the orientation step then fills the normal in.
 *   orientation, applied last; it changes only the sign, or fills a zero normal:
 *     orient 0:    the sign the Jacobi leaves: deterministic, without meaning.  A zero normal becomes (0, 0, 1).
 *     orient 1:    n^ is negated when (n^x (ref - p)x + n^y (ref - p)y) + n^z (ref - p)z < 0.  A zero normal becomes
 *                  (ref - p) / |ref - p|, |v| = sqrt((vx vx + vy vy) + vz vz), or (0, 0, 1) when that length is 0.
 *     orient 2:    n^ is negated when (n^x refx + n^y refy) + n^z refz < 0.  A zero normal becomes ref as given.
 *                  (The rules of Open3D's orient_normals_towards_camera_location and
 *                  orient_normals_to_align_with_direction; bit parity with Open3D is not claimed.)
 * Radius-only search (Open3D's KDTreeSearchParamRadius: no cap on the neighbours) is NOT offered: the sums are ordered
 * sums over a bounded sorted list, and without a cap there is no such list.  (ISS keypoints below sum an uncapped
 * radius neighbourhood in another, stated order.)
 * normals_out[b]: n[b] x 3 doubles.  cov_out: NULL, or per cloud NULL or n x 9 doubles.  eig_out: NULL, or per cloud NULL
 * or n x 3 doubles.  Empty clouds are legal.  Deterministic like every call on this handle: the same bits alone, inside
 * any batch, run after run; for k-NN search independent of "knn_ring_cap", and "knn_fallbacks" is updated (a call
 * without a k-NN cloud sets it to 0).  TEASER_HIP_ERR_BAD_ARG (argument and cloud named): non-finite points, search or
 * orient outside their ranges, reserved != 0, max_nn outside [3, TEASER_HIP_ICP_COV_MAX_NN], a radius (or its square)
 * that is not finite and > 0 in hybrid search, a non-finite ref when orient != 0, NULL where n > 0. */
typedef struct teaser_icp_normal_search_c {
  int32_t search;   /* 0 hybrid: the max_nn nearest inside radius; 1 knn: the max_nn nearest, no radius */
  int32_t max_nn;   /* [3, TEASER_HIP_ICP_COV_MAX_NN] */
  double radius;    /* search 0: finite, > 0, square finite; search 1: ignored */
  int32_t orient;   /* 0 none, 1 towards the point ref, 2 along the direction ref */
  int32_t reserved; /* 0 */
  double ref[3];
} teaser_icp_normal_search_c;
#ifdef __cplusplus
static_assert(sizeof(teaser_icp_normal_search_c) == 48, "teaser_icp_normal_search_c is 48 bytes");
#else
_Static_assert(sizeof(teaser_icp_normal_search_c) == 48, "teaser_icp_normal_search_c is 48 bytes");
#endif
TEASER_HIP_API int32_t teaser_hip_icp_normals_batch(teaser_hip_icp* icp, int32_t batch, const double* const* points,
                                                    const int32_t* n, const teaser_icp_normal_search_c* search,
                                                    double* const* normals_out, double* const* cov_out,
                                                    double* const* eig_out);
/* teaser_hip_icp_batch_cov with self-estimated target normals.  dst_normal_search: NULL, or one record per problem; a
 * record with max_nn = 0 means "none given" (its other fields are not read).  A point-to-plane problem whose
 * dst_normals[b] is NULL (or dst_normals NULL) and whose record has max_nn != 0 gets its target normals from the rule
 * above applied to dst[b], on the device: the normals kernel writes them into the buffer the correspondence pass
 * gathers from; they are neither copied to the host nor uploaded.  The result is, bit for bit, that of
 * teaser_hip_icp_normals_batch followed by teaser_hip_icp_batch_cov with those normals.  Records of problems that give
 * dst_normals, or are not point-to-plane, are not read.  Every other problem gives the bits it gives through
 * teaser_hip_icp_batch_cov; a point-to-plane problem with neither normals nor a record is refused as there
 * ("dst_normals").  A record that is read is checked as above (the argument is named dst_normal_search). */
TEASER_HIP_API int32_t teaser_hip_icp_batch_auto(teaser_hip_icp* icp, int32_t batch, const double* const* src,
                                                 const int32_t* n_src, const double* const* dst,
                                                 const int32_t* n_dst, const double* init,
                                                 const teaser_icp_params_c* params, teaser_icp_result_c* out,
                                                 int32_t* const* corr, const double* const* dst_normals,
                                                 const teaser_icp_estimation_c* est, const double* const* src_cov,
                                                 const double* const* dst_cov,
                                                 const teaser_icp_normal_search_c* dst_normal_search);
/* One problem: teaser_hip_icp_batch_auto with batch = 1. */
TEASER_HIP_API int32_t teaser_hip_icp_solve_auto(teaser_hip_icp* icp, const double* src, int32_t n_src,
                                                 const double* dst, int32_t n_dst, const double* init,
                                                 const teaser_icp_params_c* params, teaser_icp_result_c* out,
                                                 int32_t* corr, const double* dst_normals,
                                                 const teaser_icp_estimation_c* est, const double* src_cov,
                                                 const double* dst_cov,
                                                 const teaser_icp_normal_search_c* dst_normal_search);

/* ICP refinement: Colored ICP (Park, Zhou, Koltun, "Colored Point Cloud Registration Revisited", ICCV 2017; the
 * formulation of Open3D's registration_colored_icp / TransformationEstimationForColoredICP), a fourth estimation method
 * (method = 3) of the same batched ICP: same handle, search, stop rule and determinism guarantees, selectable per
 * problem and mixed freely with methods 0, 1 and 2 in one batch.
 * The loop, apply, corr (the lexicographic minimum of (d2, j), strict d2 < r r), fitness, the EUCLIDEAN inlier_rmse,
 * T = U T, the iteration count, the stop rule on absolute differences, max_iteration = 0, empty clouds and the corr
 * output are exactly those written out above.  Only U differs.
 * Additional input per Colored-ICP problem: source colours (n_s x 3 doubles), target colours (n_t x 3), target normals N
 * (n_t x 3, used as given), optionally target colour gradients (n_t x 3), and one teaser_icp_color_c record.
 * Intensity of a point with colour (r, g, b):  I = ((r + g) + b) / 3.0.
 * Colour gradient of target point i, x = Q[i], n = N[i], R = gradient_radius (<= 0: 2 max_correspondence_distance,
 * Open3D's choice):
 *   neighbourhood: exactly the covariance contract's above -- the points j (i itself included) with d2 < R R, in
 *                  ascending (d2, j), when there are more than gradient_max_nn the gradient_max_nn smallest.  m = their
 *                  number.  m < 4: the gradient is 0.
 *   slot 0 of that list is skipped, whichever point it is (Open3D skips point_idx[0]).  For slots k = 1 .. m - 1 in
 *   list order, y = the neighbour, j its index:
 *     o = y - x,  s = (o0 n0 + o1 n1) + o2 n2,  a = o - s n   (per component a_c = o_c - s n_c)
 *     b = I[j] - I[i]
 *     G += a a^T (upper triangle, six sums),  h += a b          one neighbour at a time from 0
 *   then the orthogonality row:  w = (double)(m - 1),  G[r][c] += (w n_r)(w n_c)
 *   solve G d = h by 3 x 3 LDL^T without pivoting (the recurrences of the 6 x 6 solve of point-to-plane);  d = 0 when a
 *   pivot is not finite or not > 0, or when d is not finite.  No fused operations anywhere.
 * Step U.  With c = the problem's target bounding-box centre, sg = sqrt(lambda_geometric), sp = sqrt(1 -
 * lambda_geometric), and for every correspondence (i, j) of C in ascending i, x = the current moved source point,
 * q = Q[j], n = N[j], d = gradient[j], Is = the source intensity, It = the target intensity:
 *   x' = x - c,  q' = q - c,  e = x' - q',  s = (e0 n0 + e1 n1) + e2 n2
 *   Jg = sg [ x' x n ; n ]  (each entry multiplied by sg),  rg = sg s,  wg = kernel(rg)
 *   u  = e - s n,  isp = ((d0 u0 + d1 u1) + d2 u2) + It
 *   t  = (d0 n0 + d1 n1) + d2 n2,  dm = t n - d                     (= -(I - n n^T) d)
 *   Ji = sp [ x' x dm ; dm ],  ri = sp (Is - isp),  wi = kernel(ri)
 *   A += (wg Jg[r]) Jg[c] + (wi Ji[r]) Ji[c]  (c >= r),   g += (wg rg) Jg[r] + (wi ri) Ji[r]
 *   -- the geometric term first, then the photometric one; each entry is ONE sum over the correspondences.
 *   solve A xi = -g by the LDL^T of point-to-plane;  R = Rz(gamma) Ry(beta) Rx(alpha);  U = [ R | t' + c - R c ];  the
 *   identity fall-backs are those of point-to-plane.
 * Robust kernels: the five of point-to-plane, applied to each of the two residuals (Open3D does the same).  With
 * lambda_geometric = 1 the step is point-to-plane's operation for operation, up to the sign of zeros.
 * Differences from Open3D (this states the FORMULATION; bit parity with Open3D is not claimed and was not measured):
 *   - the step is linearised in the frame centred on c, as for point-to-plane;
 *   - a is formed from the centred o = y - x rather than as vt_proj - vt;
 *   - the 3 x 3 LDL^T is unpivoted where Eigen's is pivoted.
 * Methods 0 - 3 go through the _color entry points below; the older entry points keep refusing method 3 ("method").
 * Problems of methods 0, 1 and 2 give the same bits through the _color entry points as through _cov, alone or mixed
 * with coloured problems.  Gradients that are not given are estimated inside the call, written on the device into the
 * buffer the correspondence pass gathers from and never copied to the host; the result is, bit for bit, that of
 * teaser_hip_icp_color_gradients_batch followed by the call with those gradients given.  Target normals are not estimated
 * inside the call (teaser_hip_icp_normals_batch first).
 * TEASER_HIP_ERR_BAD_ARG (argument and problem named) in addition to the lists above, for a method-3 problem:
 * lambda_geometric outside [0, 1] or not finite, gradient_max_nn outside [4, TEASER_HIP_ICP_COV_MAX_NN], reserved != 0,
 * a gradient radius whose square is not finite and > 0, n_src > 0 and no src_colors, n_dst > 0 and no dst_colors or no
 * dst_normals, a non-finite colour, normal or given gradient. */
typedef struct teaser_icp_color_c {
  double lambda_geometric; /* 0.968 (Open3D's default); [0, 1] */
  double gradient_radius;  /* <= 0: 2 max_correspondence_distance */
  int32_t gradient_max_nn; /* 30; [4, TEASER_HIP_ICP_COV_MAX_NN] */
  int32_t reserved;        /* 0 */
} teaser_icp_color_c;
#ifdef __cplusplus
static_assert(sizeof(teaser_icp_color_c) == 24, "teaser_icp_color_c is 24 bytes");
#else
_Static_assert(sizeof(teaser_icp_color_c) == 24, "teaser_icp_color_c is 24 bytes");
#endif
TEASER_HIP_API int32_t teaser_hip_icp_color_default(teaser_icp_color_c* color);
/* teaser_hip_icp_batch_cov plus src_colors / dst_colors (NULL, or per problem NULL unless the problem is Colored ICP,
 * else n x 3 doubles), dst_gradients (NULL, or per problem NULL = "estimate on the device", else n_dst x 3 doubles) and
 * color (NULL = the defaults for every problem, else one record per problem; read for method 3 only).  All borrowed
 * for the call. */
TEASER_HIP_API int32_t teaser_hip_icp_batch_color(teaser_hip_icp* icp, int32_t batch, const double* const* src,
                                                  const int32_t* n_src, const double* const* dst,
                                                  const int32_t* n_dst, const double* init,
                                                  const teaser_icp_params_c* params, teaser_icp_result_c* out,
                                                  int32_t* const* corr, const double* const* dst_normals,
                                                  const teaser_icp_estimation_c* est, const double* const* src_cov,
                                                  const double* const* dst_cov, const double* const* src_colors,
                                                  const double* const* dst_colors,
                                                  const double* const* dst_gradients,
                                                  const teaser_icp_color_c* color);
/* One problem: teaser_hip_icp_batch_color with batch = 1. */
TEASER_HIP_API int32_t teaser_hip_icp_solve_color(teaser_hip_icp* icp, const double* src, int32_t n_src,
                                                  const double* dst, int32_t n_dst, const double* init,
                                                  const teaser_icp_params_c* params, teaser_icp_result_c* out,
                                                  int32_t* corr, const double* dst_normals,
                                                  const teaser_icp_estimation_c* est, const double* src_cov,
                                                  const double* dst_cov, const double* src_colors,
                                                  const double* dst_colors, const double* dst_gradients,
                                                  const teaser_icp_color_c* color);
/* The colour gradients of the rule above for a batch of clouds: points, normals and colours (n x 3 doubles each), a
 * radius and a max_nn in [4, TEASER_HIP_ICP_COV_MAX_NN] per cloud; out[b]: n[b] x 3 doubles.  Empty clouds are legal.
 * Deterministic like every call on this handle.  TEASER_HIP_ERR_BAD_ARG (argument and cloud named): non-finite points,
 * normals or colours, a radius (or its square) that is not finite and > 0, max_nn outside its range, NULL where n > 0.
 * Performance only: a call whose largest max_nn exceeds 32 runs every cloud through the kernel with the longer list. */
TEASER_HIP_API int32_t teaser_hip_icp_color_gradients_batch(teaser_hip_icp* icp, int32_t batch,
                                                            const double* const* points, const int32_t* n,
                                                            const double* const* normals,
                                                            const double* const* colors, const double* radius,
                                                            const int32_t* max_nn, double* const* out);

/* Self k-NN (no radius), on the ICP handle: a batch of clouds (n x 3 doubles each) and a k in
 * [1, TEASER_HIP_ICP_KNN_MAX] per cloud (TEASER_HIP_ICP_KNN_MAX = 100, the same number as TEASER_HIP_ICP_COV_MAX_NN).
 * Per point i: the points j of the SAME cloud, i itself included, in ascending (d2, j), d2 = ((dx dx + dy dy) + dz dz),
 * dx = P[i].x - P[j].x (the expression of the covariance contract, never contracted); the first m = min(k, n) of them
 * are written.  idx_out[b]: n x k int32, unused slots -1; d2_out (NULL, or per cloud NULL or) n x k doubles, unused
 * slots +inf.  Copies of a point tie on d2 = 0 and come in index order (slot 0 of point i is i only when no copy of it
 * has a smaller index).  Deterministic: the same bits for a cloud alone, inside any batch and run after run; the result
 * does not depend on which search route served a point (a hash grid searched ring by ring, or a scan of the whole cloud
 * for the queries still open after "knn_ring_cap" rings: DESIGN.md section 17).  Empty clouds are legal.
 * TEASER_HIP_ERR_BAD_ARG (argument and cloud named): non-finite points, k outside its range, NULL where n > 0. */
#define TEASER_HIP_ICP_KNN_MAX 100
TEASER_HIP_API int32_t teaser_hip_icp_self_knn_batch(teaser_hip_icp* icp, int32_t batch, const double* const* points,
                                                     const int32_t* n, const int32_t* k, int32_t* const* idx_out,
                                                     double* const* d2_out);
/* Neighbour search between two clouds (Open3D's KDTreeFlann / core.nns.NearestNeighborSearch), on the ICP handle:
 * k-NN, hybrid and uncapped radius search, batched.  Problem b has a data cloud data[b] (n_data[b] x 3 doubles) and a
 * query set query[b] (n_query[b] x 3 doubles); the neighbours of query i are points j of the data cloud.
 *   d2(i, j) = ((dx dx + dy dy) + dz dz), dx = Q[i].x - P[j].x, never contracted (the expression used everywhere on this
 *   handle); every order is ascending (d2, j).  n_data = 0 and n_query = 0 are legal; queries may lie anywhere, far
 *   outside the data's bounding box included.  Deterministic: the same bits for a problem alone, inside any batch, in any
 *   batch position, run after run, and whichever route served a query.
 *   TEASER_HIP_ERR_BAD_ARG (argument and problem named): non-finite coordinates on either side, a parameter out of
 *   range, NULL where the matching n > 0.
 * knn_search:    k[b] in [1, TEASER_HIP_ICP_KNN_MAX].  Row i holds the min(k, n_data) smallest (d2, j) over the whole data
 *                cloud, then -1 / +inf.  idx_out[b]: n_query x k int32; d2_out: NULL, or per problem NULL or n_query x k
 *                doubles.  The options "knn_ring_cap" / "knn_fallbacks" are those of self k-NN: the rings are counted from
 *                the first ring that can touch the data's grid, "knn_fallbacks" is the number of queries of the call that
 *                the scan of the whole data cloud served.  Two clouds that overlap in part send every query far from the
 *                data there.
 * hybrid_search: radius, like its square, finite and > 0; max_nn[b] in [1, TEASER_HIP_ICP_KNN_MAX].  The neighbours are the
 *                j with d2 < radius radius (strict, as in the radius-outlier and covariance contracts); row i holds the
 *                first min(max_nn, number inside) of them, then -1 / +inf.  idx_out[b] / d2_out[b]: n_query x max_nn;
 *                count_out: NULL, or per problem NULL or n_query int32, the number written per row.
 * radius_search: uncapped.  count_out[b][i] (int32; required where n_query > 0) = the number of j with
 *                d2 < radius radius; total_out[b] (int64; required) = their sum over the problem's queries.  Row i
 *                occupies the slots [prefix(i), prefix(i) + count[i]) of idx_out[b] (int32) and d2_out[b] (doubles; NULL,
 *                or per problem NULL), prefix = the exclusive sum of count_out[b], in ascending (d2, j).  capacity[b]
 *                (int64, >= 0; may be NULL when idx_out is) = the entries the caller's arrays hold.  Where idx_out or
 *                idx_out[b] is NULL or capacity[b] < total, the problem gets its counts and its total only and its arrays
 *                are not touched: not an error, but the first half of count-then-fill (like the buf, len getters of the
 *                solver).  Device and host memory of a call: 12 bytes x the sum over the problems with arrays of
 *                min(capacity, n_query n_data), twice; a call that cannot get it fails with TEASER_HIP_ERR_OOM and leaves
 *                the handle usable.  Rows are ordered by ranking every entry inside its row, O(row length) per entry.
 * The last two have one route each and leave "knn_fallbacks" at 0. */
TEASER_HIP_API int32_t teaser_hip_icp_knn_search_batch(teaser_hip_icp* icp, int32_t batch, const double* const* data,
                                                       const int32_t* n_data, const double* const* query,
                                                       const int32_t* n_query, const int32_t* k,
                                                       int32_t* const* idx_out, double* const* d2_out);
TEASER_HIP_API int32_t teaser_hip_icp_hybrid_search_batch(teaser_hip_icp* icp, int32_t batch, const double* const* data,
                                                          const int32_t* n_data, const double* const* query,
                                                          const int32_t* n_query, const double* radius,
                                                          const int32_t* max_nn, int32_t* const* idx_out,
                                                          double* const* d2_out, int32_t* const* count_out);
TEASER_HIP_API int32_t teaser_hip_icp_radius_search_batch(teaser_hip_icp* icp, int32_t batch, const double* const* data,
                                                          const int32_t* n_data, const double* const* query,
                                                          const int32_t* n_query, const double* radius,
                                                          const int64_t* capacity, int32_t* const* count_out,
                                                          int32_t* const* idx_out, double* const* d2_out,
                                                          int64_t* total_out);
/* FPFH (Open3D form) (Open3D's compute_fpfh_feature with KDTreeSearchParamHybrid or KDTreeSearchParamKNN on normals that
 * are GIVEN), batched, FP64, on the ICP handle.  The PCL-form calls (teaser_hip_compute_fpfh and its batch) are another
 * descriptor with other bits and are untouched.  Per cloud: points P (n x 3 doubles), unit normals N (n x 3 doubles, used
 * as given), one search record (teaser_icp_normal_search_c: orient must be 0, ref is not read, max_nn in [2, 100]).
 *   list of i:    (j_0, d2_0), ..., (j_{m-1}, d2_{m-1}) in ascending (d2, j), i itself included, with
 *                 d2 = (e0 e0 + e1 e1) + e2 e2, e = P[i] - P[j] -- the rows of teaser_hip_icp_hybrid_search_batch /
 *                 _knn_search_batch with the cloud as its own query set.  search 0 (hybrid): the max_nn smallest with
 *                 d2 < radius radius.  search 1 (k-NN): the first min(max_nn, n).  Position 0 is skipped WHATEVER it
 *                 holds (Open3D skips by position, not by identity: among coincident points position 0 is the smallest
 *                 index of them).  Radius-only search (search 2, KDTreeSearchParamRadius) is refused by name for the
 *                 reason the normals contract gives: it is uncapped, so there is no bounded sorted list to sum over.
 *   pair (i, j_k), k >= 1, with (p1, n1) = (P[i], N[i]) and (p2, n2) = (P[j_k], N[j_k]).  dot(a, b) = (ax bx + ay by) +
 *                 az bz, cross(a, b) = (ay bz - az by, az bx - ax bz, ax by - ay bx) with every product rounded; no
 *                 product-add is fused anywhere:
 *                   dp = p2 - p1;  f3 = sqrt(dot(dp, dp));  f3 == 0: the pair is degenerate
 *                   a1 = dot(n1, dp) / f3;  a2 = dot(n2, dp) / f3
 *                   |a1| < |a2|: n1 <-> n2, dp = -dp, f2 = -a2; otherwise f2 = a1.  (Open3D tests acos(|a1|) >
 *                                acos(|a2|); stated on the cosines it is the same decision except where two different
 *                                cosines round to one arc cosine.)
 *                   v = cross(dp, n1);  |v| = sqrt(dot(v, v));  |v| == 0: the pair is degenerate;  v = v / |v| per
 *                   component;  w = cross(n1, v);  f1 = dot(v, n2)
 *                   f0 = atan2(dot(w, n2), dot(n1, n2)) by the deterministic FP64 formula of csrc/fdet_math.h (IEEE basic
 *                   operations in a fixed order: two argument halvings, a 25-term series)
 *                 A degenerate pair has f0 = f1 = f2 = 0 and is still binned (bins 5, 16 and 27), as in Open3D.
 *   SPFH row i:   33 doubles, zero when m <= 1.  Otherwise c = 100.0 / (double)(m - 1) and for k = 1 .. m-1, with
 *                 pi = 3.14159265358979323846, h0 = floor((11 (f0 + pi)) / (2.0 pi)), h1 = floor((11 (f1 + 1.0)) 0.5),
 *                 h2 = floor((11 (f2 + 1.0)) 0.5), each clamped to [0, 10] (a NaN, which only normals with overflowing
 *                 products can give, goes to 0): c is added to the bins h0, 11 + h1 and 22 + h2.  A bin's value is c added
 *                 one at a time from 0.0, as often as it was hit.
 *   FPFH row i:   zero when m <= 1.  Otherwise
 *                   F[0..32] = 0;  S[0..2] = 0
 *                   for k = 1 .. m-1 in list order:  if d2_k == 0: skip k
 *                       for j = 0 .. 32 in order:  val = SPFH[j_k][j] / d2_k  (the SQUARED distance, as in Open3D);
 *                                                  S[j / 11] += val;  F[j] += val
 *                   for g = 0 .. 2:  if S[g] != 0: S[g] = 100.0 / S[g]
 *                   for j = 0 .. 32: F[j] = F[j] S[j / 11];  F[j] = F[j] + SPFH[i][j]   (two roundings)
 *                 S[g] is one sequential chain over (k, then j inside the group).
 * fpfh_out[b]: n[b] x 33 doubles, one row per point: the transpose of Open3D's 33 x n Feature.data, the same memory as
 * Eigen's column-major matrix.  spfh_out: NULL, or per cloud NULL or n x 33 doubles.  Empty clouds are legal.
 * Normals inside the call: where normals[b] is NULL (or normals is NULL) and normal_search (NULL, or one record per
 * cloud; max_nn = 0 means "none given") has a record for the cloud, the cloud's normals are first estimated on the
 * device by the rule of teaser_hip_icp_normals_batch (any orient) and stay there; the result is bit-equal to that call
 * followed by this one on its normals.  normals_out: NULL, or per cloud NULL or n x 3 doubles: the normals the cloud
 * was computed with.  A cloud with neither normals nor a record: TEASER_HIP_ERR_BAD_ARG.
 * Deterministic like every call on this handle: a cloud gives the same bits alone, at any position in any batch, run
 * after run, for any value of "fpfh_list_bytes" (below) and, for k-NN search, of "knn_ring_cap"; "knn_fallbacks" is left
 * at 0.  Bit parity with an Open3D binary is NOT claimed: Open3D's libm (atan2, acos) and Eigen's summation order are
 * not ours; tests/fpfh_o3d_reference.py restates this text, and tests/test_fpfh_o3d_reference.py bounds its distance from
 * the libm form.  TEASER_HIP_ERR_BAD_ARG (argument and cloud named): non-finite points or normals; search, max_nn or
 * orient outside their ranges; reserved != 0; a radius (or its square) that is not finite and > 0 in hybrid search; NULL
 * where n > 0.  One stream synchronisation per call whatever the batch. */
TEASER_HIP_API int32_t teaser_hip_icp_fpfh_batch(teaser_hip_icp* icp, int32_t batch, const double* const* points,
                                                 const double* const* normals, const int32_t* n,
                                                 const teaser_icp_normal_search_c* search,
                                                 const teaser_icp_normal_search_c* normal_search,
                                                 double* const* fpfh_out, double* const* spfh_out,
                                                 double* const* normals_out);
/* Boundary points (Open3D's PointCloud.compute_boundary_points(radius, max_nn, angle_threshold): the angle criterion of
 * PCL's BoundaryEstimation, which PCL's ISS detector applies through setBorderRadius), batched, FP64, on the ICP handle.
 * Per cloud: points P (n x 3 doubles), normals N (n x 3 doubles, used as given and never normalised), one search record
 * (teaser_icp_normal_search_c: search 0 hybrid or 1 k-NN, max_nn in [2, 100], orient must be 0, ref is not read) and
 * angle_threshold[b], a double in degrees.  Radius-only search (search 2) is refused by name for the reason the FPFH
 * contract gives.  No product-add is fused anywhere; dot and cross are those of the FPFH contract.
 *   list of i:    exactly the list of the FPFH contract: ascending (d2, j), i itself included, length m.  Position 0 is
 *                 skipped WHATEVER it holds.
 *   frame of i:   Eigen's unitOrthogonal (PCL's getCoordinateSystemOnPlane).  With n = N[i]:
 *                   !(|n.x| <= 1e-12 |n.z|) || !(|n.y| <= 1e-12 |n.z|):
 *                              s = 1.0 / sqrt(n.x n.x + n.y n.y);  v = (-n.y s, n.x s, 0)
 *                   otherwise: s = 1.0 / sqrt(n.y n.y + n.z n.z);  v = (0, -n.z s, n.y s)
 *                   u = cross(n, v)
 *                 A component of u or v that is not finite (a zero or overflowing normal): the point is NOT a boundary
 *                 point and its max_gap is NaN, whatever m is.
 *   angles:       for k = 1 .. m-1:  delta = P[j_k] - P[i].  All three components zero: the angle is 0.0 (QUIRK, as in
 *                 Open3D: a coincident neighbour counts as a direction along u).  Otherwise
 *                 a_k = atan2(dot(v, delta), dot(u, delta)) by the deterministic formula of csrc/fdet_math.h.
 *                 An angle that is a NaN (delta or a dot product overflowed): NOT a boundary point, max_gap is NaN.
 *   gap:          m <= 1: NOT a boundary point, max_gap = 0.0.  Otherwise the m-1 angles are sorted in ascending order,
 *                 max_gap = 0.0; for consecutive sorted angles d = a[t+1] - a[t], and if d > max_gap then max_gap = d;
 *                 then, with pi = 3.14159265358979323846, d = (2.0 pi - a[last]) + a[first] under the same rule.
 *                 The set of differences does not depend on how equal angles (+0.0 and -0.0 included) are ordered, so
 *                 max_gap is a function of the inputs alone, whatever sort is used.
 *   boundary:     max_gap > (angle_threshold pi) / 180.0.
 * Nothing else is special-cased.  mask_out[b]: n[b] bytes, 0 or 1; the mask is the result and nothing is compacted.
 * n_boundary_out[b]: the number of ones.  max_gap_out: NULL, or per cloud NULL or n doubles.  count_out: NULL, or per
 * cloud NULL or n int32 holding m.  Empty clouds are legal.
 * Normals inside the call: where normals[b] is NULL (or normals is NULL) and normal_search (NULL, or one record per
 * cloud; max_nn = 0 means "none given") has a record for the cloud, the cloud's normals are first estimated on the
 * device by the rule of teaser_hip_icp_normals_batch (any orient) and stay there; the result is bit-equal to that call
 * followed by this one on its normals.  normals_out: NULL, or per cloud NULL or n x 3 doubles: the normals the cloud
 * was computed with.  A cloud with neither normals nor a record: TEASER_HIP_ERR_BAD_ARG.
 * Deterministic like every call on this handle: a cloud gives the same bits alone, at any position in any batch, run
 * after run, for any value of "fpfh_list_bytes" (which bounds the list scratch of this call as of the FPFH call) and of
 * "knn_ring_cap"; "knn_fallbacks" is left at 0.  Bit parity with an Open3D binary is NOT claimed: Open3D's libm and its
 * float32 path are not ours; tests/boundary_reference.py restates this text.  The tangent basis influences the mask only
 * through rounding at the threshold.  TEASER_HIP_ERR_BAD_ARG (argument and cloud named; the handle stays usable):
 * non-finite points or normals; search, max_nn or orient outside their ranges; reserved != 0; a radius (or its square)
 * that is not finite and > 0 in hybrid search; an angle_threshold that is not finite or lies outside [0, 360]; NULL
 * where n > 0.  One stream synchronisation per call whatever the batch. */
TEASER_HIP_API int32_t teaser_hip_icp_boundary_points_batch(teaser_hip_icp* icp, int32_t batch,
                                                            const double* const* points, const double* const* normals,
                                                            const int32_t* n, const teaser_icp_normal_search_c* search,
                                                            const teaser_icp_normal_search_c* normal_search,
                                                            const double* angle_threshold, uint8_t* const* mask_out,
                                                            int32_t* n_boundary_out, double* const* max_gap_out,
                                                            int32_t* const* count_out, double* const* normals_out);
/* Depth frames (Open3D's PointCloud.create_from_depth_image / create_from_rgbd_image and, the other way,
 * t.geometry.PointCloud.project_to_depth_image / project_to_rgbd_image), batched, FP64, on the ICP handle.  The text below
 * IS the contract; it restates Open3D and fixes what Open3D leaves to a race.  No product-add is fused and every sum is
 * taken left to right as written.  tests/rgbd_reference.py restates this text; bit parity with an Open3D binary is NOT
 * claimed.
 *
 * teaser_hip_icp_unproject_depth_batch: frames to clouds.  Per problem one record teaser_icp_frame_c, a depth image
 * depth[b] (height rows of depth_row_bytes bytes; uint16 or float32 samples) and, with color_format != 0, a colour image
 * color[b] (height rows of color_row_bytes bytes).  Rows may be padded; only the first width samples of a row are read.
 *   visited pixels: i = 0, stride, 2 stride, ... < height and inside that j = 0, stride, ... < width, in that row-major
 *                   order: ceil(height / stride) ceil(width / stride) of them.
 *   depth:          a uint16 sample d gives zf = (float)d / (float)depth_scale in float32, then zf = 0 if
 *                   (double)zf >= depth_trunc.  A float32 sample is zf as it is: neither scale nor truncation applies
 *                   (as in Open3D).  The pixel is valid iff zf > 0: NaN and negative samples are invalid, +inf is valid.
 *   point:          z = (double)zf;  x = (((double)j - cx) z) / fx;  y = (((double)i - cy) z) / fy;
 *                   p_r = ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3] for r = 0, 1, 2 with M = camera_pose, the
 *                   row-major 4 x 4 camera-to-world matrix (Open3D's extrinsic.inverse(); row 3 is not read).
 *   colour:         three doubles.  Format 1 (uint8 x 3, RGB): (R, G, B) / 255.0.  Format 1 with intensity = 1:
 *                   I = ((0.2990f R + 0.5870f G) + 0.1140f B) / 255.0f in float32 (R, G, B converted to float32 first), then
 *                   (I, I, I).  Format 2 (float32 x 1): (I, I, I).  Format 3 (float32 x 3): as it is.
 *   NaN:            a component of a point or a colour that is a NaN is stored as the quiet NaN 0x7ff8000000000000.
 *   rows:           valid_only = 1: one row per VALID visited pixel, packed in visiting order; count_out[b] is their number.
 *                   valid_only = 0: one row per visited pixel; an invalid pixel's point is (NaN, NaN, NaN), its colour is
 *                   computed all the same; count_out[b] is the number of visited pixels.
 * points_out[b]: room for the visited-pixel count x 3 doubles (required where that count is > 0).  colors_out: NULL, or
 * per problem NULL or as many rows (only with color_format != 0).  pixel_out: NULL, or per problem NULL or as many
 * int32: i width + j of every row.  Rows behind count_out[b] are not written.  A frame with width or height 0 is legal
 * and gives count 0; an empty batch and a batch of empty frames return OK without touching the device.
 * TEASER_HIP_ERR_BAD_ARG (argument and problem named; the handle stays usable): a depth_format outside {0, 1} or a
 * color_format outside {0 .. 3}; intensity outside {0, 1} or set without color_format 1; valid_only outside {0, 1};
 * reserved != 0; stride < 1; fx or fy zero or not finite; a pose, cx, cy, depth_scale or depth_trunc that is not finite;
 * depth_scale <= 0; row bytes below a row's size; width or height negative or above 16384; more than 2^31 - 1 visited
 * pixels in one call; NULL where something is required; colors_out[b] given for a frame without colour.
 *
 * teaser_hip_icp_project_depth_batch: clouds to frames.  Per problem points (n x 3 doubles), optionally colours (n x 3
 * doubles) and one record teaser_icp_projection_c; E = extrinsic, the row-major 4 x 4 world-to-camera matrix, used as
 * given (row 3 is not read).  For point k = (X, Y, Z):
 *   c_r = ((E[r][0] X + E[r][1] Y) + E[r][2] Z) + E[r][3] for r = 0, 1, 2;  (xc, yc, zc) = (c_0, c_1, c_2)
 *   skipped unless zc > 0 and zc <= depth_max (a NaN is skipped)
 *   u = (fx xc) / zc + cx;  v = (fy yc) / zc + cy;  skipped unless both are finite and below 2^31 in magnitude
 *   ui = round(u), vi = round(v), halves away from zero;  skipped unless 0 <= ui < width and 0 <= vi < height
 *   d = (float)(zc depth_scale);  skipped if d is not finite
 *   winner:  pixel (vi, ui) keeps the point with the smallest d and, among equal d, the smallest k (Open3D leaves this to
 *            a race).
 * depth_out[b]: height x width float32, the winner's d, 0 where no point landed (required where the image has pixels).
 * color_out: NULL, or per problem NULL or height x width x 3 float32: the winner's colour rounded to float32, 0 where
 * empty (only for a problem with colours).  index_out: NULL, or per problem NULL or height x width int32: the winner's
 * k, -1 where empty.  n_hit_out[b] (required): the number of non-empty pixels.  Images are dense, without row padding.
 * TEASER_HIP_ERR_BAD_ARG: as above for width, height, fx, fy, cx, cy, the matrix, depth_scale and (in place of
 * depth_trunc) depth_max, for more than 2^31 - 1 pixels in one call and for NULL; n < 0; non-finite points or colours;
 * color_out[b] given for a problem without colours.
 *
 * Both calls are deterministic like every call on this handle: a problem gives the same bits alone, at any position in
 * any batch, run after run.  The number of launches depends neither on the data nor on the batch; one stream
 * synchronisation per call. */
typedef struct teaser_icp_frame_c {
  int32_t width, height;
  int32_t depth_format;     /* 0 uint16, 1 float32 */
  int32_t color_format;     /* 0 none, 1 uint8 x 3 (RGB), 2 float32 x 1, 3 float32 x 3 */
  int64_t depth_row_bytes;  /* bytes from one row of the depth image to the next */
  int64_t color_row_bytes;  /* likewise for the colour image; not read with color_format 0 */
  int32_t intensity;        /* 1: a format-1 colour becomes its float32 intensity */
  int32_t stride;           /* every stride-th row and column is visited (default 1) */
  int32_t valid_only;       /* 1 (default): only valid pixels give rows */
  int32_t reserved;         /* must be 0 */
  double fx, fy, cx, cy;
  double camera_pose[16];   /* row-major, camera to world (default: identity) */
  double depth_scale;       /* default 1000.0 */
  double depth_trunc;       /* default 1000.0 */
} teaser_icp_frame_c;
typedef struct teaser_icp_projection_c {
  int32_t width, height;
  double fx, fy, cx, cy;
  double extrinsic[16];     /* row-major, world to camera */
  double depth_scale;
  double depth_max;
} teaser_icp_projection_c;
#ifdef __cplusplus
static_assert(sizeof(teaser_icp_frame_c) == 224, "teaser_icp_frame_c is 224 bytes");
static_assert(sizeof(teaser_icp_projection_c) == 184, "teaser_icp_projection_c is 184 bytes");
#else
_Static_assert(sizeof(teaser_icp_frame_c) == 224, "teaser_icp_frame_c is 224 bytes");
_Static_assert(sizeof(teaser_icp_projection_c) == 184, "teaser_icp_projection_c is 184 bytes");
#endif
/* Zeroes the record and sets the defaults noted beside the fields (the sizes, formats, row bytes and intrinsics are the
 * caller's to fill). */
TEASER_HIP_API int32_t teaser_hip_icp_frame_default(teaser_icp_frame_c* frame);
TEASER_HIP_API int32_t teaser_hip_icp_unproject_depth_batch(teaser_hip_icp* icp, int32_t batch,
                                                            const teaser_icp_frame_c* frames, const void* const* depth,
                                                            const void* const* color, int32_t* count_out,
                                                            double* const* points_out, double* const* colors_out,
                                                            int32_t* const* pixel_out);
TEASER_HIP_API int32_t teaser_hip_icp_project_depth_batch(teaser_hip_icp* icp, int32_t batch,
                                                          const double* const* points, const double* const* colors,
                                                          const int32_t* n, const teaser_icp_projection_c* cameras,
                                                          float* const* depth_out, float* const* color_out,
                                                          int32_t* const* index_out, int32_t* n_hit_out);
/* RGB-D odometry (Open3D's pipelines.odometry.compute_rgbd_odometry with RGBDOdometryJacobianFromColorTerm /
 * FromHybridTerm), batched, on the ICP handle: the motion between two RGB-D frames, source to target, with its 6 x 6
 * information matrix.  The text below IS the contract; it restates Open3D's Odometry.cpp, RGBDOdometryJacobian.cpp and
 * Image filters from knowledge and fixes what Open3D leaves to a race.  No product-add is fused; every sum is taken left
 * to right as written; "float32" operations round to float32 after every operation, everything else is FP64.
 * tests/odometry_reference.py restates this text; bit parity with an Open3D binary is NOT claimed.  Every float32 value
 * that is stored in an image is stored as the quiet NaN 0x7fc00000 when it is a NaN, every double that is handed out as
 * 0x7ff8000000000000.
 *
 * Per pair one record teaser_icp_odometry_pair_c and four images: source and target depth (uint16 or float32), source
 * and target colour (color_format 1: uint8 x 3, RGB; 2: float32 x 1, an intensity).  Rows may be padded; only the first
 * width samples of a row are read.  One record teaser_icp_odometry_option_c serves the call: n_levels L in 1 .. 8 and
 * iterations[0 .. L - 1], iterations[0] belonging to the COARSEST level (Open3D's iteration_number_per_pyramid_level).
 *
 * Images.  Level l of a pair has w_l = width >> l columns, h_l = height >> l rows, n_l = w_l h_l pixels and eleven
 * float32 planes, row-major: 0 I_s, 1 I_t (intensity of source, target), 2 D_s, 3 D_t (depth), 4 X, 5 Y, 6 Z (the source
 * XYZ image), 7 I_t dx, 8 I_t dy, 9 D_t dx, 10 D_t dy.  Level intrinsics: fx_l = fx 2^-l, and so fy_l, cx_l, cy_l.
 *   filter      F(p; kh, kv)(y, x) = (kv[0] H(y - 1, x) + kv[1] H(y, x)) + kv[2] H(y + 1, x) with
 *               H(y, x) = (kh[0] p(y, x - 1) + kh[1] p(y, x)) + kh[2] p(y, x + 1), float32, row and column indices clamped
 *               into the image.  Gaussian: kh = kv = (0.25, 0.5, 0.25).  Sobel dx: kh = (-1, 0, 1), kv = (1, 2, 1).  Sobel
 *               dy: kh = (1, 2, 1), kv = (-1, 0, 1).  A NaN propagates.
 *   1 convert   depth: zf by the rule of "Depth frames" (uint16: (float)d / (float)depth_scale, 0 when (double)zf >=
 *               depth_trunc; float32: the sample); then NaN when zf is not finite, (double)zf <= depth_min or (double)zf >
 *               depth_max.  Intensity: format 1 by the float32 formula of "Depth frames", format 2 the sample.
 *   2 smooth    planes 0 .. 3 of level 0 = the Gaussian of the converted images.
 *   3 match     the correspondences at level 0 and pose odo_init (below), n of them.
 *   4 normalise if n > 0: sum_s = SUM (double)I_s(source pixel), sum_t = SUM (double)I_t(target pixel) over the
 *               correspondences in the summation order (below); every I_s becomes (float)((0.5 / (sum_s / n)) (double)I_s),
 *               every I_t likewise with sum_t.  n = 0: the images stay.
 *   5 XYZ       level 0: z = D_s(y, x);  X = (float)((((double)x - cx) (double)z) (1.0 / fx)),
 *               Y = (float)((((double)y - cy) (double)z) (1.0 / fy)),  Z = z.
 *   6 pyramid   level l + 1 from level l:  q(y, x) = (((p(2y, 2x) + p(2y, 2x + 1)) + p(2y + 1, 2x)) + p(2y + 1, 2x + 1)) / 4.0f
 *               in float32, where p is the Gaussian of plane 0 or 1, and plane 2 .. 6 itself.
 *   7 gradients planes 7, 8 of every level = Sobel dx, dy of plane 1; planes 9, 10 = Sobel dx, dy of plane 3.
 *
 * Correspondences at level l and pose T = [R | t] (row-major 4 x 4, source to target).  With f = fx_l, g = fy_l, a = cx_l,
 * b = cy_l:  A[0][c] = f R[0][c] + a R[2][c];  A[1][c] = g R[1][c] + b R[2][c];  A[2][c] = R[2][c];
 *   M[r][0] = A[r][0] / f;  M[r][1] = A[r][1] / g;  M[r][2] = (A[r][2] - (A[r][0] a) / f) - (A[r][1] b) / g;
 *   Kt = (f t_0 + a t_2, g t_1 + b t_2, t_2)                                   (M = K R K^-1, Kt = K t)
 * For source pixel (v, u), index s = v w_l + u, with d = D_s(v, u) not a NaN:
 *   q_r = (double)d ((M[r][0] u + M[r][1] v) + M[r][2]) + Kt_r for r = 0, 1, 2;  skipped unless q_2 > 0
 *   x = q_0 / q_2 + 0.5, y = q_1 / q_2 + 0.5;  skipped unless both are finite and below 2^31 in magnitude
 *   ut = (int)x, vt = (int)y (truncated towards zero);  skipped unless 0 <= ut < w_l and 0 <= vt < h_l
 *   skipped if D_t(vt, ut) is a NaN, unless |q_2 - (double)D_t(vt, ut)| <= depth_diff_max, or if zf = (float)q_2 is not finite
 *   winner: target pixel (vt, ut) keeps the source pixel with the smallest zf and, among equal zf, the smallest s (the rule
 *   of "Depth frames"; Open3D leaves ties to a race).  The correspondences are listed in ascending target pixel vt w_l + ut.
 *
 * Summation order.  Every sum below runs over the n_l target pixels p = vt w_l + ut of the level; a pixel without a
 * correspondence contributes +0.0, as do the positions behind n_l.  Blocks of TEASER_HIP_ODOMETRY_BLOCK = 256 consecutive
 * pixels; within a block four runs of 64, each summed by the tree  for o = 32, 16, 8, 4, 2, 1: v[i] = v[i] + v[i + o] for
 * i < o;  block = (run_0 + run_1) + (run_2 + run_3).  Groups of TEASER_HIP_ODOMETRY_GROUP = 64 consecutive blocks: a group
 * sum starts at 0.0 and adds its block sums in ascending order; the total starts at 0.0 and adds the group sums in
 * ascending order.
 *
 * One iteration at level l (pose T).  The correspondences; then per correspondence (target (vt, ut), source (vs, us)):
 *   P = (X, Y, Z)(vs, us) as doubles;  p_r = ((R[r][0] P_0 + R[r][1] P_1) + R[r][2] P_2) + t_r
 *   dp = (double)(I_t(vt, ut) - I_s(vs, us)) (the difference in float32);  dg = (double)D_t(vt, ut) - p_2;  iz = 1.0 / p_2
 *   gIx = 0.125 (double)(I_t dx)(vt, ut), gIy, gDx, gDy likewise from planes 8, 9, 10;  a NaN gDx or gDy counts as 0
 *   c0 = (gIx f) iz;  c1 = (gIy g) iz;  c2 = (-(c0 p_0 + c1 p_1)) iz;  d0, d1, d2 likewise from gDx, gDy
 *   colour term (jacobian 0), one row:  J = ((-p_2) c1 + p_1 c2,  p_2 c0 - p_0 c2,  (-p_1) c0 + p_0 c1,  c0, c1, c2),  r = dp
 *   hybrid term (jacobian 1), two rows with sI = sqrt(1.0 - 0.968), sD = sqrt(0.968):  row 0 = sI times every component of
 *     the colour row, r_0 = sI dp;  row 1 = sD times (((-p_2) d1 + p_1 d2) - p_1,  (p_2 d0 - p_0 d2) + p_0,
 *     (-p_1) d0 + p_0 d1,  d0, d1, d2 - 1.0),  r_1 = sD dg
 *   the pixel's 29 values: J_i J_j for i <= j by rows (21), J_i r (6), r r, and 1.0 -- for two rows the value of row 0
 *   plus the value of row 1.
 * Their sums give A (symmetric 6 x 6), g, e and the count n.  A x = -g by LDL^T without pivoting:
 *   for j = 0 .. 5:  d_j = A[j][j] - SUM_{m < j} (L[j][m] L[j][m]) d_m (subtracted one at a time, m ascending);  the pair
 *   FAILS if d_j is zero or not finite;  L[i][j] = (A[i][j] - SUM_{m < j} (L[i][m] L[j][m]) d_m) / d_j for i > j.
 *   the pair FAILS if |((((d_0 d_1) d_2) d_3) d_4) d_5| < 1e-6
 *   y_i = -g_i - SUM_{m < i} L[i][m] y_m;  y_i = y_i / d_i;  x_i = y_i - SUM_{m > i} L[m][i] x_m for i = 5 .. 0 (m ascending)
 *   the pair FAILS if an x_i is not finite.
 * Update: (sa, ca), (sb, cb), (sc, cc) = the deterministic sine and cosine of x_0, x_1, x_2 (csrc/fdet_math.h,
 * fdet_sincos_d: the reduction and the series are written out there and are part of this contract);
 *   U = [[cc cb, (cc sb) sa - sc ca, (cc sb) ca + sc sa, x_3], [sc cb, (sc sb) sa + cc ca, (sc sb) ca - cc sa, x_4],
 *        [-sb, cb sa, cb ca, x_5]];  T'[r][c] = (U[r][0] T[0][c] + U[r][1] T[1][c]) + U[r][2] T[2][c], plus U[r][3] for
 *   c = 3;  row 3 stays (0, 0, 0, 1).
 * Levels run from L - 1 down to 0, level l for iterations[L - 1 - l] iterations (an entry may be 0), starting from
 * odo_init.  A pair that FAILS stops there: success = 0, transformation = the identity, information = zero, count = the
 * count of the failing iteration; the other pairs of the call are not touched by it.
 *
 * Information matrix of a pair that has not failed: the correspondences at level 0 and the final pose; count = their
 * number.  Per correspondence with z = D_t(vt, ut):  x = (double)(float)((((double)ut - cx) (double)z) (1.0 / fx)),
 * y likewise with vt, cy, fy, z = (double)z;  rows G_0 = (0, z, -y, 1, 0, 0), G_1 = (-z, 0, x, 0, 1, 0), G_2 = (y, -x, 0, 0,
 * 0, 1);  the pixel's values (G_0i G_0j + G_1i G_1j) + G_2i G_2j for i <= j, summed in the summation order; information is
 * the symmetric matrix.
 *
 * teaser_hip_icp_rgbd_odometry_batch: results[b] per pair.  trace_out: NULL, or per pair NULL or room for N = SUM
 * iterations[] records teaser_icp_odometry_trace_c, one per iteration in execution order: level, executed (0 for the
 * iterations behind a failure: the rest of such a record is zero), count, failed, e, A (21), g (6) and the pose after the
 * update (the identity when the iteration failed).
 * teaser_hip_icp_rgbd_odometry_pyramid_batch: steps 1 .. 7 alone, run by the same kernels.  images_out[b] takes
 * 11 SUM_l n_l float32: level l begins at 11 SUM_{k < l} n_k, plane p of it n_l p further on.
 * Both calls: batch = 0 does nothing.  The launch sequence depends on the options and the image sizes alone, never on
 * the data; one stream synchronisation per call.  Every output of a pair is a function of that pair alone: the same bits
 * alone, at any position of any batch, run after run.
 * TEASER_HIP_ERR_BAD_ARG (argument and pair named, before the device is asked for; the handle stays usable): NULL where
 * something is required; depth_format outside {0, 1}, color_format outside {1, 2}, jacobian outside {0, 1}; reserved != 0;
 * n_levels outside 1 .. 8; a negative iteration count; fx or fy not finite or not > 0; cx, cy, odo_init, depth_scale,
 * depth_trunc, depth_diff_max, depth_min or depth_max not finite; depth_scale <= 0; depth_diff_max < 0; depth_min < 0;
 * target_width / target_height different from width / height; width or height below 2^(n_levels - 1) (a level without a
 * pixel) or above 16384; row bytes below a row's size; more than 2^31 - 1 pixels in one call. */
#define TEASER_HIP_ODOMETRY_BLOCK 256
#define TEASER_HIP_ODOMETRY_GROUP 64
#define TEASER_HIP_ODOMETRY_MAX_LEVELS 8
typedef struct teaser_icp_odometry_option_c {
  int32_t n_levels;        /* default 3 */
  int32_t iterations[8];   /* default {20, 10, 5}: the first entry is the coarsest level's */
  int32_t reserved[3];     /* must be 0 */
  double depth_diff_max;   /* default 0.03 */
  double depth_min;        /* default 0.0 */
  double depth_max;        /* default 4.0 */
  double reserved2;        /* must be 0 */
} teaser_icp_odometry_option_c;
typedef struct teaser_icp_odometry_pair_c {
  int32_t width, height;                /* of the source images */
  int32_t target_width, target_height;  /* must equal them */
  int32_t depth_format;                 /* 0 uint16, 1 float32 (both depth images) */
  int32_t color_format;                 /* 1 uint8 x 3 (RGB), 2 float32 x 1 (both colour images) */
  int32_t jacobian;                     /* 0 colour term, 1 hybrid term */
  int32_t reserved;                     /* must be 0 */
  int64_t source_depth_row_bytes, source_color_row_bytes;
  int64_t target_depth_row_bytes, target_color_row_bytes;
  double fx, fy, cx, cy;
  double odo_init[16];                  /* row-major, source to target; row 3 must be finite and counts as (0, 0, 0, 1) */
  double depth_scale;                   /* uint16 depth only */
  double depth_trunc;
} teaser_icp_odometry_pair_c;
typedef struct teaser_icp_odometry_result_c {
  int32_t success;
  int32_t count;            /* correspondences at the final pose (of the failing iteration for a failed pair) */
  int32_t iterations;       /* iterations executed */
  int32_t reserved;
  double transformation[16];
  double information[36];
} teaser_icp_odometry_result_c;
typedef struct teaser_icp_odometry_trace_c {
  int32_t level, executed, count, failed;
  double e;
  double A[21];
  double g[6];
  double pose[16];
  double reserved[2];
} teaser_icp_odometry_trace_c;
#ifdef __cplusplus
static_assert(sizeof(teaser_icp_odometry_option_c) == 80, "teaser_icp_odometry_option_c is 80 bytes");
static_assert(sizeof(teaser_icp_odometry_pair_c) == 240, "teaser_icp_odometry_pair_c is 240 bytes");
static_assert(sizeof(teaser_icp_odometry_result_c) == 432, "teaser_icp_odometry_result_c is 432 bytes");
static_assert(sizeof(teaser_icp_odometry_trace_c) == 384, "teaser_icp_odometry_trace_c is 384 bytes");
#else
_Static_assert(sizeof(teaser_icp_odometry_option_c) == 80, "teaser_icp_odometry_option_c is 80 bytes");
_Static_assert(sizeof(teaser_icp_odometry_pair_c) == 240, "teaser_icp_odometry_pair_c is 240 bytes");
_Static_assert(sizeof(teaser_icp_odometry_result_c) == 432, "teaser_icp_odometry_result_c is 432 bytes");
_Static_assert(sizeof(teaser_icp_odometry_trace_c) == 384, "teaser_icp_odometry_trace_c is 384 bytes");
#endif
TEASER_HIP_API int32_t teaser_hip_icp_odometry_option_default(teaser_icp_odometry_option_c* option);
TEASER_HIP_API int32_t teaser_hip_icp_rgbd_odometry_batch(teaser_hip_icp* icp, int32_t batch,
                                                          const teaser_icp_odometry_pair_c* pairs,
                                                          const teaser_icp_odometry_option_c* option,
                                                          const void* const* source_depth,
                                                          const void* const* source_color,
                                                          const void* const* target_depth,
                                                          const void* const* target_color,
                                                          teaser_icp_odometry_result_c* results,
                                                          teaser_icp_odometry_trace_c* const* trace_out);
TEASER_HIP_API int32_t teaser_hip_icp_rgbd_odometry_pyramid_batch(teaser_hip_icp* icp, int32_t batch,
                                                                  const teaser_icp_odometry_pair_c* pairs,
                                                                  const teaser_icp_odometry_option_c* option,
                                                                  const void* const* source_depth,
                                                                  const void* const* source_color,
                                                                  const void* const* target_depth,
                                                                  const void* const* target_color,
                                                                  float* const* images_out);
/* Depth odometry (Open3D's t.pipelines.odometry.rgbd_odometry_multi_scale with Method.PointToPlane, the tracker of its
 * dense-SLAM loop, t.pipelines.slam.Model.track_frame_to_model), batched, on the ICP handle: the motion between two
 * DEPTH frames, source to target, by projective data association on vertex maps with a point-to-plane residual against
 * the target's normal map (KinectFusion), and its 6 x 6 information matrix.  No colour is read.  The text below IS the
 * contract; it restates Open3D from knowledge and fixes what Open3D leaves loose.  tests/depth_odometry_reference.py
 * restates this text; bit parity with an Open3D binary is NOT claimed.  The arithmetic follows "RGB-D odometry" above:
 * no product-add is fused; every sum is taken left to right as written; "float32" operations round to float32 after
 * every operation, everything else is FP64; every float32 NaN that is stored in an image is 0x7fc00000, every double NaN
 * that is handed out 0x7ff8000000000000.
 *
 * Per pair one record teaser_icp_depth_odometry_pair_c and two depth images of one size and format (uint16 or float32).
 * Rows may be padded; only the first width samples of a row are read.  One record teaser_icp_depth_odometry_option_c
 * serves the call: n_levels L in 1 .. 8 and iterations[0 .. L - 1], iterations[0] belonging to the COARSEST level.
 *
 * Images.  Level l of a pair has w_l = width >> l columns, h_l = height >> l rows, n_l = w_l h_l pixels and eleven
 * float32 planes, row-major: 0 D_s, 1 D_t (depth of source, target), 2 .. 4 the source vertex map (X, Y, Z), 5 .. 7 the
 * target vertex map, 8 .. 10 the target normal map.  Level intrinsics: fx_l = fx 2^-l, and so fy_l, cx_l, cy_l.
 *   1 convert   level 0, both images.  uint16: zf = (float)d / (float)depth_scale; float32: zf = the sample.  NaN when zf
 *               is not finite, (double)zf <= depth_min or (double)zf > depth_max.
 *   2 pyramid   level l + 1 from level l, both images.  c = D(2y, 2x); a NaN c gives NaN.  Otherwise with
 *               k = (0.0625, 0.25, 0.375, 0.25, 0.0625), thr = (float)(2.0 depth_outlier_trunc), float32 s = 0, ws = 0:
 *               for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner): the neighbour (2y + dy, 2x + dx) counts when it lies
 *               inside the image (one outside is skipped, not clamped), its value v is not a NaN and
 *               fabsf(v - c) < thr;  then wgt = k[dy + 2] k[dx + 2];  s = s + wgt v;  ws = ws + wgt.   out = s / ws.
 *   3 vertex    every level, both images, z = D(y, x).  A NaN z gives three NaNs.  Otherwise
 *               X = (float)((((double)x - cx_l) (double)z) (1.0 / fx_l)),  Y likewise from y, cy_l, fy_l,  Z = z.
 *   4 normal    every level, the target.  NaN unless x + 1 < w_l, y + 1 < h_l and the vertices V(y, x), V(y, x + 1),
 *               V(y + 1, x) are free of NaN.  a = V(y, x + 1) - V(y, x), b = V(y + 1, x) - V(y, x), componentwise in
 *               float32.  In FP64 m = b x a:  m0 = b1 a2 - b2 a1;  m1 = b2 a0 - b0 a2;  m2 = b0 a1 - b1 a0;
 *               len = sqrt((m0 m0 + m1 m1) + m2 m2).  NaN if len is zero or not finite, else N_i = (float)(m_i / len).
 *               The normal points towards the camera; its sign cancels in every sum below.
 *
 * 5 One iteration at level l, pose T = [R | t] (row-major 4 x 4, source to target).  For source pixel s = v w_l + u whose
 * vertex P is free of NaN, in doubles:
 *   p_r = ((R[r][0] P_0 + R[r][1] P_1) + R[r][2] P_2) + t_r;  skipped unless p_2 > 0
 *   x = ((fx_l p_0) / p_2 + cx_l) + 0.5, y likewise;  skipped unless both are finite, >= 0 and < 2^31
 *   ut = (int)x, vt = (int)y;  skipped unless ut < w_l and vt < h_l
 *   Q = the target vertex, N = the target normal at (vt, ut);  skipped if any of the six is a NaN
 *   r = ((p_0 - Q_0) N_0 + (p_1 - Q_1) N_1) + (p_2 - Q_2) N_2;  skipped unless |r| <= depth_outlier_trunc
 *   J = ((-p_2) N_1 + p_1 N_2,  p_2 N_0 - p_0 N_2,  (-p_1) N_0 + p_0 N_1,  N_0, N_1, N_2)
 *   Huber, delta = depth_huber_delta:  |r| < delta:  dh = r, lh = (0.5 r) r;  otherwise dh = delta with the sign of r,
 *   lh = delta (|r| - 0.5 delta)
 *   the pixel's 29 values: J_i J_j for i <= j by rows (21), J_i dh (6), lh, and 1.0.  A skipped pixel contributes +0.0.
 * Summation order: that of "RGB-D odometry" (blocks of TEASER_HIP_ODOMETRY_BLOCK, the tree inside a run of 64, groups of
 * TEASER_HIP_ODOMETRY_GROUP), taken over the level's n_l SOURCE pixels s.  The sums give A, g, e and the count.
 * Solve: the LDL^T of "RGB-D odometry" with its three failure rules.  Update: T = U(x) T as there, with fdet_sincos_d.
 * Measures, after the update: fitness_k = (double)count / (double)n_l, rmse_k = sqrt(e / (double)count).
 * Convergence: the level is converged behind this iteration if it is not the level's first iteration and
 *   |fitness_k - fitness_{k-1}| <= relative_fitness fitness_k  and  |rmse_k - rmse_{k-1}| <= relative_rmse rmse_k
 * (k - 1: the level's previous iteration), so a negative threshold never converges.  The level's remaining iterations
 * are then not executed: their trace records have executed = 0 and are zero otherwise, like the records behind a
 * failure.  Levels run from L - 1 down to 0, level l for at most iterations[L - 1 - l] iterations (an entry may be 0),
 * starting from init.  A pair that FAILS is reported as in "RGB-D odometry": success = 0, transformation = the identity,
 * information = zero, count = the count of the failing iteration; fitness = inlier_rmse = 0.
 *
 * 6 Information matrix of a pair that has not failed, at level 0 and the final pose: over the source pixels with the
 * projection of step 5; Q must be free of NaN (the normal is not looked at); skipped unless
 * ((p_0 - Q_0)^2 + (p_1 - Q_1)^2) + (p_2 - Q_2)^2 <= depth_outlier_trunc depth_outlier_trunc.  The rows G_0 .. G_2 of
 * "RGB-D odometry" from (x, y, z) = Q as doubles; the 21 values per pixel summed in the summation order.
 * Result: count, fitness, inlier_rmse = those of the last executed iteration (0 when none was executed); iterations =
 * the executed ones; converged_levels: bit l is set when level l converged.
 *
 * teaser_hip_icp_depth_odometry_pairs: results[b] per pair.  trace_out: NULL, or per pair NULL or room for N = SUM
 * iterations[] records teaser_icp_depth_odometry_trace_c, one per iteration in launch order: level, executed, count,
 * failed, converged (1 in the record of the iteration behind which the level converged), e, A (21), g (6) and the pose
 * after the update (the identity when the iteration failed).
 * teaser_hip_icp_depth_odometry_pyramid_pairs: steps 1 .. 4 alone, run by the same kernels.  images_out[b] takes
 * 11 SUM_l n_l float32: level l begins at 11 SUM_{k < l} n_k, plane p of it n_l p further on.
 * Both calls: batch = 0 does nothing.  The launch sequence depends on the options and the image sizes alone, never on
 * the data (the blocks of a pair that has failed or converged return at once); one stream synchronisation per call.
 * Every output of a pair is a function of that pair alone: the same bits alone, at any position of any batch, run after
 * run, whatever the handle's buffers held before.
 * TEASER_HIP_ERR_BAD_ARG (argument and pair named, before the device is asked for; the handle stays usable): NULL where
 * something is required; depth_format outside {0, 1}; reserved != 0; n_levels outside 1 .. 8; a negative iteration
 * count; fx or fy not finite or not > 0; cx, cy, init, depth_scale, depth_min or depth_max not finite; depth_scale <= 0;
 * depth_min < 0; depth_outlier_trunc or depth_huber_delta not finite or not > 0; relative_rmse or relative_fitness not
 * finite; width or height below 2^(n_levels - 1) (a level without a pixel) or above 16384; row bytes below a row's size;
 * more than 2^31 - 1 pixels in one call. */
typedef struct teaser_icp_depth_odometry_option_c {
  int32_t n_levels;            /* default 3 */
  int32_t iterations[8];       /* default {10, 5, 3}: the first entry is the coarsest level's */
  int32_t reserved[3];         /* must be 0 */
  double depth_outlier_trunc;  /* default 0.07 */
  double depth_huber_delta;    /* default 0.05 */
  double depth_min;            /* default 0.0 */
  double depth_max;            /* default 3.0 */
  double relative_rmse;        /* default 1e-6 */
  double relative_fitness;     /* default 1e-6 */
  double reserved2[2];         /* must be 0 */
} teaser_icp_depth_odometry_option_c;
typedef struct teaser_icp_depth_odometry_pair_c {
  int32_t width, height;       /* of both images */
  int32_t depth_format;        /* 0 uint16, 1 float32 (both images) */
  int32_t reserved;            /* must be 0 */
  int64_t source_depth_row_bytes, target_depth_row_bytes;
  double fx, fy, cx, cy;
  double init[16];             /* row-major, source to target; row 3 must be finite and counts as (0, 0, 0, 1) */
  double depth_scale;          /* uint16 depth only */
  double reserved2;            /* must be 0 */
} teaser_icp_depth_odometry_pair_c;
typedef struct teaser_icp_depth_odometry_result_c {
  int32_t success;
  int32_t count;               /* of the last executed iteration */
  int32_t iterations;          /* iterations executed */
  int32_t converged_levels;    /* bit l: level l converged */
  double fitness, inlier_rmse; /* of the last executed iteration */
  double transformation[16];
  double information[36];
} teaser_icp_depth_odometry_result_c;
typedef struct teaser_icp_depth_odometry_trace_c {
  int32_t level, executed, count, failed, converged, reserved;
  double e;
  double A[21];
  double g[6];
  double pose[16];
  double reserved2;
} teaser_icp_depth_odometry_trace_c;
#ifdef __cplusplus
static_assert(sizeof(teaser_icp_depth_odometry_option_c) == 112, "teaser_icp_depth_odometry_option_c is 112 bytes");
static_assert(sizeof(teaser_icp_depth_odometry_pair_c) == 208, "teaser_icp_depth_odometry_pair_c is 208 bytes");
static_assert(sizeof(teaser_icp_depth_odometry_result_c) == 448, "teaser_icp_depth_odometry_result_c is 448 bytes");
static_assert(sizeof(teaser_icp_depth_odometry_trace_c) == 384, "teaser_icp_depth_odometry_trace_c is 384 bytes");
#else
_Static_assert(sizeof(teaser_icp_depth_odometry_option_c) == 112, "teaser_icp_depth_odometry_option_c is 112 bytes");
_Static_assert(sizeof(teaser_icp_depth_odometry_pair_c) == 208, "teaser_icp_depth_odometry_pair_c is 208 bytes");
_Static_assert(sizeof(teaser_icp_depth_odometry_result_c) == 448, "teaser_icp_depth_odometry_result_c is 448 bytes");
_Static_assert(sizeof(teaser_icp_depth_odometry_trace_c) == 384, "teaser_icp_depth_odometry_trace_c is 384 bytes");
#endif
TEASER_HIP_API int32_t teaser_hip_icp_depth_odometry_option_default(teaser_icp_depth_odometry_option_c* option);
TEASER_HIP_API int32_t teaser_hip_icp_depth_odometry_pairs(teaser_hip_icp* icp, int32_t batch,
                                                           const teaser_icp_depth_odometry_pair_c* pairs,
                                                           const teaser_icp_depth_odometry_option_c* option,
                                                           const void* const* source_depth,
                                                           const void* const* target_depth,
                                                           teaser_icp_depth_odometry_result_c* results,
                                                           teaser_icp_depth_odometry_trace_c* const* trace_out);
TEASER_HIP_API int32_t teaser_hip_icp_depth_odometry_pyramid_pairs(teaser_hip_icp* icp, int32_t batch,
                                                                   const teaser_icp_depth_odometry_pair_c* pairs,
                                                                   const teaser_icp_depth_odometry_option_c* option,
                                                                   const void* const* source_depth,
                                                                   const void* const* target_depth,
                                                                   float* const* images_out);
/* Outlier removal: statistical (Open3D's remove_statistical_outlier), on the ICP handle.  Per cloud, with
 * nb_neighbors in [1, TEASER_HIP_ICP_KNN_MAX] and std_ratio finite and > 0:
 *   avg[i]    = (sum of sqrt(d2) over point i's m = min(nb_neighbors, n) nearest of self k-NN, the point itself
 *               included -- its 0 comes first --, added one term at a time in ascending (d2, j) from 0.0) / m
 *   valid     = n
 *   mean      = (SUM of avg[i] over the points with avg[i] > 0) / valid
 *   std       = sqrt((SUM of (avg[i] - mean)^2 over the same points) / (valid - 1))
 *   threshold = mean + std_ratio std
 *   SUM:        inside each block of 256 consecutive indices (0..255, 256..511, ...) the terms are added in ascending i
 *               from 0.0; then the block sums are added in ascending block order from 0.0
 *   kept:       point i is kept iff avg[i] > 0 and avg[i] < threshold.
 * What follows from the rule (nothing is special-cased): n = 1 keeps nothing (avg = 0; std = 0 / 0); nb_neighbors = 1
 * keeps nothing (every avg is 0); a point whose nb_neighbors nearest are all copies of itself has avg = 0 and is dropped,
 * and does not enter the sums although it counts in valid.
 * keep_out[b]: n bytes (0 / 1); n_kept_out[b]: int32; avg_out (NULL, or per cloud NULL or) n doubles; stats_out: NULL or
 * 3 doubles per cloud (mean, std, threshold; NaN for an empty cloud, which is legal and keeps nothing).  The mask is the
 * result: the host compacts nothing.  Deterministic like self k-NN.  TEASER_HIP_ERR_BAD_ARG (argument and cloud named):
 * non-finite points, nb_neighbors outside its range, a std_ratio that is not finite and > 0, NULL where n > 0. */
TEASER_HIP_API int32_t teaser_hip_icp_remove_statistical_outliers_batch(
    teaser_hip_icp* icp, int32_t batch, const double* const* points, const int32_t* n, const int32_t* nb_neighbors,
    const double* std_ratio, uint8_t* const* keep_out, int32_t* n_kept_out, double* const* avg_out, double* stats_out);
/* Outlier removal: radius (Open3D's remove_radius_outlier), on the ICP handle.  Per cloud, with nb_points >= 1 and a
 * radius that is, like its square, finite and > 0: count[i] = the number of j, i itself included, with
 * d2 < radius radius (d2 as above; the comparison of the covariance contract: a point at exactly the radius does not
 * count); point i is kept iff count[i] > nb_points.  keep_out / n_kept_out as above; count_out (NULL, or per cloud NULL
 * or) n int32.  TEASER_HIP_ERR_BAD_ARG as above, with radius and nb_points in place of std_ratio and nb_neighbors. */
TEASER_HIP_API int32_t teaser_hip_icp_remove_radius_outliers_batch(teaser_hip_icp* icp, int32_t batch,
                                                                   const double* const* points, const int32_t* n,
                                                                   const int32_t* nb_points, const double* radius,
                                                                   uint8_t* const* keep_out, int32_t* n_kept_out,
                                                                   int32_t* const* count_out);
/* ISS keypoints (Open3D's compute_iss_keypoints, PCL's ISSKeypoint3D), on the ICP handle: a batch of clouds (n x 3
 * doubles each) with one parameter record per cloud.  Nothing is fused; d2 = ((dx dx + dy dy) + dz dz),
 * dx = P[i].x - P[j].x, as everywhere on this handle.  Per cloud:
 *   resolution   (Open3D's ComputeModelResolution) only when salient_radius == 0 || non_max_radius == 0:
 *                res = SUM_i sqrt(d2 of slot 1 of point i's self k-NN with k = 2) / n, SUM the 256-index block rule of
 *                statistical outlier removal above; res = 0 when n < 2.  Then BOTH radii are replaced, as Open3D does:
 *                r_s = 6 res, r_n = 4 res.  Otherwise r_s, r_n are as given.
 *   no radius    a cloud whose r_s r_s or r_n r_n is not > 0 after this step (an empty cloud, n = 1 or identical points
 *                under automatic radii, a radius whose square underflows): no j has d2 < 0, so there are no neighbours
 *                and no keypoints; m = cnt = 0, saliency 0.  No grid is built and nothing divides by it.
 *   salient      neighbourhood of i: every j, i included, with d2 < r_s r_s.  NO cap.  m = their number.
 *   sum order    c(j) = the cell coordinates the handle's grid gives point j for radius r_s over this cloud: per axis a
 *                floor((P[j].a - lo_a) * (1 / h)) clamped to [-2, 2^40], lo = the bounding box's minimum,
 *                h = r_s (1 + 1e-6) + 1e-12 max |bounding-box coordinate|.  The neighbours are added one at a time from
 *                0 in ascending (c_x, c_y, c_z, j):  o = P[j] - P[i];  S1 = sum o;  S2 = sum o o^T (upper triangle);
 *                cov[a][b] = (S2[a][b] - (S1[a] S1[b]) / m) / m   (the POPULATION covariance of Open3D's
 *                ComputeCovariance).  This is the one place a contract names the grid: an order by (d2, j) needs a sort
 *                of an unbounded list per point, an order by j alone a 27-way merge; the cell order is the order a
 *                sorted grid stores the points in, so the sum is taken while streaming (voxel down-sampling fixes its
 *                output order the same way).
 *   saliency     sal[i] = 0 when m < min_neighbors.  Otherwise the cyclic Jacobi of the covariance contract above, word
 *                for word, and its three diagonal entries in ascending order e3 <= e2 <= e1 (three exchanges);
 *                sal[i] = e3 when e2 / e1 < gamma_21 and e3 / e2 < gamma_32, else 0.  IEEE divisions: 0 / 0 is NaN and
 *                a comparison with NaN is false, so a neighbourhood of copies gives 0 with nothing special-cased.
 *   suppression  cnt[i] = the number of j, i included, with d2 < r_n r_n.  Point i is a keypoint iff sal[i] > 0 and
 *                cnt[i] >= min_neighbors and no such j has sal[j] > sal[i] (ties survive together: Open3D's
 *                IsLocalMaxima with its strict <).  Any ratio r_n / r_s is served.
 * keep_out[b]: n bytes (0 / 1); n_keypoints_out[b]: int32; saliency_out (NULL, or per cloud NULL or) n doubles; count_out
 * (NULL, or per cloud NULL or) n x 2 int32 (m, cnt); radii_out: NULL or 3 doubles per cloud (res, NaN when it was not
 * computed; r_s; r_n).  The mask is the result: the host compacts nothing.  Empty clouds are legal.  Deterministic like
 * every call on this handle: the same bits alone, inside any batch, run after run; clouds of mixed sizes share the
 * launches.  "knn_fallbacks" is updated by the resolution's self k-NN (0 when no cloud asks for automatic radii).
 * TEASER_HIP_ERR_BAD_ARG (argument and cloud named): non-finite points; a radius that is negative or whose value or
 * square is not finite (also an automatic one); non-finite gammas; a negative min_neighbors; reserved != 0; NULL where
 * n > 0; and a radius so small against the cloud's extent that the cell keys of the call (grid id, c_x, c_y, c_z, each
 * with the bits its largest value needs) exceed 63 bits.  The handle stays usable after a refusal. */
typedef struct teaser_icp_iss_params_c {
  double salient_radius; /* >= 0; 0 (in either radius): both radii from the resolution */
  double non_max_radius; /* >= 0 */
  double gamma_21;       /* default 0.975 */
  double gamma_32;       /* default 0.975 */
  int32_t min_neighbors; /* >= 0, default 5 */
  int32_t reserved;      /* 0 */
} teaser_icp_iss_params_c;
#ifdef __cplusplus
static_assert(sizeof(teaser_icp_iss_params_c) == 40, "teaser_icp_iss_params_c is 40 bytes");
#else
_Static_assert(sizeof(teaser_icp_iss_params_c) == 40, "teaser_icp_iss_params_c is 40 bytes");
#endif
/* Open3D's defaults: radii 0 (automatic), gammas 0.975, min_neighbors 5. */
TEASER_HIP_API int32_t teaser_hip_icp_iss_params_default(teaser_icp_iss_params_c* params);
TEASER_HIP_API int32_t teaser_hip_icp_iss_keypoints_batch(teaser_hip_icp* icp, int32_t batch,
                                                          const double* const* points, const int32_t* n,
                                                          const teaser_icp_iss_params_c* params,
                                                          uint8_t* const* keep_out, int32_t* n_keypoints_out,
                                                          double* const* saliency_out, int32_t* const* count_out,
                                                          double* radii_out);
/* DBSCAN clustering (Open3D's PointCloud.cluster_dbscan), on the ICP handle: a batch of clouds (n x 3 doubles each)
 * with one parameter record per cloud.  Open3D's loop was restated in closed form (tests/dbscan_reference.py), not run:
 * its result is a function of the cloud alone, whatever order its unordered_set is popped in.  Per cloud of n points:
 *   neighbours   j is a neighbour of i iff d2(i, j) < eps eps, d2 = ((dx dx + dy dy) + dz dz), dx = P[i].x - P[j].x, in
 *                FP64 without contraction, as everywhere on this handle (nanoflann's strict radius rule).  d2 is
 *                symmetric bit for bit, and a point is its own neighbour when eps eps > 0.
 *                count[i] = the number of neighbours of i, itself included.  NO cap.
 *   core         i is a core point iff count[i] >= min_points.
 *   components   core points that are neighbours belong to one cluster; clusters are the connected components of that
 *                relation.  root[i] = the smallest point index among the core points of i's component; -1 for a point
 *                that is not core.
 *   numbering    clusters are numbered 0 .. c - 1 in ascending order of their root: the order in which Open3D's outer
 *                loop opens them (a cluster is opened at a core point and labelled whole before the loop moves on).
 *   border/noise a point that is not core gets the smallest label among the clusters of its core neighbours (the first
 *                cluster whose flood reaches it in Open3D, where -1 is overwritten once and never again), -1 without one.
 *   no radius    a cloud whose eps eps is not > 0: no neighbours; every count 0, every label and root -1, c = 0.  No
 *                grid is built for it and nothing divides by it.
 * Departures from Open3D: min_points >= 1 (its size_t accepts 0, which makes every point core).
 * labels_out[b]: n int32; n_clusters_out[b]: int32 (c); count_out (NULL, or per cloud NULL or) n int32; root_out (NULL,
 * or per cloud NULL or) n int32, the stage output of "components".  Empty clouds are legal.  Every output is an integer
 * and a function of the cloud and its record only: the same bits alone, inside any batch, in any batch position, run
 * after run, although the components are found by concurrent lock-free hooks (the smallest index of a component is its
 * root whatever the interleaving).  One upload, one copy back; the launches do not depend on the data.
 * TEASER_HIP_ERR_BAD_ARG (argument and cloud named): non-finite points; an eps that is negative or whose value or square
 * is not finite; min_points < 1; reserved != 0; NULL where it is required; total >= INT32_MAX points; and an eps so small
 * against the cloud's extent that the cell keys of the call (grid id, c_x, c_y, c_z, each with the bits its largest value
 * needs; the grid is that of ISS keypoints with h from eps) exceed 63 bits.  The handle stays usable after a refusal. */
typedef struct teaser_icp_dbscan_params_c {
  double eps;         /* >= 0, finite like its square */
  int32_t min_points; /* >= 1 */
  int32_t reserved;   /* 0 */
} teaser_icp_dbscan_params_c;
#ifdef __cplusplus
static_assert(sizeof(teaser_icp_dbscan_params_c) == 16, "teaser_icp_dbscan_params_c is 16 bytes");
#else
_Static_assert(sizeof(teaser_icp_dbscan_params_c) == 16, "teaser_icp_dbscan_params_c is 16 bytes");
#endif
TEASER_HIP_API int32_t teaser_hip_icp_cluster_dbscan_batch(teaser_hip_icp* icp, int32_t batch,
                                                           const double* const* points, const int32_t* n,
                                                           const teaser_icp_dbscan_params_c* params,
                                                           int32_t* const* labels_out, int32_t* n_clusters_out,
                                                           int32_t* const* count_out, int32_t* const* root_out);
/* Farthest-point down-sampling (Open3D's PointCloud.farthest_point_down_sample(num_samples, start_index)), on the ICP
 * handle: a batch of clouds (n x 3 doubles each) with one parameter record per cloud.  Open3D's loop was restated
 * (tests/fps_reference.py), not run.  Per cloud of n points P, K = num_samples, s = start_index:
 *   d[j] = +inf for all j;  cur = s
 *   for k = 0 .. K - 1:
 *     index[k]    = cur
 *     sel_dist[k] = d[cur]           before the update: +inf for k = 0, else the squared distance of sample k to the
 *                                    nearest earlier sample
 *     d[j] = min(d[j], d2(j, cur))   for all j; d2 = ((dx dx + dy dy) + dz dz), dx = P[j].x - P[cur].x, in FP64 without
 *                                    contraction, as everywhere on this handle
 *     m = the SMALLEST j among those with the largest d[j]
 *     if d[m] > 0: cur = m           else cur stays (Open3D's max_dist = 0 and its strict >): a cloud with fewer than K
 *                                    distinct positions repeats its last sample
 * index_out[b]: K int32 (required when K > 0); sel_dist_out (NULL, or per cloud NULL or) K doubles; final_dist_out (NULL,
 * or per cloud NULL or) n doubles: d after the last round, the squared distance of every point to its nearest sample.
 * K = 0 is legal, also for n = 0: nothing is written for the cloud and start_index is not looked at.  K = n is legal and
 * runs the loop as stated (Open3D's shortcut for it is the Python wrapper's business).  A d2 that overflows to +inf is
 * no error, and ties at +inf go to the smallest index like every tie.
 * min, and max under the total order on (distance, index), are exact, so the outputs are a function of (P, K, s) alone:
 * the same bits alone, inside any batch, in any batch position, run after run, and on both routes.  A cloud of at most
 * "fps_resident_max" points (an option of the handle, below) is served by one workgroup that keeps it in registers for
 * the whole loop, all such clouds of a call in ONE launch; the others by one launch per round, max K launches for all of
 * them.  One upload, one copy back, one synchronisation; the launch count depends on (n, K, the option) only.
 * TEASER_HIP_ERR_BAD_ARG (argument and cloud named): non-finite points; num_samples < 0 or > n; with num_samples > 0 a
 * start_index < 0 or >= n; NULL where it is required; total >= INT32_MAX points.  The handle stays usable after a
 * refusal. */
typedef struct teaser_icp_fps_params_c {
  int32_t num_samples; /* 0 .. n */
  int32_t start_index; /* 0 .. n - 1 when num_samples > 0 */
} teaser_icp_fps_params_c;
#ifdef __cplusplus
static_assert(sizeof(teaser_icp_fps_params_c) == 8, "teaser_icp_fps_params_c is 8 bytes");
#else
_Static_assert(sizeof(teaser_icp_fps_params_c) == 8, "teaser_icp_fps_params_c is 8 bytes");
#endif
TEASER_HIP_API int32_t teaser_hip_icp_farthest_point_down_sample_batch(teaser_hip_icp* icp, int32_t batch,
                                                                       const double* const* points, const int32_t* n,
                                                                       const teaser_icp_fps_params_c* params,
                                                                       int32_t* const* index_out,
                                                                       double* const* sel_dist_out,
                                                                       double* const* final_dist_out);
/* Options of an ICP handle (none changes a result).  "knn_ring_cap" (0 .. 16, default 4): the number of rings self
 * k-NN and statistical removal search on the grid before a query goes to the whole-cloud scan; 0 sends every query
 * there.  "knn_fallbacks" (read-only): how many queries of the handle's last self k-NN or statistical-removal call the
 * whole-cloud scan served.  "fps_resident_max" (0 .. 10240, the compiled capacity, which is also the default): the
 * largest cloud farthest-point down-sampling serves by its one-launch resident route; 0 sends every cloud to the
 * launch-per-round route.  "fpfh_list_bytes" (1 .. 2^40, default 512 MiB): the bound of the neighbour-list scratch of
 * teaser_hip_icp_fpfh_batch and teaser_hip_icp_boundary_points_batch (12 bytes per point and max_nn slot); a call
 * whose lists exceed it runs in several passes (the FPFH call then computes its lists twice); a piece of a cloud is
 * never smaller than 64 points.  An unknown name, a value outside the range or a write to a read-only option:
 * TEASER_HIP_ERR_BAD_ARG, from both calls with teaser_hip_icp_last_error naming the option. */
TEASER_HIP_API int32_t teaser_hip_icp_set_option(teaser_hip_icp* icp, const char* name, int64_t value);
TEASER_HIP_API int32_t teaser_hip_icp_get_option(teaser_hip_icp* icp, const char* name, int64_t* value);

/* Information matrices (Open3D's GetInformationMatrixFromPointClouds, the 6 x 6 weight a registered pair enters a
 * pose graph with, and evaluate_registration, whose result the same call returns): batched, on the ICP handle, from the
 * correspondences of a GIVEN pose.  Open3D's formulation was restated (tests/information_reference.py), not run.
 * Per problem: source P (n_s points), target Q (n_t points), T = transformation (4 x 4 row-major, last row 0 0 0 1),
 * r = max_correspondence_distance.  With apply and corr exactly as "ICP refinement" above defines them:
 *   X = apply(T, P);  C = corr(X)          -- the bits of teaser_hip_icp_batch with max_iteration = 0 and init = T:
 *                                             the same correspondence set, fitness, inlier_rmse and n_correspondences
 *   for every (i, j) of C, q = Q[j] in the caller's own coordinates (NOT centred: a pose graph takes its residual
 *   about the origin too):
 *     G_j = [ -[q]x | I3 ]   rows (0, q_z, -q_y, 1, 0, 0), (-q_z, 0, q_x, 0, 1, 0), (q_y, -q_x, 0, 0, 0, 1)
 *     information = SUM_j G_j^T G_j         (rotation block first: the order of Open3D's 6-vectors)
 *   so information[3:,3:] = |C| I3 and information(5,5) = |C| exactly, and an empty C (n_s = 0, n_t = 0, or no point
 *   within r) gives the zero matrix.  Per term nothing is fused: (0,0) = q_z q_z + q_y q_y, (0,1) = 0 - q_y q_x,
 *   (0,2) = 0 - q_z q_x, (1,1) = q_z q_z + q_x q_x, (1,2) = 0 - q_z q_y, (2,2) = q_y q_y + q_x q_x; the off-diagonal
 *   block holds the coordinates themselves.
 *   SUM: 21 FP64 sums (the upper triangle; the lower one is its mirror image, bit for bit).  The source points are cut
 *   into blocks of 256 consecutive indices (a point without a match adds 0); inside a block lane l of each 64-lane
 *   wave adds across lanes by xor 32, 16, 8, 4, 2, 1, then (w0 + w1) + (w2 + w3) over its four waves; the block
 *   results b = t, t + 256, ... are added in ascending order by thread t of a 256-thread block, which is then summed by
 *   the same rule.  No atomics: the same bits run to run, and for a problem alone or inside any batch.  With inputs
 *   for which every product and sum is exact (integer coordinates of moderate size) the result is THE sum, whatever
 *   the order.  In general |information - exact| <= (|C| + 3) 2^-52 SUM_j |term_j| elementwise.
 * transformation: batch x 16; max_correspondence_distance: [batch]; information: batch x 36 row-major; out: NULL, or
 * [batch] records (transformation echoed, iterations 0); corr: NULL, or as in teaser_hip_icp_batch.  Problems of mixed
 * sizes share the launches; one synchronisation per call.  TEASER_HIP_ERR_BAD_ARG (argument and problem named): a
 * non-finite transformation or one whose last row is not 0 0 0 1, a non-finite or non-positive r (or r r), non-finite
 * points, NULL where n > 0, a NULL transformation / max_correspondence_distance / information.  n = 0 is valid. */
TEASER_HIP_API int32_t teaser_hip_icp_information_batch(teaser_hip_icp* icp, int32_t batch, const double* const* src,
                                                        const int32_t* n_src, const double* const* dst,
                                                        const int32_t* n_dst, const double* transformation,
                                                        const double* max_correspondence_distance,
                                                        double* information, teaser_icp_result_c* out,
                                                        int32_t* const* corr);
/* One problem: teaser_hip_icp_information_batch with batch = 1.  out may be NULL; corr NULL or room for n_src x 2. */
TEASER_HIP_API int32_t teaser_hip_icp_information(teaser_hip_icp* icp, const double* src, int32_t n_src,
                                                  const double* dst, int32_t n_dst, const double* transformation,
                                                  double max_correspondence_distance, double* information,
                                                  teaser_icp_result_c* out, int32_t* corr);

/* Voxel down-sampling (the reference's 3DMatch tutorial, examples/teaser_python_fpfh_icp/example.py:19-20, runs
 * Open3D's pcd.voxel_down_sample(0.05) on the raw clouds): batched, with Open3D's arithmetic and a deterministic output
 * order, on its OWN handle (nothing is shared with teaser_hip_solver or teaser_hip_icp).
 * Per problem: n points p (xyz interleaved doubles, the layout ICP takes) and a voxel size v.  In FP64 per axis a:
 *   lo_a = min_bound_a - 0.5 v,  hi_a = max_bound_a + 0.5 v      (min / max_bound: componentwise min / max of the points)
 *   i_a  = floor((p_a - lo_a) / v)                                  (an IEEE division: no reciprocal, nothing fused)
 * Every occupied voxel gives one output point: the FP64 sum of its points, added one at a time in input order
 * starting from 0 (Open3D's AccumulatedPoint), divided by the voxel's count.
 * Output order: ascending lexicographic (i_x, i_y, i_z).  This is the one deliberate difference from Open3D, which
 * emits its hash map's (unspecified) order.  Normals and colours are not handled (the tutorial never reads them after
 * down-sampling).
 * Optional outputs per problem: counts[k] = number of points in output voxel k; voxel_of_point[i] = output index of
 * input point i (maps keypoints back to the raw cloud).
 * n = 0 is valid (0 outputs); n points of room per problem always suffice and n_out[b] returns the number written.
 * TEASER_HIP_ERR_BAD_ARG (teaser_hip_voxel_last_error names the argument) for a voxel_size that is not finite or
 * <= 0, a non-finite point, a NULL pointer where n > 0, and -- Open3D's guard -- v * INT_MAX < max_a (hi_a - lo_a):
 * the voxel size is too small for 32-bit voxel indices.  The handle stays usable after a refusal.
 * Results are deterministic (no floating-point atomics): the same bits run to run, and for a problem alone or inside
 * any batch.  A voxel handle is not re-entrant (one call at a time; distinct handles are independent). */
typedef struct teaser_hip_voxel teaser_hip_voxel;
/* device < 0: the current device.  TEASER_HIP_ERR_NO_DEVICE without a GPU: there is no CPU path. */
TEASER_HIP_API int32_t teaser_hip_voxel_create(int32_t device, teaser_hip_voxel** out);
TEASER_HIP_API int32_t teaser_hip_voxel_destroy(teaser_hip_voxel* voxel);
TEASER_HIP_API const char* teaser_hip_voxel_last_error(const teaser_hip_voxel* voxel);
/* DIAGNOSTIC: fills the handle's scratch and staging buffers with `byte`; see teaser_hip_icp_fill_scratch. */
TEASER_HIP_API int32_t teaser_hip_voxel_fill_scratch(teaser_hip_voxel* voxel, int32_t byte, int64_t* bytes_out);
/* `batch` independent problems, HOST pointers per problem, borrowed for the call.  pts[b]: n[b] x 3 doubles;
 * voxel_size[b]; out[b]: room for n[b] x 3 doubles; n_out[b] receives the number of voxels.  counts and
 * voxel_of_point: NULL, or per problem NULL or room for n[b] int32.  Problems of mixed sizes share the launches. */
TEASER_HIP_API int32_t teaser_hip_voxel_down_sample_batch(teaser_hip_voxel* voxel, int32_t batch,
                                                          const double* const* pts, const int32_t* n,
                                                          const double* voxel_size, double* const* out,
                                                          int64_t* n_out, int32_t* const* counts,
                                                          int32_t* const* voxel_of_point);
/* One problem: teaser_hip_voxel_down_sample_batch with batch = 1; counts / voxel_of_point may be NULL. */
TEASER_HIP_API int32_t teaser_hip_voxel_down_sample(teaser_hip_voxel* voxel, const double* pts, int32_t n,
                                                    double voxel_size, double* out, int64_t* n_out, int32_t* counts,
                                                    int32_t* voxel_of_point);

/* Batched correspondence front-end: teaser_hip_compute_fpfh and teaser_hip_match_features (see "Correspondence
 * front-end" above for the arithmetic) for a BATCH of clouds / pairs per call, on its OWN handle.  This is the one
 * implementation of the front-end: those two calls on a teaser_hip_solver are batches of one, run on a features handle
 * that the solver handle creates at their first use and destroys with itself (they keep their own argument checks:
 * they accept every radius > 0).  Problems of mixed sizes share the launches; radii are given per problem.  A call waits for its stream (hipStreamSynchronize) a fixed number of times whatever the batch: twice where
 * FPFH is computed, once for matching alone.  The copies of requested features / normals into the caller's arrays, and
 * of the features match_batch reads from them, are one per problem and additional.  Neighbour lists that would exceed
 * an internal budget (4 GiB per wave of clouds) are built in several waves inside the call, with the same results.
 * n = 0 clouds, empty sides (zero pairs) and batch = 0 are valid.  TEASER_HIP_ERR_BAD_ARG
 * (teaser_hip_features_last_error names the argument and the problem index) for a negative n, a NULL pointer where
 * n > 0, a radius that is not finite and > 0, dim outside [1, 64], a pair_cap[b] that is too small (n_pairs[b] then
 * holds the count needed, for every problem) and non-finite features that leave a query without a nearest neighbour.
 * The handle stays usable after a refusal.  Results are deterministic: the same bits run to run, and for a problem
 * alone or inside any batch.  A handle is not re-entrant (one call at a time; distinct handles are independent). */
typedef struct teaser_hip_features teaser_hip_features;
/* device < 0: the current HIP device.  TEASER_HIP_ERR_NO_DEVICE without a GPU. */
TEASER_HIP_API int32_t teaser_hip_features_create(int32_t device, teaser_hip_features** out);
TEASER_HIP_API int32_t teaser_hip_features_destroy(teaser_hip_features* features);
TEASER_HIP_API const char* teaser_hip_features_last_error(const teaser_hip_features* features);
/* DIAGNOSTIC: fills the handle's scratch and staging buffers with `byte`; see teaser_hip_icp_fill_scratch. */
TEASER_HIP_API int32_t teaser_hip_features_fill_scratch(teaser_hip_features* features, int32_t byte, int64_t* bytes_out);
/* DIAGNOSTIC (exists for the tests of the wave splitting; may be removed): the budgets of one wave in bytes, each
 * <= 0 for its default -- list_bytes: neighbour lists of a wave of clouds (4 GiB); part_bytes: partial nearest-
 * neighbour results of a wave of searches (1 GiB).  Small values force a call into many waves; no value changes a result. */
TEASER_HIP_API int32_t teaser_hip_features_set_budgets(teaser_hip_features* features, int64_t list_bytes,
                                                       int64_t part_bytes);
/* FPFH of `batch` clouds.  cloud[b]: n[b] x 3 floats; fpfh_out[b]: n[b] x 33 floats; normals_out: NULL, or per cloud
 * NULL or n[b] x 3 floats. */
TEASER_HIP_API int32_t teaser_hip_features_fpfh_batch(teaser_hip_features* features, int32_t batch,
                                                      const float* const* cloud, const int32_t* n,
                                                      const double* normal_radius, const double* fpfh_radius,
                                                      float* const* fpfh_out, float* const* normals_out);
/* Matching of `batch` feature pairs.  src_feat[b]: n_src[b] x dim floats, dst_feat[b] likewise; pairs[b]: room for
 * pair_cap[b] (src, dst) pairs (n_src[b] + n_dst[b] always suffices); n_pairs[b] receives the count. */
TEASER_HIP_API int32_t teaser_hip_features_match_batch(teaser_hip_features* features, int32_t batch,
                                                       const float* const* src_feat, const int32_t* n_src,
                                                       const float* const* dst_feat, const int32_t* n_dst,
                                                       int32_t dim, int32_t use_crosscheck, int32_t* const* pairs,
                                                       const int64_t* pair_cap, int64_t* n_pairs);
/* Clouds in, correspondences out: FPFH of both clouds of every pair, then matching, the features staying on the
 * device in between.  Optional outputs (each array NULL, or per pair NULL or room for the side's n x 33 features /
 * n x 3 normals). */
TEASER_HIP_API int32_t teaser_hip_features_correspondences_batch(
    teaser_hip_features* features, int32_t batch, const float* const* src_xyz, const int32_t* n_src,
    const float* const* dst_xyz, const int32_t* n_dst, const double* normal_radius, const double* fpfh_radius,
    int32_t use_crosscheck, int32_t* const* pairs, const int64_t* pair_cap, int64_t* n_pairs,
    float* const* src_feat_out, float* const* dst_feat_out, float* const* src_normals_out,
    float* const* dst_normals_out);

/* k-nearest-neighbour matching on the same handle (no counterpart in the reference library; its tutorial,
 * examples/teaser_python_fpfh_icp/helpers.py:19-43, feeds the solver the k nearest descriptors per point from a host
 * KD-tree).  Everything the comment above promises holds here too: mixed sizes, empty sides, batch = 0, one
 * synchronisation for search or matching alone and two where FPFH is computed, the same refusals, and the same bits
 * run to run, for a problem alone or inside any batch, and for any value of the part_bytes budget.
 *   Distance.  The distance of a query row q to a data row x is the 1-NN search's, unchanged: in float,
 *     d = 0; for c in 0 .. dim-1: t = q_c - x_c; d += t * t     (every operation rounded, nothing fused).
 *   k nearest.  The k nearest of a query are the k_eff = min(k, nd) smallest candidates under the lexicographic order
 *     (d, data index): ties go to the lower index, and the slots appear in ascending (d, index) order.
 *     k lies in [1, TEASER_HIP_FEATURES_KNN_MAX].
 *   Non-finite values.  A candidate whose d is NaN or +inf never enters a list.  A query that ends with fewer than
 *     k_eff entries therefore had non-finite features: TEASER_HIP_ERR_BAD_ARG naming the problem index.
 *   Lists.  For a pair with source features S (n_src rows) and target features T (n_dst rows): F[i] = the k nearest
 *     rows of T for source row i; B[j] = the k nearest rows of S for target row j.
 *   Pairs.  mutual = 0: all (i, j) with j in F[i].  mutual = 1: only those where also i is in B[j].  Output: (src, dst)
 *     int32 pairs in ascending lexicographic order, without duplicates; n_src x min(k, n_dst) pairs of room always
 *     suffice, and a pair_cap[b] that is too small behaves as in match_batch (every n_pairs[b] reports the count
 *     needed, the call returns TEASER_HIP_ERR_BAD_ARG).
 *   Relation to match_batch.  With k = 1 and mutual = 1 the pairs equal those of
 *     teaser_hip_features_match_batch(..., use_crosscheck = 1) exactly.  With mutual = 0 the result is deliberately the
 *     tutorial's one-directional set {(i, j): j in F[i]}, NOT the reference matcher's two-directional union
 *     (use_crosscheck = 0). */
#define TEASER_HIP_FEATURES_KNN_MAX 16
/* The raw search of `batch` problems.  data_feat[b]: n_data[b] x dim floats, query_feat[b]: n_query[b] x dim floats;
 * idx[b]: n_query[b] x k int32 (indices of data rows); dist: NULL, or per problem NULL or n_query[b] x k floats (the
 * squared distances d).  Slots beyond k_eff hold -1 / +inf. */
TEASER_HIP_API int32_t teaser_hip_features_knn_batch(teaser_hip_features* features, int32_t batch,
                                                     const float* const* data_feat, const int32_t* n_data,
                                                     const float* const* query_feat, const int32_t* n_query,
                                                     int32_t dim, int32_t k, int32_t* const* idx, float* const* dist);
/* Features in, pairs out (arguments as teaser_hip_features_match_batch, with k and mutual in place of
 * use_crosscheck). */
TEASER_HIP_API int32_t teaser_hip_features_match_knn_batch(teaser_hip_features* features, int32_t batch,
                                                           const float* const* src_feat, const int32_t* n_src,
                                                           const float* const* dst_feat, const int32_t* n_dst,
                                                           int32_t dim, int32_t k, int32_t mutual,
                                                           int32_t* const* pairs, const int64_t* pair_cap,
                                                           int64_t* n_pairs);
/* Clouds in, pairs out: FPFH of both clouds of every pair, then the k-NN matching, the features staying on the device
 * in between (arguments and optional outputs as teaser_hip_features_correspondences_batch). */
TEASER_HIP_API int32_t teaser_hip_features_correspondences_knn_batch(
    teaser_hip_features* features, int32_t batch, const float* const* src_xyz, const int32_t* n_src,
    const float* const* dst_xyz, const int32_t* n_dst, const double* normal_radius, const double* fpfh_radius,
    int32_t k, int32_t mutual, int32_t* const* pairs, const int64_t* pair_cap, int64_t* n_pairs,
    float* const* src_feat_out, float* const* dst_feat_out, float* const* src_normals_out,
    float* const* dst_normals_out);

/* The tuple constraint for `batch` problems on the GPU: the contract is written out under "tuple_test_batch" in the
 * "Correspondence front-end" comment above.  src_xyz[b]: n_src[b] x 3 floats, dst_xyz[b] likewise; tuple_scale and
 * seed: one value per problem; pairs[b]: n_pairs[b] (src, dst) int32 pairs on entry, the survivors on return, and
 * n_pairs[b] their count.  One upload of the packed points and pairs, one launch sequence for all problems, one copy
 * of the keep flags back and one synchronisation, whatever the batch; compaction, sort and unique of the survivors run
 * on the host.  Problems whose pairs exceed the part_bytes budget together are run in several waves inside the call,
 * with the same results. */
TEASER_HIP_API int32_t teaser_hip_features_tuple_test_batch(teaser_hip_features* features, int32_t batch,
                                                            const float* const* src_xyz, const int32_t* n_src,
                                                            const float* const* dst_xyz, const int32_t* n_dst,
                                                            const float* tuple_scale /* per problem */,
                                                            const uint64_t* seed /* per problem */,
                                                            int32_t* const* pairs /* in / out */,
                                                            int64_t* n_pairs /* in / out */);

/* Pose-graph optimisation: Open3D's global_optimization with GlobalOptimizationLevenbergMarquardt (Levenberg-Marquardt
 * with a line process on the uncertain edges, then edge pruning and a second pass) for a BATCH of graphs per call, on
 * its OWN handle.  It consumes the 6 x 6 matrices of "Information matrices" above as edge weights.  Everything is FP64.
 *   Data.  n node poses T_i (4 x 4 row-major, node i's frame -> the common frame); m edges (s, t, X, L, uncertain): X
 *     aligns s to t, so a consistent graph has T_t^-1 T_s = X; L is the 6 x 6 information matrix (the upper triangle is
 *     read and taken symmetric), rotation block first.
 *   V(xi)    xi = (a, b, c, tx, ty, tz): R = Rz(c) Ry(b) Rx(a), translation (tx, ty, tz)
 *   v6(M)    its inverse: sy = sqrt(M00^2 + M10^2); sy > 1e-6: a = atan2(M21, M22), b = atan2(-M20, sy),
 *            c = atan2(M10, M00); otherwise a = atan2(-M12, M11), b = atan2(-M20, sy), c = 0; then the translation
 *   inverse  of a pose or an edge transformation: the transpose of the rotation block and -(R^T t)
 *   edge k   e_k = v6(X^-1 T_t^-1 T_s), r_k = e_k^T L e_k; l_k = 1 (certain) or (mu / (mu + r_k))^2 (uncertain)
 *   F        SUM l_k r_k + SUM_uncertain mu (sqrt(l_k) - 1)^2
 *   mu       preference_loop_closure * max_correspondence_distance^2 * mean over the pass's uncertain edges of L(5,5);
 *            0 without uncertain edges; fixed per pass from the edges the pass starts with
 *   Jacobian left perturbation T_i <- V(d_i) T_i: J_s[:, c] = lin6(X^-1 T_t^-1 D_c T_s), D_c the six generators of V
 *            at 0, lin6(M) = ((M21 - M12)/2, (M02 - M20)/2, (M10 - M01)/2, M03, M13, M23); J_t = -J_s
 *   system   A_k = l_k J^T L J (computed on its upper triangle and mirrored) goes into the blocks (s,s), (t,t) with
 *            + and (s,t), (t,s) with -; b_k = l_k J^T L e_k into g(s) with + and g(t) with -; every entry is summed
 *            over its edges in ascending edge index.  The reference node is held: its six unknowns are left out, so
 *            the system has N = 6 (n - 1) unknowns.
 *   LM loop of one pass (tau = 1e-5), in trials; T, F, H, g belong to the current poses:
 *     start  lam = tau * max diag H, nu = 2, it = 0, lm = 0; |g|inf <= min_right_term -> stop RIGHT_TERM
 *     trial  solve (H + lam I) d = -g by Cholesky; a pivot that is not finite or not positive -> rejected step
 *            |d|2 <= min_relative_increment (|x|2 + min_relative_increment), x the stacked v6 of the free poses
 *                -> stop INCREMENT
 *            T' = V(d_i) T_i, F' = F(T'), rho = (F - F') / d^T (lam d - g)
 *            rho > 0:  F - F' < min_relative_residual_increment F -> stop REL_RESIDUAL (the step is not taken)
 *                      accept: lam *= max(lower_scale_factor, min(upper_scale_factor, 1 - (2 rho - 1)^3)), nu = 2,
 *                      T = T', relinearise; |g|inf <= min_right_term -> stop RIGHT_TERM; it += 1, lm = 0;
 *                      F < min_residual -> stop RESIDUAL; it >= max_iteration -> stop MAX_ITERATION
 *            else      (a NaN rho and a failed factorisation too) lam *= nu, nu *= 2, lm += 1;
 *                      lm >= max_iteration_lm -> stop MAX_ITERATION_LM
 *   Passes.  After pass one every uncertain edge with l_k < edge_prune_threshold (l_k at the final poses) is pruned;
 *     if any was, pass two runs from pass one's poses without them.  edge_prune_threshold = 0: one pass.
 *   Trivial graphs.  n = 0, n = 1 or m = 0 return the input, confidence 1 and status TRIVIAL.  batch = 0 is valid.
 * One workgroup owns a graph and runs both passes in one launch: a call waits for its stream once, whatever the batch
 * and the number of trials.  The system is dense, which is why n is limited; more nodes need another method.
 * TEASER_HIP_ERR_BAD_ARG (teaser_hip_posegraph_last_error names the argument and the problem index) when anything
 * read is not finite, the last row of a pose or an edge transformation is not 0 0 0 1, an edge endpoint is out of
 * range or source == target, reference_node >= n, a limit below is exceeded, an iteration cap is negative, or an
 * array that is needed is NULL.  A refusal leaves every output untouched and the handle usable.  The information
 * matrices are NOT checked for positive definiteness: an indefinite system ends as rejected trials.
 * Results are deterministic: the same bits run to run, and for a graph alone or at any position of any batch.  A
 * handle is not re-entrant (one call at a time; distinct handles are independent). */
#define TEASER_HIP_POSEGRAPH_MAX_NODES 128
#define TEASER_HIP_POSEGRAPH_MAX_EDGES 16384
#define TEASER_HIP_POSEGRAPH_MAX_ITERATION 1000   /* max_iteration and max_iteration_lm bound one kernel's */
#define TEASER_HIP_POSEGRAPH_MAX_ITERATION_LM 100 /* running time */
/* Why a pass stopped (the status of the last pass run is reported). */
#define TEASER_HIP_PG_RIGHT_TERM 0
#define TEASER_HIP_PG_INCREMENT 1
#define TEASER_HIP_PG_REL_RESIDUAL 2
#define TEASER_HIP_PG_RESIDUAL 3
#define TEASER_HIP_PG_MAX_ITERATION 4
#define TEASER_HIP_PG_MAX_ITERATION_LM 5
#define TEASER_HIP_PG_TRIVIAL 6
typedef struct teaser_posegraph_option_c {
  int32_t max_iteration;    /* 100 */
  int32_t max_iteration_lm; /* 20 */
  double min_relative_increment;          /* 1e-6 */
  double min_relative_residual_increment; /* 1e-6 */
  double min_right_term;                  /* 1e-6 */
  double min_residual;                    /* 1e-6 */
  double upper_scale_factor;              /* 2/3 */
  double lower_scale_factor;              /* 1/3 */
  double max_correspondence_distance;     /* 0.03 */
  double edge_prune_threshold;            /* 0.25 */
  double preference_loop_closure;         /* 1.0 */
  int32_t reference_node;                 /* -1: node 0 */
  int32_t reserved;
} teaser_posegraph_option_c;
typedef struct teaser_posegraph_result_c {
  double F0, F;          /* the objective at the input poses (pass one's weights) and at the end of the last pass */
  double mu[2];          /* per pass; 0 for a pass that did not run */
  int32_t iterations[2]; /* accepted steps per pass */
  int32_t trials[2];     /* trace rows per pass: trials that reached the gain ratio or failed to factorise */
  int32_t status;        /* TEASER_HIP_PG_* of the last pass run */
  int32_t n_trace;       /* rows the call produced, whether or not they fitted */
} teaser_posegraph_result_c;
/* One trial: lam it was solved with, the gain ratio and F' (0 when the factorisation failed), and whether the step
 * was accepted (rho > 0).  A trial that stops with INCREMENT leaves no row. */
typedef struct teaser_posegraph_trace_c {
  double lam, rho, F_new;
  int32_t pass, accepted, factorised, reserved;
} teaser_posegraph_trace_c;
typedef struct teaser_hip_posegraph teaser_hip_posegraph;
/* device < 0: the current HIP device.  TEASER_HIP_ERR_NO_DEVICE without a GPU. */
TEASER_HIP_API int32_t teaser_hip_posegraph_create(int32_t device, teaser_hip_posegraph** out);
TEASER_HIP_API int32_t teaser_hip_posegraph_destroy(teaser_hip_posegraph* posegraph);
TEASER_HIP_API const char* teaser_hip_posegraph_last_error(const teaser_hip_posegraph* posegraph);
/* DIAGNOSTIC: fills the handle's scratch and staging buffers with `byte`; see teaser_hip_icp_fill_scratch. */
TEASER_HIP_API int32_t teaser_hip_posegraph_fill_scratch(teaser_hip_posegraph* posegraph, int32_t byte, int64_t* bytes_out);
/* The defaults noted beside the fields above. */
TEASER_HIP_API int32_t teaser_hip_posegraph_option_default(teaser_posegraph_option_c* out);
/* `batch` graphs as concatenated arrays: n_nodes[b] and poses (16 doubles per node); n_edges[b], edge_source,
 * edge_target (node indices within the graph), edge_transformation (16 doubles per edge), edge_information (36 per
 * edge), edge_uncertain (one byte per edge); options: NULL for the defaults, or one record per graph.  Outputs, each
 * laid out like its input: poses_out (16 per node; the reference node's pose is the input's, bit for bit), confidence
 * (the final l_k; of a pruned edge its value when it was pruned), pruned (one byte per edge), results (one record per
 * graph); confidence, pruned and results may be NULL.  trace: NULL, or room for SUM trace_cap[b] rows, graph b's rows
 * starting at SUM_{c<b} trace_cap[c]; rows beyond a graph's capacity are dropped, results[b].n_trace counts them all. */
TEASER_HIP_API int32_t teaser_hip_posegraph_optimize_batch(
    teaser_hip_posegraph* posegraph, int32_t batch, const int32_t* n_nodes, const double* poses,
    const int32_t* n_edges, const int32_t* edge_source, const int32_t* edge_target, const double* edge_transformation,
    const double* edge_information, const uint8_t* edge_uncertain, const teaser_posegraph_option_c* options,
    double* poses_out, double* confidence, uint8_t* pruned, teaser_posegraph_result_c* results,
    teaser_posegraph_trace_c* trace, const int32_t* trace_cap);
/* One graph: teaser_hip_posegraph_optimize_batch with batch = 1; trace_cap is the room of `trace` in rows. */
TEASER_HIP_API int32_t teaser_hip_posegraph_optimize(
    teaser_hip_posegraph* posegraph, int32_t n_nodes, const double* poses, int32_t n_edges,
    const int32_t* edge_source, const int32_t* edge_target, const double* edge_transformation,
    const double* edge_information, const uint8_t* edge_uncertain, const teaser_posegraph_option_c* option,
    double* poses_out, double* confidence, uint8_t* pruned, teaser_posegraph_result_c* result,
    teaser_posegraph_trace_c* trace, int32_t trace_cap);
/* Stage call: the linearisation at the given poses, with pass one's mu.  Per graph, concatenated: e (6 per edge), r,
 * l (one per edge), mu, F (one per graph), H ((6 n)^2 per graph, row-major; the reference node's rows and columns are
 * zero and the lower triangle mirrors the upper bit for bit) and g (6 n per graph).  Any output may be NULL. */
TEASER_HIP_API int32_t teaser_hip_posegraph_linearize_batch(
    teaser_hip_posegraph* posegraph, int32_t batch, const int32_t* n_nodes, const double* poses,
    const int32_t* n_edges, const int32_t* edge_source, const int32_t* edge_target, const double* edge_transformation,
    const double* edge_information, const uint8_t* edge_uncertain, const teaser_posegraph_option_c* options,
    double* e, double* r, double* l, double* mu, double* F, double* H, double* g);
/* One graph: teaser_hip_posegraph_linearize_batch with batch = 1. */
TEASER_HIP_API int32_t teaser_hip_posegraph_linearize(
    teaser_hip_posegraph* posegraph, int32_t n_nodes, const double* poses, int32_t n_edges,
    const int32_t* edge_source, const int32_t* edge_target, const double* edge_transformation,
    const double* edge_information, const uint8_t* edge_uncertain, const teaser_posegraph_option_c* option,
    double* e, double* r, double* l, double* mu, double* F, double* H, double* g);

/* RANSAC registration on correspondences: Open3D's registration_ransac_based_on_correspondence with
 * TransformationEstimationPointToPoint(with_scaling = false), CorrespondenceCheckerBasedOnEdgeLength and
 * CorrespondenceCheckerBasedOnDistance, batched, on its OWN handle.  Open3D is RESTATED here, not run: what follows is
 * the contract, and where it departs from Open3D it says so.
 * Per problem: source P (n_s x 3 doubles) and target Q (n_t x 3 doubles), xyz interleaved; ncorr pairs (i, j) int32,
 * used in the caller's order, repeats allowed; r = max_correspondence_distance; ransac_n in 3 .. 8; max_iteration
 * (int32 >= 0); confidence in [0, 1]; a uint64 seed; optionally the edge-length checker with its threshold s in (0, 1]
 * and the distance checker with its threshold d > 0.  apply(T, p) is the ICP contract's (above), nothing fused.
 *   trial i (int64, from 0): its samples are c_k = z(seed, ransac_n i + k + 1) mod ncorr for k = 0 .. ransac_n - 1,
 *            z(seed, m) the splitmix64 finaliser of seed + m 0x9E3779B97F4A7C15 exactly as the tuple-test contract
 *            writes it (wrapping 64-bit arithmetic, the exact 64-bit remainder).  A trial is a function of (seed, i)
 *            alone and samples WITH replacement, as Open3D does (Open3D draws from its own generator, so its trials are
 *            other trials).  seed = 0 means "from the clock": the call reads time(NULL) once and uses that value for
 *            every problem whose seed is 0.
 *   edge-length checker: for all a < b among the samples, ls = |P[i_a] - P[i_b]|, lt = |Q[j_a] - Q[j_b]|, each
 *            sqrt((dx dx + dy dy) + dz dz) in FP64 with a correctly rounded sqrt; the trial fails when ls < lt s or
 *            lt < ls s for any pair.
 *   estimate: Umeyama without scaling on the ransac_n sampled pairs: mu_P, mu_Q = the sums in sample order divided by
 *            ransac_n; H = sum (p - mu_P)(q - mu_Q)^T in sample order; R = V diag(1, 1, det) U^T from the SVD of H as
 *            the ICP contract's umeyama, t = mu_Q - R mu_P, T = [R | t].  Where rank(H) <= 1 (repeated samples,
 *            collinear triples) R is a maximiser of tr(R H) among the proper rotations, not a specified one, exactly
 *            as the ICP contract words it; H = 0 gives the identity rotation.
 *   distance checker: the trial fails when sqrt(d2(apply(T, P[i_k]), Q[j_k])) > d for any sample k.
 *   score    of a trial that passed its checkers, over ALL ncorr pairs in input order: x = apply(T, P[i]),
 *            d2 = (dx dx + dy dy) + dz dz, dx = x.x - Q[j].x; the pair is an inlier iff d2 < r r -- the rule of corr()
 *            above.  Open3D compares sqrt(d2) < r: the two differ only for a pair at the boundary.  count = the number
 *            of inliers; S = the sum of d2 over the inliers in this order: the pairs are cut into blocks of 256
 *            consecutive input positions, a block's inliers are added in ascending position starting from 0, and the
 *            block sums are added in ascending block order starting from 0.  fitness = count / ncorr,
 *            inlier_rmse = sqrt(S / count), 0 when count = 0.
 *   loop     Open3D's, as ONE thread runs it (Open3D runs it in parallel and its result depends on the schedule):
 *            best = {identity, count 0, rmse 0}, est_k = max_iteration; for i = 0, 1, ... while i < max_iteration and
 *            i < est_k: a trial that fails a checker is skipped; it replaces best iff count > best.count, or
 *            count == best.count and rmse < best.rmse (strict: ties stay with the earlier trial); on a replacement
 *            k = log(1 - confidence) / log(1 - pow(count / ncorr, ransac_n)) in host double with the C library's log
 *            and pow, and if k < est_k then est_k = ceil(k).  The IEEE special cases fall as they fall: confidence = 1
 *            gives k = +inf or NaN and never stops early; count = ncorr gives k = 0 and stops at once; a ratio so
 *            small that 1 - pow(..) rounds to 1 gives k = -inf and stops at once, too.
 * Output per problem: the winning trial's T bit for bit, fitness, inlier_rmse, n_correspondences = its inlier count,
 * best_trial (-1: no trial replaced the start), trials = the loop indices visited, valid_trials = those of them that
 * passed their checkers, and optionally the inlier pairs of T in input order.  The result is a function of the inputs
 * alone: not of how the trials are cut into launches ("chunk_trials" below), not of the batch around the problem, and
 * the same bits run to run.  Work past the stopping trial is discarded, never reported.
 * ncorr < ransac_n or max_iteration = 0 is not an error: the result is the start (identity, zeros, best_trial = -1,
 * trials = 0).  TEASER_HIP_ERR_BAD_ARG (teaser_hip_ransac_last_error names the argument and the problem), found on the
 * host before anything is launched or written: a non-finite or non-positive r, ransac_n outside 3 .. 8, a confidence
 * outside [0, 1] or NaN, a negative max_iteration, a checker threshold out of range, an index outside its cloud,
 * non-finite points, NULL where a count is positive.  NOT OFFERED, and refused by name with the same status rather
 * than stubbed: with_scaling, point-to-plane estimation inside RANSAC, the normal-angle checker. */
typedef struct teaser_ransac_params_c {
  double max_correspondence_distance; /* r; no default (Open3D's argument is required) */
  int32_t ransac_n;                   /* 3 */
  int32_t max_iteration;              /* 100000 */
  double confidence;                  /* 0.999 */
  uint64_t seed;                      /* 0: from the clock */
  double edge_length_threshold;       /* 0: checker off; else s in (0, 1] (Open3D's similarity_threshold) */
  double distance_threshold;          /* 0: checker off; else d > 0 */
  int32_t with_scaling;               /* must be 0 */
  int32_t estimation;                 /* must be 0 (point to point) */
  int32_t normal_checker;             /* must be 0 */
  int32_t reserved;
} teaser_ransac_params_c;
typedef struct teaser_ransac_result_c {
  double transformation[16]; /* row-major 4 x 4 */
  double fitness;
  double inlier_rmse;
  int64_t best_trial;
  int64_t trials;
  int64_t valid_trials;
  int32_t n_correspondences;
  int32_t reserved;
} teaser_ransac_result_c;
typedef struct teaser_hip_ransac teaser_hip_ransac;
/* device < 0: the current HIP device.  TEASER_HIP_ERR_NO_DEVICE without a GPU: there is no CPU path. */
TEASER_HIP_API int32_t teaser_hip_ransac_create(int32_t device, teaser_hip_ransac** out);
TEASER_HIP_API int32_t teaser_hip_ransac_destroy(teaser_hip_ransac* ransac);
TEASER_HIP_API const char* teaser_hip_ransac_last_error(const teaser_hip_ransac* ransac);
/* DIAGNOSTIC: fills the handle's scratch and staging buffers with `byte`; see teaser_hip_icp_fill_scratch. */
TEASER_HIP_API int32_t teaser_hip_ransac_fill_scratch(teaser_hip_ransac* ransac, int32_t byte, int64_t* bytes_out);
/* The defaults noted beside the fields above (Open3D's RANSACConvergenceCriteria; both checkers off). */
TEASER_HIP_API int32_t teaser_hip_ransac_params_default(teaser_ransac_params_c* params);
/* `batch` independent problems, HOST pointers per problem, borrowed for the call: src[b] n_src[b] x 3, dst[b]
 * n_dst[b] x 3, corr[b] n_corr[b] x 2 int32 (source index, target index); params and out: one per problem; inliers:
 * NULL, or per problem NULL or room for n_corr[b] x 2 int32, out[b].n_correspondences pairs written.
 * A batch holds at most 65535 problems (the grids carry the problem in blockIdx.y or blockIdx.z): more, in this call
 * or the stage call below, is refused with
 * TEASER_HIP_ERR_UNSUPPORTED before anything is allocated or copied, and the handle stays usable. */
TEASER_HIP_API int32_t teaser_hip_ransac_correspondence_batch(
    teaser_hip_ransac* ransac, int32_t batch, const double* const* src, const int32_t* n_src,
    const double* const* dst, const int32_t* n_dst, const int32_t* const* corr, const int32_t* n_corr,
    const teaser_ransac_params_c* params, teaser_ransac_result_c* out, int32_t* const* inliers);
/* One problem: teaser_hip_ransac_correspondence_batch with batch = 1; inliers NULL or room for n_corr x 2. */
TEASER_HIP_API int32_t teaser_hip_ransac_correspondence(teaser_hip_ransac* ransac, const double* src, int32_t n_src,
                                                        const double* dst, int32_t n_dst, const int32_t* corr,
                                                        int32_t n_corr, const teaser_ransac_params_c* params,
                                                        teaser_ransac_result_c* out, int32_t* inliers);
/* One knob per handle, "chunk_trials" in [64, 65536] (default 4096): the trials of a problem one launch sequence
 * covers.  A tuning switch: no value changes a bit of any result.  BAD_ARG for another name or a value out of range. */
TEASER_HIP_API int32_t teaser_hip_ransac_set_option(teaser_hip_ransac* ransac, const char* name, int64_t value);
TEASER_HIP_API int32_t teaser_hip_ransac_get_option(const teaser_hip_ransac* ransac, const char* name, int64_t* value);
/* Stage call (in the spirit of teaser_hip_certify_stages): trials first .. first + n - 1 (first >= 0, 0 <= n <= 65536)
 * of every problem through the SAME kernels, with no stopping rule and no use of max_iteration or confidence.  Per
 * problem b and trial q, at [b n + q]: samples (8 int32, the first ransac_n used, the rest -1), flags (one byte: bit 0
 * the edge-length test passed or is off, bit 1 the distance test passed or is off, bit 2 scored = both; a trial that
 * fails the edge-length test is not estimated: T = identity, bits 1 and 2 clear), T (16 doubles), count and sum_d2 (0
 * where not scored).  A problem with ncorr < ransac_n draws nothing: samples -1, flags 0.  Any output may be NULL. */
TEASER_HIP_API int32_t teaser_hip_ransac_trials_batch(
    teaser_hip_ransac* ransac, int32_t batch, const double* const* src, const int32_t* n_src,
    const double* const* dst, const int32_t* n_dst, const int32_t* const* corr, const int32_t* n_corr,
    const teaser_ransac_params_c* params, int64_t first, int32_t n, int32_t* samples, uint8_t* flags,
    double* transformations, int32_t* count, double* sum_d2);

/* Fast Global Registration on correspondences: Open3D's registration_fgr_based_on_correspondence (Zhou, Park, Koltun,
 * ECCV 2016; Open3D's FastGlobalRegistration.cpp from NormalizePointCloud on), batched, on its OWN handle.  Open3D is
 * RESTATED here, not run: what follows is the contract, and where it departs from Open3D it says so.  Everything is
 * FP64, nothing is fused, there are no floating-point atomics, and every summation order depends on the problem's own
 * sizes alone.
 * Per problem: source P (n_s x 3 doubles) and target Q (n_t x 3), xyz interleaved, both non-empty; ncorr >= 0 pairs
 * (i, j) int32, used in the caller's order, repeats allowed; the options of teaser_fgr_params_c.
 *   block order of a sum over n items (points of a cloud, or pairs): the items are cut into blocks of 256 consecutive
 *            items, the last one padded with +0.0 terms.  Inside a block item k sits in lane k mod 64 of wave k div 64;
 *            the 64 lanes of a wave are combined by v <- v + v[lane xor o] for o = 32, 16, 8, 4, 2, 1 (every lane ends
 *            with the same value), and the four waves as (w0 + w1) + (w2 + w3): the block's partial.  The partials of
 *            the ceil(n / 256) blocks are combined by 256 accumulators, accumulator t = ((0.0 + partial[t]) +
 *            partial[t + 256]) + ... in ascending block index, and the 256 accumulators by the same rule as the 256
 *            items of a block.
 *   normalise (Open3D's NormalizePointCloud): mu_P, mu_Q = the coordinate sums over ALL points of each cloud in the
 *            block order, divided by n; scale = the largest sqrt((dx dx + dy dy) + dz dz) of any centred point
 *            (dx = x - mu.x ...) of either cloud.  use_absolute_scale: scale_global = 1, scale_start = scale; otherwise
 *            scale_global = scale, scale_start = 1.  Records per pair c: p~_c = (P[i_c] - mu_P) / scale_global,
 *            q_c = (Q[j_c] - mu_Q) / scale_global, one subtraction and one correctly rounded division per coordinate.
 *            scale = 0 (both clouds a single repeated point whose mean is that point): the records are 0, the
 *            optimisation is skipped and flag bit 1 is set.
 *   optimise (Open3D's OptimizePairwiseRegistration; the TARGET side moves, as in Open3D): trans = I, mu = scale_start.
 *            ncorr < 10: Open3D's rule, no iterations, flag bit 0.  Otherwise for itr = 0 .. iteration_number - 1, per
 *            pair with p = p~_c, q = q_c:
 *              e = p - q;  t = mu / (((e0 e0 + e1 e1) + e2 e2) + mu);  s = t t
 *              rows J0 = (0, -q2, q1, -1, 0, 0), J1 = (q2, 0, -q0, 0, -1, 0), J2 = (-q1, q0, 0, 0, 0, -1), residuals e0 e1 e2
 *              the pair's term of A = s (J0 J0^T + J1 J1^T + J2 J2^T), upper triangle by rows:
 *                A00 = s (q2 q2 + q1 q1)  A01 = s (0 - q1 q0)  A02 = s (0 - q2 q0)  A03 = 0  A04 = s (0 - q2)  A05 = s q1
 *                A11 = s (q2 q2 + q0 q0)  A12 = s (0 - q2 q1)  A13 = s q2  A14 = 0  A15 = s (0 - q0)
 *                A22 = s (q1 q1 + q0 q0)  A23 = s (0 - q1)  A24 = s q0  A25 = 0
 *                A33 = s  A34 = 0  A35 = 0  A44 = s  A45 = 0  A55 = s
 *              and of g = s (e0 J0 + e1 J1 + e2 J2):
 *                g0 = s (e1 q2 - e2 q1)  g1 = s (e2 q0 - e0 q2)  g2 = s (e0 q1 - e1 q0)
 *                g3 = s (0 - e0)  g4 = s (0 - e1)  g5 = s (0 - e2)
 *            A and g = the 27 sums over the pairs in the block order.  Solve A xi = -g by the unpivoted LDL^T of
 *            point-to-plane ICP (above: the same recurrences); delta = [Rz(xi2) Ry(xi1) Rx(xi0) | xi3 xi4 xi5] with
 *            the entries of R written as the ICP contract's.  If a pivot is not finite or not positive, or xi is not
 *            finite, delta = I and failed_solves counts the step; the ICP contract's wording on pivots that are zero
 *            only up to rounding applies.  trans = delta trans (row r, column c: ((d_r0 t_0c + d_r1 t_1c) + d_r2 t_2c)
 *            + d_r3 t_3c); every record moves in place, q <- apply(delta, q) of the ICP contract (Open3D also moves
 *            its copy step by step).  Then, if decrease_mu and itr % 4 == 0 and mu > maximum_correspondence_distance:
 *            mu = mu / division_factor.  Open3D's quirk is kept: with use_absolute_scale = 0 this compares a distance
 *            given in the caller's units with mu in NORMALISED units.
 *   back to the caller's frame (Open3D's GetTransformationOriginalScale, then the inverse): with trans = [R | t],
 *            t_M = ((t scale_global) - ((R_r0 muQ_0 + R_r1 muQ_1) + R_r2 muQ_2)) + muP_r per row r, M = [R | t_M] maps
 *            target to source, and the result T = [R^T | 0 - ((R_0r tM_0 + R_1r tM_1) + R_2r tM_2)] maps source to
 *            target.  DEPARTURE: Open3D calls a general 4 x 4 inverse; this takes the rigid inverse.  ncorr < 10,
 *            iteration_number = 0 and scale = 0 therefore give the centroid alignment [I | mu_Q - mu_P], not the
 *            identity.
 * Output per problem: transformation (T), optimised (trans), scale_global, scale_start, final_mu, iterations,
 * n_corr, failed_solves, flags (bit 0: ncorr < 10, bit 1: scale = 0).  The result is a function of the inputs alone:
 * not of the batch around the problem, not of the route ("resident_max_corr" below), and the same bits run to run.
 * maximum_tuple_count, tuple_scale and the tuple test itself belong to the front-ends (teaser_hip_features_tuple_test_batch).
 * TEASER_HIP_ERR_BAD_ARG (teaser_hip_fgr_last_error names the argument and the problem), found on the host before
 * anything is launched or written: an empty cloud, non-finite points, an index outside its cloud, division_factor not
 * finite or <= 1, maximum_correspondence_distance not finite or <= 0, iteration_number outside 0 .. 1024, a switch
 * that is not 0 or 1, NULL where a count is positive. */
typedef struct teaser_fgr_params_c {
  double division_factor;                 /* 1.4 */
  double maximum_correspondence_distance; /* 0.025 */
  int32_t use_absolute_scale;             /* 0 */
  int32_t decrease_mu;                    /* 1 */
  int32_t iteration_number;               /* 64 */
  int32_t reserved;
} teaser_fgr_params_c;
typedef struct teaser_fgr_result_c {
  double transformation[16]; /* row-major 4 x 4, source -> target */
  double optimised[16];      /* trans: moves the normalised target records */
  double scale_global;
  double scale_start;
  double final_mu;
  int32_t iterations;
  int32_t n_corr;
  int32_t failed_solves;
  int32_t flags;
} teaser_fgr_result_c;
typedef struct teaser_hip_fgr teaser_hip_fgr;
/* device < 0: the current HIP device.  TEASER_HIP_ERR_NO_DEVICE without a GPU: there is no CPU path. */
TEASER_HIP_API int32_t teaser_hip_fgr_create(int32_t device, teaser_hip_fgr** out);
TEASER_HIP_API int32_t teaser_hip_fgr_destroy(teaser_hip_fgr* fgr);
TEASER_HIP_API const char* teaser_hip_fgr_last_error(const teaser_hip_fgr* fgr);
/* DIAGNOSTIC: fills the handle's scratch and staging buffers with `byte`; see teaser_hip_icp_fill_scratch. */
TEASER_HIP_API int32_t teaser_hip_fgr_fill_scratch(teaser_hip_fgr* fgr, int32_t byte, int64_t* bytes_out);
/* The defaults noted beside the fields above (Open3D's FastGlobalRegistrationOption). */
TEASER_HIP_API int32_t teaser_hip_fgr_params_default(teaser_fgr_params_c* params);
/* `batch` independent problems, HOST pointers per problem, borrowed for the call: src[b] n_src[b] x 3, dst[b]
 * n_dst[b] x 3, corr[b] n_corr[b] x 2 int32 (source index, target index); params and out: one per problem.  One
 * upload, one download and one synchronisation per call, whatever the batch.
 * A batch holds at most 65535 problems (the grids carry the problem in blockIdx.y or blockIdx.z): more, in this call
 * or the stage call below, is refused with
 * TEASER_HIP_ERR_UNSUPPORTED before anything is allocated or copied, and the handle stays usable. */
TEASER_HIP_API int32_t teaser_hip_fgr_correspondence_batch(
    teaser_hip_fgr* fgr, int32_t batch, const double* const* src, const int32_t* n_src, const double* const* dst,
    const int32_t* n_dst, const int32_t* const* corr, const int32_t* n_corr, const teaser_fgr_params_c* params,
    teaser_fgr_result_c* out);
/* One problem: teaser_hip_fgr_correspondence_batch with batch = 1. */
TEASER_HIP_API int32_t teaser_hip_fgr_correspondence(teaser_hip_fgr* fgr, const double* src, int32_t n_src,
                                                     const double* dst, int32_t n_dst, const int32_t* corr,
                                                     int32_t n_corr, const teaser_fgr_params_c* params,
                                                     teaser_fgr_result_c* out);
/* One knob per handle, "resident_max_corr" in [0, 3072] (default 256): a problem with at most that many pairs is
 * solved by ONE launch that keeps its records (48 bytes a pair, whole blocks of 256) in LDS; a larger one streams its
 * records from device memory, two launches an iteration.  0 forces the streamed route.  The bound is 12 blocks =
 * 147 456 bytes, what fits the 160 KB of LDS a workgroup may own beside the sums; the default is 1 block = 12 KB: a
 * resident problem's one workgroup walks its blocks in turn, and from a few blocks up the streamed route, which spreads
 * them over the device, was measured faster.  A tuning switch: no value changes a bit of any result.  BAD_ARG for
 * another name or a value out of range. */
TEASER_HIP_API int32_t teaser_hip_fgr_set_option(teaser_hip_fgr* fgr, const char* name, int64_t value);
TEASER_HIP_API int32_t teaser_hip_fgr_get_option(const teaser_hip_fgr* fgr, const char* name, int64_t* value);
/* Stage call: the first n iterations (0 <= n <= iteration_number of every problem) through the SAME kernels and
 * routes.  Per problem b and iteration k, at [b n + k]: mu (the value the step used), A (36, row-major, mirrored),
 * g (6), xi (6; zeros when a pivot failed), solve_flag (1: the solve failed and delta = I) and trans (16) after the
 * step; a problem that is not optimised (ncorr < 10, scale = 0) leaves zeros.  p_records / q_records: p~ and the moved
 * records q AFTER the n-th step, 3 doubles a pair, the problems' pairs one after the other in batch order.  out as in
 * the full call, with transformation taken from trans after n steps.  Any output may be NULL. */
TEASER_HIP_API int32_t teaser_hip_fgr_iterations_batch(
    teaser_hip_fgr* fgr, int32_t batch, const double* const* src, const int32_t* n_src, const double* const* dst,
    const int32_t* n_dst, const int32_t* const* corr, const int32_t* n_corr, const teaser_fgr_params_c* params,
    int32_t n, teaser_fgr_result_c* out, double* mu, double* A, double* g, double* xi, int32_t* solve_flag,
    double* trans, double* p_records, double* q_records);

/* Plane segmentation: Open3D's PointCloud.segment_plane (RANSAC for the dominant plane), batched, on its OWN handle.
 * Open3D is RESTATED here, not run: what follows is the contract, and where it departs from Open3D it says so.
 * Everything is FP64, nothing is fused, there are no floating-point atomics, square roots and divisions are correctly
 * rounded, and every summation order is a function of the problem's own n alone.
 * Per problem: the cloud P (n x 3 doubles, xyz interleaved); distance_threshold d, finite and > 0; ransac_n in 3 .. 8;
 * num_iterations (int32 >= 0); probability in (0, 1]; a uint64 seed (0: from the clock, time(NULL) read once per call
 * and used for every problem whose seed is 0, as in the RANSAC contract).
 *   trial i (int64, from 0): its samples are c_k = z(seed, ransac_n i + k + 1) mod n for k = 0 .. ransac_n - 1, z the
 *            splitmix64 finaliser of the tuple-test and RANSAC contracts (wrapping 64-bit arithmetic, the exact 64-bit
 *            remainder).  Sampling is WITH replacement.  DEPARTURE: Open3D samples without replacement from its own
 *            generator; here a repeated index simply gives a degenerate (ransac_n = 3) or a less spread trial.
 *   normalise(abc, anchor): len = sqrt((a a + b b) + c c).  If len is zero or not finite (inf, NaN) the result is the
 *            ZERO plane (0, 0, 0, 0).  Otherwise a, b, c are each divided by len (three divisions),
 *            s = (a anchor.x + b anchor.y) + c anchor.z and the plane is (a, b, c, -s).
 *   model, ransac_n = 3: p0, p1, p2 = the samples; e0 = p1 - p0, e1 = p2 - p0; abc = e0 x e1, each component
 *            u v - w x as two products and one subtraction: (e0.y e1.z - e0.z e1.y, e0.z e1.x - e0.x e1.z,
 *            e0.x e1.y - e0.y e1.x); the plane is normalise(abc, p0).
 *   model, ransac_n > 3: plane_from_points over the samples in sample order, every sum sequential from 0.0.
 *   A trial whose model is the zero plane is DEGENERATE.
 *   plane_from_points(S): Open3D's GetPlaneFromPoints, the determinant-based fast fit -- NOT a total-least-squares
 *            plane.  m = |S|; centroid = the three coordinate sums, each divided by (double) m; with r = p - centroid
 *            the six sums xx, xy, xz, yy, yz, zz of the products of r's components; det_x = yy zz - yz yz,
 *            det_y = xx zz - xz xz, det_z = xx yy - xy xy.  The axis is x, unless det_y > det_x: then y; and z if det_z
 *            exceeds the larger of the two (on a tie the first of x, y, z wins).
 *              x: abc = (det_x, xz yz - xy zz, xy yz - xz yy)
 *              y: abc = (xz yz - xy zz, det_y, xy xz - yz xx)
 *              z: abc = (xy yz - xz yy, xy xz - yz xx, det_z)
 *            The result is normalise(abc, centroid).
 *   position order of a sum over the n positions of the cloud: the positions are cut into blocks of 256 consecutive
 *            indices; a block's terms are added in ascending index starting from 0.0; the blocks are cut into groups of
 *            64 consecutive blocks and a group's block sums are added in ascending order from 0.0; the group sums are
 *            added in ascending order from 0.0.  A position that contributes nothing adds nothing (it is skipped, not
 *            added as 0.0).  DEPARTURE: Open3D adds in plain index order.
 *   score    of a trial that is not degenerate, over ALL n points: dist = |((a x + b y) + c z) + d4|; a point is an
 *            inlier iff dist < d; count = the number of inliers; E = the sum of dist over the inliers in position
 *            order; fitness = count / n; inlier_rmse = E / sqrt(count), 0 when count = 0 (Open3D's expression, kept
 *            although it sums distances and not squares: it only breaks ties).
 *   loop     Open3D's, as ONE thread runs it: best = {zero plane, count 0, rmse 0}, k = +inf (a double), counted = 0;
 *            for i = 0 .. num_iterations - 1: stop when counted > k; a degenerate trial is skipped and not counted; a
 *            trial replaces best iff count > best.count, or count == best.count and rmse < best.rmse (strict: earlier
 *            trials keep ties); on a replacement k = 0 when count == n, otherwise
 *            k = min(log(1 - probability) / log(1 - pow(fitness, ransac_n)), num_iterations) in host double with the C
 *            library's log and pow, min(a, b) = a < b ? a : b with the quotient first; then counted += 1 for every
 *            trial that is not degenerate.  DEPARTURE: k stays a double; this equals Open3D's truncated size_t
 *            wherever that conversion is defined; a negative or -inf k stops at once (a fitness so small that
 *            1 - pow(..) rounds to 1 gives log(..) = 0 and k = -inf, whatever the probability), a NaN k (min gives
 *            num_iterations) never stops early, and neither does probability = 1 otherwise (k = +inf, capped).
 *   finish   No trial replaced the start: the zero plane, no inliers.  Otherwise the inliers are the indices with
 *            dist < d under the WINNING TRIAL's plane, ascending, and the returned plane is plane_from_points over
 *            those inliers with all nine sums in position order (m > 0 always holds here).  As in Open3D the inliers
 *            are those of the trial's plane, not of the refit; a refit that gives the zero plane is returned as such
 *            with the inliers kept.
 * Output per problem: plane[4], n_inliers, fitness and inlier_rmse of the winning trial, best_trial (-1: none),
 * trials = the loop indices visited, valid_trials = those of them that were not degenerate, and optionally the inlier
 * indices (int32, ascending, room for n) and / or a byte mask of n entries.  The result is a function of the inputs
 * alone: not of "chunk_trials" or "partial_bytes" below, not of the batch around the problem, and the same bits run to
 * run.  Work past the stopping trial is discarded, never reported.  n < ransac_n or num_iterations = 0 is not an
 * error: the result is the start (zero plane, zeros, best_trial = -1, trials = 0).
 * TEASER_HIP_ERR_BAD_ARG (teaser_hip_plane_last_error names the argument and the problem), found on the host before
 * anything is launched or written: non-finite points, d not finite and > 0, ransac_n outside 3 .. 8, probability
 * outside (0, 1] or NaN, a negative num_iterations, a negative n, NULL where a count is positive.  The handle stays
 * usable after a refusal. */
typedef struct teaser_plane_params_c {
  double distance_threshold; /* d; no default (Open3D's argument is required) */
  int32_t ransac_n;          /* 3 */
  int32_t num_iterations;    /* 100 */
  double probability;        /* 0.99999999 */
  uint64_t seed;             /* 0: from the clock */
} teaser_plane_params_c;
typedef struct teaser_plane_result_c {
  double plane[4]; /* a, b, c, d4: a x + b y + c z + d4 = 0 */
  double fitness;
  double inlier_rmse;
  int64_t best_trial;
  int64_t trials;
  int64_t valid_trials;
  int32_t n_inliers;
  int32_t reserved;
} teaser_plane_result_c;
typedef struct teaser_hip_plane teaser_hip_plane;
/* device < 0: the current HIP device.  TEASER_HIP_ERR_NO_DEVICE without a GPU: there is no CPU path. */
TEASER_HIP_API int32_t teaser_hip_plane_create(int32_t device, teaser_hip_plane** out);
TEASER_HIP_API int32_t teaser_hip_plane_destroy(teaser_hip_plane* plane);
TEASER_HIP_API const char* teaser_hip_plane_last_error(const teaser_hip_plane* plane);
/* DIAGNOSTIC: fills the handle's scratch and staging buffers with `byte`; see teaser_hip_icp_fill_scratch. */
TEASER_HIP_API int32_t teaser_hip_plane_fill_scratch(teaser_hip_plane* plane, int32_t byte, int64_t* bytes_out);
/* The defaults noted beside the fields above (Open3D's segment_plane). */
TEASER_HIP_API int32_t teaser_hip_plane_params_default(teaser_plane_params_c* params);
/* `batch` independent problems, HOST pointers per problem, borrowed for the call: points[b] n[b] x 3; params and out:
 * one per problem; inliers: NULL, or per problem NULL or room for n[b] int32, out[b].n_inliers written; mask: NULL, or
 * per problem NULL or n[b] bytes (1: inlier).  Mixed sizes share the launches; batch = 0 and n[b] = 0 are valid.
 * A batch holds at most 65535 problems (the grids carry the problem in blockIdx.y or blockIdx.z): more, in this call
 * or the stage call below, is refused with
 * TEASER_HIP_ERR_UNSUPPORTED before anything is allocated or copied, and the handle stays usable. */
TEASER_HIP_API int32_t teaser_hip_plane_segment_batch(teaser_hip_plane* plane, int32_t batch,
                                                      const double* const* points, const int32_t* n,
                                                      const teaser_plane_params_c* params, teaser_plane_result_c* out,
                                                      int32_t* const* inliers, uint8_t* const* mask);
/* One problem: teaser_hip_plane_segment_batch with batch = 1. */
TEASER_HIP_API int32_t teaser_hip_plane_segment(teaser_hip_plane* plane, const double* points, int32_t n,
                                                const teaser_plane_params_c* params, teaser_plane_result_c* out,
                                                int32_t* inliers, uint8_t* mask);
/* Two knobs per handle, both tuning switches: no value changes a bit of any result.  "chunk_trials" in [64, 4096]
 * (default 256): the trials of a problem one launch sequence covers.  "partial_bytes" in [65536, 17179869184] (default
 * 67108864): the budget of the (block, trial) partial array; a cloud whose partials exceed it is scored in waves of
 * groups of blocks (one group per problem is the floor).  BAD_ARG for another name or a value out of range. */
TEASER_HIP_API int32_t teaser_hip_plane_set_option(teaser_hip_plane* plane, const char* name, int64_t value);
TEASER_HIP_API int32_t teaser_hip_plane_get_option(const teaser_hip_plane* plane, const char* name, int64_t* value);
/* Stage call: trials first .. first + cnt - 1 (first >= 0, 0 <= cnt <= 65536) of every problem through the SAME
 * kernels, with no stopping rule and no use of num_iterations or probability.  Per problem b and trial q, at
 * [b cnt + q]: samples (8 int32, the first ransac_n used, the rest -1), flags (one byte: bit 0 = not degenerate),
 * planes (4 doubles, zero when degenerate), count and E (0 when degenerate).  A problem with n < ransac_n draws
 * nothing: samples -1, flags 0.  Any output may be NULL. */
TEASER_HIP_API int32_t teaser_hip_plane_trials_batch(teaser_hip_plane* plane, int32_t batch,
                                                     const double* const* points, const int32_t* n,
                                                     const teaser_plane_params_c* params, int64_t first, int32_t cnt,
                                                     int32_t* samples, uint8_t* flags, double* planes, int32_t* count,
                                                     double* E);

/* TSDF volume: Open3D's pipelines.integration.UniformTSDFVolume (integrate, extract_point_cloud,
 * extract_voxel_point_cloud), on its OWN handle.  A handle owns ONE volume, which lives on the device from create to
 * destroy: frames go up, the extracted surface comes back, the voxels move only through download and upload.  The text
 * below IS the contract.  It restates Open3D's UniformTSDFVolume.cpp from memory; Open3D is not run and bit parity with
 * an Open3D binary is NOT claimed.  tests/tsdf_reference.py restates this text in numpy and is the parity target of the
 * host and GPU tests.  No product-add is fused and every sum is taken left to right as written; float32 divisions and
 * square roots are correctly rounded.
 *
 * State.  R = resolution.  Per voxel (x, y, z), 0 <= x, y, z < R: tsdf and weight, float32, both 0 after create and
 * reset; with a colour type, color: three doubles, 0.  vl = length / R in double.  The float32 constants:
 *   vl_f = (float)vl;  half_f = vl_f 0.5f;  trunc_f = (float)sdf_trunc;  inv_f = 1.0f / trunc_f;  o_f = (float)origin,
 *   and per frame E_f = (float)E element by element (E = extrinsic, the row-major 4 x 4 world-to-camera matrix, used as
 *   given; row 3 is not read);  s_r = E_f[r][2] vl_f;  fx_f, fy_f, cx_f, cy_f = (float) of the intrinsics;
 *   safe_w = (float)width - 0.0001f;  safe_h = (float)height - 0.0001f.
 *
 * Depth sample: the rule of "Depth frames".  A uint16 sample d gives (float)d / (float)depth_scale, set to 0 when
 * (double) of it is >= depth_trunc; a float32 sample is taken as it is.
 *
 * teaser_hip_tsdf_integrate_batch: the frames apply in the order given, and a voxel's result equals applying them one
 * call at a time.  All arithmetic is float32 unless stated.  For each column (x, y):
 *   p   = ((half_f + vl_f (float)x) + o_f[0], (half_f + vl_f (float)y) + o_f[1], half_f + o_f[2])
 *   c_r = ((E_f[r][0] p_x + E_f[r][1] p_y) + E_f[r][2] p_z) + E_f[r][3]   for r = 0, 1, 2
 *   voxel z uses c after z successive additions c_r = c_r + s_r.  This is Open3D's running sum; it is part of the bits
 *   and is never replaced by a product.
 * Then for each voxel:
 *   skip unless c_2 > 0
 *   u_f = ((c_0 fx_f) / c_2 + cx_f) + 0.5f;  v_f = ((c_1 fy_f) / c_2 + cy_f) + 0.5f
 *   skip unless u_f >= 0.0001f && u_f < safe_w && v_f >= 0.0001f && v_f < safe_h   (a NaN skips)
 *   u = (int)u_f, v = (int)v_f;  d = the depth sample of row v, column u;  skip unless d > 0   (a NaN skips; +inf does not)
 *   xx = ((float)u - cx_f) (1.0f / fx_f);  yy = ((float)v - cy_f) (1.0f / fy_f);  m = sqrtf((xx xx + yy yy) + 1.0f)
 *   sdf = (d - c_2) m;  skip unless sdf > -trunc_f
 *   q = sdf inv_f;  t = q < 1.0f ? q : 1.0f
 *   tsdf = (tsdf weight + t) / (weight + 1.0f)
 *   with colour, per component in double: color = (color (double)weight + (double)s) / (double)(weight + 1.0f), s the
 *   uint8 channel of pixel (v, u) for RGB8, or its float32 sample for all three components for Gray32 (a NaN colour of
 *   a Gray32 volume is stored as the quiet NaN 0x7ff8000000000000)
 *   last: weight = weight + 1.0f
 * Per frame one record teaser_tsdf_frame_c, a depth image depth[b] (height rows of depth_row_bytes bytes) and, for a
 * volume with a colour type, a colour image color[b] (height rows of color_row_bytes bytes): RGB8 needs color_format 1
 * (uint8 x 3), Gray32 color_format 2 (float32 x 1).  A volume without colour reads no colour image: color may be NULL and
 * color_format only has to lie in [0, 3].  Rows may be padded.  A frame with width or height 0 is legal and touches
 * nothing; n_frames = 0 returns OK without touching the device.
 *
 * teaser_hip_tsdf_extract_point_cloud.  A voxel is USABLE when weight != 0 && tsdf < 0.98f && tsdf >= -0.98f.  The rows
 * come in the order of Open3D's serial loop: x, y, z ascending and inside a voxel the axes i = 0, 1, 2.  For a usable
 * voxel 0 = (x, y, z) with value f0 and its +1 neighbour 1 along axis i with value f1, a row is emitted when the
 * neighbour's index along i is < R - 1, the neighbour is usable and f0 f1 < 0 (float32).  Then
 *   r0 = |f0|, r1 = |f1| in float32;  half = vl 0.5 and p0 = (half + vl x, half + vl y, half + vl z) in double
 *   p = p0 except p_i = (p0_i (double)r1 + (p0_i + vl) (double)r0) / (double)(r0 + r1);  the point is p + origin
 *   colour: (c0 (double)r1 + c1 (double)r0) / (double)(r0 + r1) per component, then / 255.0 for RGB8 only
 *   normal, in double: g = 0.99 vl;  n_k = T(p + g e_k) - T(p - g e_k) with p in volume coordinates (without the
 *   origin);  T(q): a = q / vl - 0.5 per component, idx = floor(a), r = a - idx;  the value is the eight-corner sum in
 *   the order 000, 001, 010, 011, 100, 101, 110, 111 of the offsets (x y z), each term
 *   ((wx wy) wz) (double)tsdf(idx + offset) with w = r for offset 1 and 1.0 - r for offset 0, the first term starting
 *   the sum.  A corner outside the volume has tsdf 0 (DEPARTURE: Open3D reads out of bounds there).  Then
 *   s = (n_0 n_0 + n_1 n_1) + n_2 n_2 and n = n / sqrt(s) (three divisions) if s > 0.
 * teaser_hip_tsdf_extract_voxel_point_cloud: every usable voxel in x, y, z order: the point
 * ((half + vl x) + origin_x, ...), the colour ((double)tsdf + 1.0) 0.5 three times.
 * Both: count_out (required) receives the number of rows.  capacity = 0 with points NULL returns the count alone.
 * Otherwise points has room for capacity x 3 doubles and normals, colors are NULL or as large (colors of the surface
 * only for a volume with a colour type).  A capacity below the count is TEASER_HIP_ERR_BAD_ARG: the message names the
 * count, count_out holds it, and no row is written.  Rows behind the count are not written.
 *
 * teaser_hip_tsdf_extract_triangle_mesh: Open3D's UniformTSDFVolume::ExtractTriangleMesh (marching cubes), vertices and
 * triangles in the order of Open3D's serial loop with its hash map.  tests/tsdf_mesh_reference.py restates it as that
 * loop and is the parity target.
 *   Cubes.  Cube (x, y, z) exists for 0 <= x, y, z < R - 1 (R = 1 has none).  Corner i lies at (x, y, z) + shift[i]:
 *   shift = (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1).  Edge i is the lattice edge with base voxel
 *   (x, y, z) + the first three of edge_shift[i] along the axis that is its fourth: edge_shift = (0,0,0,0) (1,0,0,1)
 *   (0,1,0,0) (0,0,0,1) (0,0,1,0) (1,0,1,1) (0,1,1,0) (0,0,1,1) (0,0,0,2) (1,0,0,2) (1,1,0,2) (0,1,0,2).  Its corners are
 *   edge_to_vert[i] = {0,1} {1,2} {3,2} {0,3} {4,5} {5,6} {7,6} {4,7} {0,4} {1,5} {2,6} {3,7}, the base voxel first.
 *   ACTIVE.  cube_index has bit i set when tsdf(corner i) < 0.0f.  A cube is ACTIVE when all eight corner weights are
 *   != 0 and cube_index is neither 0 nor 255 (no 0.98 test here, unlike the point cloud).
 *   Tables.  edge_table[256] (bit i: the corners of edge i differ in sign) and tri_table[256][16] (edge numbers, -1
 *   terminated, at most five triangles) are Paul Bourke's public-domain "polygonise" tables, written out from memory
 *   and checked by property (tests/test_tsdf_mesh_reference.py).  The table as written is part of the contract: the
 *   SHA-256 of tri_table as 4096 int8, row-major, is
 *   19bf7699e214903d72c94c296546f2e31337d637a1e4b118c3108a0f428e809b.  teaser_hip_tsdf_mesh_tables hands both out
 *   (host only, no device needed).
 *   Vertices.  A lattice edge carries a vertex when its end voxels differ in sign (tsdf < 0.0f) and at least one of the
 *   up to four cubes that contain it is ACTIVE.  Its CREATOR is the smallest such ACTIVE cube, compared as (x, y, z),
 *   its slot the edge's number i inside the creator.  Vertices are numbered in ascending (creator's (x R + y) R + z,
 *   slot): the order in which Open3D's loop first meets them.  With a, b = edge_to_vert[slot] in the creator, all in
 *   double: f0 = |(double)tsdf(a)|, f1 = |(double)tsdf(b)|;  p = (half + vl bx, half + vl by, half + vl bz) for the
 *   base voxel (bx, by, bz);  p_axis = p_axis + (f0 vl) / (f0 + f1);  the vertex is p + origin.  Colour (a volume with a
 *   colour type): c0, c1 the end voxels' colours, each / 255.0 first for RGB8; (f1 c0 + f0 c1) / (f0 + f1) per
 *   component; a NaN colour of a Gray32 volume is the quiet NaN.  (This order of operations is not the point cloud's.)
 *   Triangles.  For every ACTIVE cube in ascending (x, y, z) and t = 0, 3, 6, ... until tri_table[cube_index][t] = -1
 *   one row (v[T[t]], v[T[t + 2]], v[T[t + 1]]) -- Open3D swaps the last two -- with v[e] the index of the vertex on the
 *   cube's edge e, int32.  Coincident vertices (a corner value of exactly 0) keep distinct indices; degenerate triangles
 *   are kept.
 *   Vertex normals (an EXTENSION: Open3D's mesh has none until compute_vertex_normals(), and this is not what that
 *   computes): when vertex_normals is given, the normal rule of the point cloud above evaluated at p (volume
 *   coordinates, before the origin is added): the same T, g = 0.99 vl, zero outside the volume, the same normalisation.
 *   The call.  vertex_count_out and triangle_count_out (both required) receive the counts.  Both capacities 0 with
 *   vertices and triangles NULL returns the counts alone.  Otherwise vertices has room for vertex_capacity x 3 doubles,
 *   vertex_colors (only for a volume with a colour type) and vertex_normals are NULL or as large, triangles has room for
 *   triangle_capacity x 3 int32.  A capacity below its count is TEASER_HIP_ERR_BAD_ARG: the message names both counts,
 *   both outputs hold them, and no row of either array is written.  Rows behind the counts are not written.  A vertex
 *   count above 2^31 - 1 is TEASER_HIP_ERR_BAD_ARG with the count in the message.  Scratch: 5 bytes per voxel (a byte
 *   and a 32-bit record per cube) plus 24 bytes per column, allocated by the first call and kept on the handle; a
 *   failed allocation is TEASER_HIP_ERR_OOM and leaves the volume intact.  Three launches for the counts and one
 *   more for each array with a capacity above 0; no floating-point atomic, the same bits run after run.
 *
 * teaser_hip_tsdf_download / _upload: tsdf_weight is R^3 x 2 float32 (tsdf, weight), color R^3 x 3 doubles (only for a
 * volume with a colour type), both in Open3D's voxel order (x R + y) R + z whatever the device layout is; either may be
 * NULL, not both.  upload refuses values that are not finite, except a NaN colour of a Gray32 volume, which is stored
 * as the quiet NaN.
 *
 * TEASER_HIP_ERR_BAD_ARG (the argument and the frame are named; the handle stays usable; create has no handle yet, so
 * teaser_hip_tsdf_last_error(NULL) returns the calling thread's last create message): resolution outside [1, 1024];
 * length or sdf_trunc not finite or <= 0; origin not finite; color_type outside {0, 1, 2}; reserved != 0; per frame
 * width or height negative or above 16384, fx or fy zero or not finite, cx, cy, the extrinsic, depth_scale or
 * depth_trunc not finite, depth_scale <= 0, depth_format outside {0, 1}, color_format outside [0, 3] or not the one the
 * volume's colour type needs, row bytes below a row's size; NULL where something is required; a capacity below the
 * count.  An allocation failure is TEASER_HIP_ERR_OOM.  Every call is deterministic: the same bits run after run, for
 * any split of the frames into calls.  One stream synchronisation per call; the number of launches does not depend on
 * the data. */
typedef struct teaser_tsdf_volume_c {
  double length;      /* the cube's side; default 4.0 */
  double sdf_trunc;   /* default 0.04 */
  double origin[3];   /* the corner of voxel (0, 0, 0); default 0 */
  int32_t resolution; /* R; default 512 */
  int32_t color_type; /* 0 none (default), 1 RGB8, 2 Gray32 */
  int64_t reserved;   /* must be 0 */
} teaser_tsdf_volume_c;
typedef struct teaser_tsdf_frame_c {
  int32_t width, height;
  int32_t depth_format;    /* 0 uint16, 1 float32 */
  int32_t color_format;    /* 0 none, 1 uint8 x 3 (RGB), 2 float32 x 1, 3 float32 x 3 */
  int64_t depth_row_bytes; /* bytes from one row of the depth image to the next */
  int64_t color_row_bytes; /* likewise for the colour image; not read by a volume without colour */
  double fx, fy, cx, cy;
  double extrinsic[16];    /* row-major, world to camera */
  double depth_scale;
  double depth_trunc;
} teaser_tsdf_frame_c;
#ifdef __cplusplus
static_assert(sizeof(teaser_tsdf_volume_c) == 56, "teaser_tsdf_volume_c is 56 bytes");
static_assert(sizeof(teaser_tsdf_frame_c) == 208, "teaser_tsdf_frame_c is 208 bytes");
#else
_Static_assert(sizeof(teaser_tsdf_volume_c) == 56, "teaser_tsdf_volume_c is 56 bytes");
_Static_assert(sizeof(teaser_tsdf_frame_c) == 208, "teaser_tsdf_frame_c is 208 bytes");
#endif
typedef struct teaser_hip_tsdf teaser_hip_tsdf;
/* The defaults noted beside the fields above. */
TEASER_HIP_API int32_t teaser_hip_tsdf_volume_default(teaser_tsdf_volume_c* volume);
/* device < 0: the current HIP device.  The record is checked first; then TEASER_HIP_ERR_NO_DEVICE without a GPU: there
 * is no CPU path.  The volume is allocated (8 bytes per voxel, 32 with a colour type) and zeroed here. */
TEASER_HIP_API int32_t teaser_hip_tsdf_create(const teaser_tsdf_volume_c* volume, int32_t device, teaser_hip_tsdf** out);
TEASER_HIP_API int32_t teaser_hip_tsdf_destroy(teaser_hip_tsdf* tsdf);
TEASER_HIP_API const char* teaser_hip_tsdf_last_error(const teaser_hip_tsdf* tsdf);
/* DIAGNOSTIC: fills the handle's scratch and staging buffers with `byte`; see teaser_hip_icp_fill_scratch. */
TEASER_HIP_API int32_t teaser_hip_tsdf_fill_scratch(teaser_hip_tsdf* tsdf, int32_t byte, int64_t* bytes_out);
/* Every voxel back to the state after create. */
TEASER_HIP_API int32_t teaser_hip_tsdf_reset(teaser_hip_tsdf* tsdf);
TEASER_HIP_API int32_t teaser_hip_tsdf_integrate_batch(teaser_hip_tsdf* tsdf, int32_t n_frames,
                                                       const teaser_tsdf_frame_c* frames, const void* const* depth,
                                                       const void* const* color);
TEASER_HIP_API int32_t teaser_hip_tsdf_extract_point_cloud(teaser_hip_tsdf* tsdf, int64_t capacity, double* points,
                                                           double* normals, double* colors, int64_t* count_out);
TEASER_HIP_API int32_t teaser_hip_tsdf_extract_voxel_point_cloud(teaser_hip_tsdf* tsdf, int64_t capacity, double* points,
                                                                 double* colors, int64_t* count_out);
TEASER_HIP_API int32_t teaser_hip_tsdf_download(teaser_hip_tsdf* tsdf, float* tsdf_weight, double* color);
TEASER_HIP_API int32_t teaser_hip_tsdf_upload(teaser_hip_tsdf* tsdf, const float* tsdf_weight, const double* color);
TEASER_HIP_API int32_t teaser_hip_tsdf_extract_triangle_mesh(teaser_hip_tsdf* tsdf, int64_t vertex_capacity,
                                                             double* vertices, double* vertex_colors,
                                                             double* vertex_normals, int64_t triangle_capacity,
                                                             int32_t* triangles, int64_t* vertex_count_out,
                                                             int64_t* triangle_count_out);
/* Host only: the marching-cubes tables of the call above, edge_table[256] and tri_table[256][16] row-major. */
TEASER_HIP_API int32_t teaser_hip_tsdf_mesh_tables(int32_t* edge_table, int8_t* tri_table);

/* TSDF ray casting: the volume of a TSDF handle rendered into cameras -- per pixel the z-depth, the world point, the
 * normal and the colour of the first surface a ray meets.  The semantics follow Open3D's
 * t.geometry.VoxelBlockGrid.ray_cast, restated for the dense volume; Open3D is not run and bit parity with an Open3D
 * binary is NOT claimed.  The text below IS the contract; tests/tsdf_raycast_reference.py restates it in numpy and is
 * the parity target of the host and GPU tests.  No product-add is fused, every sum is taken left to right as written,
 * every min and max is written as a comparison (so a NaN's path is stated), float32 divisions are correctly rounded.
 *
 * The view.  One record teaser_tsdf_view_c per view; E = extrinsic, the row-major 4 x 4 world-to-camera matrix as in
 * integration.  On the host, in double: the camera-to-world rotation is the transpose of E's upper 3 x 3 and the centre
 *   c_k = -((E[0][k] E[0][3] + E[1][k] E[1][3]) + E[2][k] E[2][3]).
 * That is the inverse of a rigid E; a non-rigid extrinsic is NOT inverted (its rays are whatever these formulas give).
 * Per-view float32 constants:  o_f[k] = (float)(c_k - origin_k) (the centre in volume coordinates);
 *   Rt_f[k][j] = (float)E[j][k];  fx_f, fy_f, cx_f, cy_f, dmin_f, dmax_f, wthr_f = (float) of the view's fields;
 *   L_f = (float)length;  vl_f and trunc_f are those of "TSDF volume".
 *
 * The ray of pixel (v, u) (row v, column u), all float32:
 *   a = ((float)u - cx_f) / fx_f;  b = ((float)v - cy_f) / fy_f;  d_k = (Rt_f[k][0] a + Rt_f[k][1] b) + Rt_f[k][2].
 * The point at parameter t is o_f + t d, so t is the z-depth in the camera.
 *
 * The box clip.  t0 = dmin_f, t1 = dmax_f.  For each axis k = 0, 1, 2 in turn: with d_k != 0,
 *   lo = (0.0f - o_k) / d_k;  hi = (L_f - o_k) / d_k;  if (hi < lo) the two are exchanged;
 *   t0 = t0 < lo ? lo : t0;  t1 = hi < t1 ? hi : t1;
 * with d_k == 0 the pixel is a MISS unless o_k >= 0.0f && o_k < L_f.  The clip only saves steps: safety comes from the
 * sample rule below, which reads no voxel outside the volume whatever t is.
 *
 * The march.  t = t0, t_prev = t0, f_prev = -1.0f.  At most 2 R + 2 steps; a ray that has taken them all is a MISS.  (A
 * ray inside the box takes fewer than sqrt(3) R + 1, every step being at least vl_f long; the cap exists so that a
 * rounding t + step == t can never hang a device.)  Each step, in order:
 *   1. MISS unless t <= t1  (a NaN misses).
 *   2. p_k = o_k + t d_k;  q_k = floorf(p_k / vl_f).
 *   3. The sample is voxel ((int)q_0, (int)q_1, (int)q_2) when every q_k >= 0.0f && q_k < (float)R -- the float is tested
 *      before it is converted, so no conversion overflows; f = its tsdf, w = its weight.  Otherwise f = 0 and w = 0, as
 *      for an unobserved voxel.
 *   4. HIT when f_prev > 0.0f && w >= wthr_f && f <= 0.0f.
 *   5. Otherwise t_prev = t, f_prev = f;  delta = f trunc_f;  t = t + (delta < vl_f ? vl_f : delta).
 * Consequences: a camera that starts behind a surface sees nothing until its ray has passed an observed positive
 * voxel (f_prev starts negative), and a surface met from unobserved space (f_prev = 0) is not a hit.  With
 * weight_threshold <= 0 the space outside the volume (f = 0, w = 0) ends a ray that comes from a positive voxel.
 *
 * A hit.  t* = (t f_prev - t_prev f) / (f_prev - f) in float32;  depth = t*.  In double
 *   q_k = (double)o_k + (double)t* (double)d_k   (volume coordinates);  vertex_k = q_k + origin_k, rounded to float32.
 * NEAR: every q_k >= -(2.0 vl) && q_k <= vl (double)R + 2.0 vl (double; a NaN is not near).  A hit that is not near has
 * the normal and the colour 0: every corner the two rules below would read lies outside the volume, so this is their value, and
 * the test keeps an enormous q from being converted to an integer.  (It needs a camera so far from the volume that
 * float32 no longer resolves a voxel.)  Otherwise:
 *   normal: the normal rule of teaser_hip_tsdf_extract_point_cloud at q (the same T, g = 0.99 vl, zero outside the
 *   volume, the same normalisation), rounded to float32 -- so the point cloud, the mesh and the ray cast agree.
 *   colour (a volume with a colour type): with a = q / vl - 0.5, idx = floor(a), r = a - idx as in T, over the eight
 *   corners in T's order 000, 001, ..., 111 with T's weights omega = (wx wy) wz: a corner COUNTS when it lies inside the
 *   volume and its voxel weight is != 0.  Starting from num_c = 0.0 and den = 0.0, each counting corner adds
 *   num_c = num_c + omega color_c and den = den + omega.  The value is num_c / den when den > 0, else 0 (no corner
 *   counts, or only corners of omega 0); then / 255.0 for RGB8 only.  Rounded to float32; a NaN (a Gray32 volume) is
 *   stored as the quiet NaN 0x7fc00000.
 * A missed pixel is 0 in every output.
 *
 * teaser_hip_tsdf_ray_cast_views.  depth, vertex, normal and color are arrays of n_views host pointers; a whole array
 * or any single entry may be NULL when that map is not wanted.  depth[b] is height x width float32, the others
 * height x width x 3 float32, row-major and packed.  color is allowed only for a volume with a colour type.  hit_counts
 * (optional) receives per view the int64 number of hit pixels (summed in integers).  Views of any mix of sizes go into
 * one call: one launch covers all pixels of all views (blocks of 16 x 16 pixels and a block map), one stream
 * synchronisation per call, the maps come back through the handle's page-locked buffer and only the requested ones are
 * computed and copied.  A view with width or height 0 is legal; n_views = 0 returns OK without touching the device.
 * The call does not modify the volume, is stream-ordered after earlier integrations on the handle, uses no
 * floating-point atomic and gives the same bits run after run and for any grouping of the views into calls.
 * TEASER_HIP_ERR_BAD_ARG (the message names the view and the field; the handle stays usable): n_views negative; width
 * or height negative or above 16384; fx or fy zero or not finite; cx, cy or the extrinsic not finite; depth_min
 * negative; depth_min, depth_max or weight_threshold not finite; depth_max < depth_min; reserved != 0; color asked of a
 * volume without colour; a NULL handle or, with n_views > 0, NULL views; more than 2^31 - 1 blocks in one call. */
typedef struct teaser_tsdf_view_c {
  int32_t width, height;
  double fx, fy, cx, cy;
  double extrinsic[16];    /* row-major, world to camera */
  double depth_min;        /* default 0.1 */
  double depth_max;        /* default 3.0 */
  double weight_threshold; /* default 3.0 (Open3D's) */
  int64_t reserved;        /* must be 0 */
} teaser_tsdf_view_c;
#ifdef __cplusplus
static_assert(sizeof(teaser_tsdf_view_c) == 200, "teaser_tsdf_view_c is 200 bytes");
#else
_Static_assert(sizeof(teaser_tsdf_view_c) == 200, "teaser_tsdf_view_c is 200 bytes");
#endif
/* Zeroes the record, sets the defaults noted beside the fields and the identity extrinsic. */
TEASER_HIP_API int32_t teaser_hip_tsdf_view_default(teaser_tsdf_view_c* view);
TEASER_HIP_API int32_t teaser_hip_tsdf_ray_cast_views(teaser_hip_tsdf* tsdf, int32_t n_views,
                                                      const teaser_tsdf_view_c* views, float* const* depth,
                                                      float* const* vertex, float* const* normal, float* const* color,
                                                      int64_t* hit_counts);

/* Scalable TSDF volume: Open3D's pipelines.integration.ScalableTSDFVolume (integrate, extract_point_cloud,
 * extract_voxel_point_cloud), on its OWN handle.  Only the blocks of 16^3 voxels that depth frames have come near are
 * stored; the space needs no bounds.  The text below IS the contract.  It restates Open3D's ScalableTSDFVolume.cpp from
 * memory and fixes what Open3D leaves to an unordered map; Open3D is not run and bit parity with an Open3D binary is NOT
 * claimed.  Every deliberate difference is marked DEPARTURE.  tests/stsdf_reference.py restates this text in numpy and
 * is the parity target of the host and GPU tests.  No product-add is fused and every sum is taken left to right as
 * written.  Ray casting is "Scalable TSDF ray casting" below; extract_triangle_mesh is not offered in this section:
 * the mesh is "Scalable TSDF triangle mesh" below.
 *
 * Parameters.  voxel_length, sdf_trunc, color_type (0 none, 1 RGB8, 2 Gray32) as for "TSDF volume";
 * volume_unit_resolution U (default 16): this version supports ONLY 16 and refuses 4, 8 and 32 by name;
 * depth_sampling_stride (default 4).  vl = voxel_length and ul = vl U in double (exact).  sdf_trunc > ul is
 * TEASER_HIP_ERR_BAD_ARG (DEPARTURE: it bounds the blocks of a point to 4 an axis, 3 but for a rounding corner).
 *
 * Block.  Block (bx, by, bz), each index in [-2^20, 2^20), IS the dense volume of "TSDF volume" with length = ul,
 * resolution = U, origin = (bx ul, by ul, bz ul) (products in double): its voxels follow the integrate rule there word
 * for word with o_f = (float)(b ul), and start as zeros when the block is opened.
 *
 * Touch.  For frame k the points of "Depth frames" unprojection are taken with stride = depth_sampling_stride and
 * valid_only = 1, the depth sample by the rule of "TSDF volume" (uint16: scale and depth_trunc; float32 as it is), and
 * camera_pose M = the inverse of the frame's extrinsic E, formed on the host in double by this closed form (DEPARTURE:
 * Open3D calls Eigen's general inverse).  A = rows and columns 0 .. 2 of E, t = its column 3, row 3 is not read:
 *   c00 = A11 A22 - A12 A21;  c01 = A12 A20 - A10 A22;  c02 = A10 A21 - A11 A20
 *   c10 = A02 A21 - A01 A22;  c11 = A00 A22 - A02 A20;  c12 = A01 A20 - A00 A21
 *   c20 = A01 A12 - A02 A11;  c21 = A02 A10 - A00 A12;  c22 = A00 A11 - A01 A10
 *   det = (A00 c00 + A01 c01) + A02 c02;  M[r][c] = c_cr / det;  M[r][3] = -((M[r][0] t0 + M[r][1] t1) + M[r][2] t2)
 * A det of 0 or an M with an entry that is not finite is TEASER_HIP_ERR_BAD_ARG ("extrinsic is singular").  A point with a
 * component that is not finite touches nothing (DEPARTURE).  Per finite point p and axis a, in double:
 *   lo_a = floor((p_a - sdf_trunc) / ul);  hi_a = floor((p_a + sdf_trunc) / ul)
 * and frame k TOUCHES every block of [lo, hi]^3 whose three indices lie in [-2^20, 2^20).  Blocks outside that range are
 * never opened; out_of_range counts the (frame, point) pairs that have at least one such block.
 *
 * teaser_hip_stsdf_integrate_frames (the frames of ONE volume, any number of them: the counterpart of
 * teaser_hip_tsdf_integrate_batch).  The frames apply in the order given.  Frame k applies to exactly the blocks it
 * touches; a block touched for the first time is opened zeroed and gets frame k first -- never the frames before it, as
 * in Open3D -- and a block touched earlier but not by frame k is left alone.  The result is the same bits for any split
 * of the frames into calls.  Frames are teaser_tsdf_frame_c with the images of "TSDF volume".  Outputs (each may be
 * NULL): touched_out = the number of (frame, block) pairs touched, opened_out = the blocks opened by the call,
 * out_of_range_out as above.
 *
 * teaser_hip_stsdf_extract_point_cloud.  Order (DEPARTURE: Open3D walks an unordered map): blocks in ascending
 * (bx, by, bz); inside a block x, y, z ascending; inside a voxel the axes i = 0, 1, 2.  USABLE is the dense rule.  The
 * neighbour of voxel (x, y, z) along i is inside the block when its index is < U; otherwise it is voxel 0 along i of
 * block b + e_i and gives no row when that block is not open (there is no R - 1 rule here).  A row is emitted when the
 * neighbour is usable and f0 f1 < 0 (float32).  With r0 = |f0|, r1 = |f1| in float32, half = vl 0.5:
 *   p0 = ((half + vl x) + bx ul, (half + vl y) + by ul, (half + vl z) + bz ul) in double
 *   the point is p0 except p_i = (p0_i (double)r1 + (p0_i + vl) (double)r0) / (double)(r0 + r1)
 *   colour: the dense rule in double (DEPARTURE: Open3D rounds through float)
 *   normal: the dense rule with T on the GLOBAL lattice and p the point itself: per component a = q / vl - 0.5,
 *   g = floor(a), r = a - g; the eight corners in the dense order and term form; corner g + offset lies in block
 *   floor_div(g + offset, U) at the local index (g + offset) - U floor_div(g + offset, U); a corner of a block that is
 *   not open has the value 0; step 0.99 vl and the dense normalisation.
 * teaser_hip_stsdf_extract_voxel_point_cloud: every usable voxel in that order, the point p0, the colour
 * ((double)tsdf + 1.0) 0.5 three times.  Both follow the capacity rules of the dense extractions: capacity 0 with points
 * NULL returns the count alone; a capacity below the count is TEASER_HIP_ERR_BAD_ARG with the count named, count_out
 * holding it and nothing written.
 *
 * Blocks.  teaser_hip_stsdf_block_count; teaser_hip_stsdf_block_keys: (bx, by, bz) as int32 x 3 per block in ascending
 * order; teaser_hip_stsdf_download_blocks: per block, in that order, U^3 x 2 float32 (tsdf, weight) and U^3 x 3 doubles
 * in Open3D's voxel order (x U + y) U + z; either array may be NULL, not both, colours only for a volume with a colour
 * type.  teaser_hip_stsdf_upload_blocks: n_blocks keys in any order with the same arrays; a block that is not open is
 * opened (zeroed) first; a key that occurs twice, an index outside [-2^20, 2^20) and a value that is not finite (but for
 * a NaN colour of a Gray32 volume) are TEASER_HIP_ERR_BAD_ARG.  teaser_hip_stsdf_reset closes every block.
 *
 * Memory and limits.  Blocks lie in slabs: the first holds initial_blocks blocks, every further one slab_blocks; a slab
 * is allocated when the first block in it is opened and growth never copies a voxel.  A block takes 32 KiB, 128 KiB with
 * a colour type.  max_blocks (0: no limit): a call that would open more returns TEASER_HIP_ERR_OOM before the directory
 * or any voxel is changed, and so does a failed allocation; the handle stays usable.
 *
 * The calls.  TEASER_HIP_ERR_BAD_ARG names the argument and the frame; the frame checks are those of "TSDF volume";
 * more than 65535 frames in one call is TEASER_HIP_ERR_UNSUPPORTED.  An integrate call synchronises the stream TWICE:
 * once to read back the distinct touch candidates of the call -- the directory is merged on the host -- and once at the
 * end; a third time only when there are more than 262144 distinct candidates.  The launches depend on the data only
 * through the sizes read back there: one integration launch per pass of 8 frames over the blocks that pass touches.
 * Every call is deterministic: the same bits run after run; the only atomic is an integer add. */
typedef struct teaser_stsdf_volume_c {
  double voxel_length;            /* default 4.0 / 512 */
  double sdf_trunc;               /* default 0.04 */
  int32_t color_type;             /* 0 none (default), 1 RGB8, 2 Gray32 */
  int32_t volume_unit_resolution; /* U; default 16, the only value supported */
  int32_t depth_sampling_stride;  /* default 4 */
  int32_t initial_blocks;         /* blocks of the first slab; default 1024 */
  int32_t slab_blocks;            /* blocks of every further slab; default 1024 */
  int32_t reserved32;             /* must be 0 */
  int64_t max_blocks;             /* 0 (default): no limit */
  int64_t reserved;               /* must be 0 */
} teaser_stsdf_volume_c;
#ifdef __cplusplus
static_assert(sizeof(teaser_stsdf_volume_c) == 56, "teaser_stsdf_volume_c is 56 bytes");
#else
_Static_assert(sizeof(teaser_stsdf_volume_c) == 56, "teaser_stsdf_volume_c is 56 bytes");
#endif
typedef struct teaser_hip_stsdf teaser_hip_stsdf;
/* The defaults noted beside the fields above. */
TEASER_HIP_API int32_t teaser_hip_stsdf_volume_default(teaser_stsdf_volume_c* volume);
/* device < 0: the current HIP device.  The record is checked first (teaser_hip_stsdf_last_error(NULL) returns the calling
 * thread's last create message); then TEASER_HIP_ERR_NO_DEVICE without a GPU.  Nothing is allocated here. */
TEASER_HIP_API int32_t teaser_hip_stsdf_create(const teaser_stsdf_volume_c* volume, int32_t device, teaser_hip_stsdf** out);
TEASER_HIP_API int32_t teaser_hip_stsdf_destroy(teaser_hip_stsdf* stsdf);
TEASER_HIP_API const char* teaser_hip_stsdf_last_error(const teaser_hip_stsdf* stsdf);
/* DIAGNOSTIC: fills the handle's scratch and staging buffers with `byte`; see teaser_hip_icp_fill_scratch.  The blocks
 * and the directory are state and are left alone. */
TEASER_HIP_API int32_t teaser_hip_stsdf_fill_scratch(teaser_hip_stsdf* stsdf, int32_t byte, int64_t* bytes_out);
/* DIAGNOSTIC: the host's wall clock over the phases of the last integrate call, three doubles in milliseconds: upload,
 * touch pass and read-back (to the first synchronisation); the directory merge on the host; the zeroing of new blocks
 * and the integration launches (to the second synchronisation).  Zeros before the first call. */
TEASER_HIP_API int32_t teaser_hip_stsdf_last_phases(const teaser_hip_stsdf* stsdf, double* ms);
TEASER_HIP_API int32_t teaser_hip_stsdf_reset(teaser_hip_stsdf* stsdf);
TEASER_HIP_API int32_t teaser_hip_stsdf_integrate_frames(teaser_hip_stsdf* stsdf, int32_t n_frames,
                                                         const teaser_tsdf_frame_c* frames, const void* const* depth,
                                                         const void* const* color, int64_t* touched_out,
                                                         int64_t* opened_out, int64_t* out_of_range_out);
TEASER_HIP_API int32_t teaser_hip_stsdf_extract_point_cloud(teaser_hip_stsdf* stsdf, int64_t capacity, double* points,
                                                            double* normals, double* colors, int64_t* count_out);
TEASER_HIP_API int32_t teaser_hip_stsdf_extract_voxel_point_cloud(teaser_hip_stsdf* stsdf, int64_t capacity,
                                                                  double* points, double* colors, int64_t* count_out);
TEASER_HIP_API int32_t teaser_hip_stsdf_block_count(teaser_hip_stsdf* stsdf, int64_t* count_out);
/* keys: room for capacity x 3 int32; a capacity below the count is TEASER_HIP_ERR_BAD_ARG as for the extractions. */
TEASER_HIP_API int32_t teaser_hip_stsdf_block_keys(teaser_hip_stsdf* stsdf, int64_t capacity, int32_t* keys,
                                                   int64_t* count_out);
TEASER_HIP_API int32_t teaser_hip_stsdf_download_blocks(teaser_hip_stsdf* stsdf, int64_t capacity, float* tsdf_weight,
                                                        double* color, int64_t* count_out);
TEASER_HIP_API int32_t teaser_hip_stsdf_upload_blocks(teaser_hip_stsdf* stsdf, int64_t n_blocks, const int32_t* keys,
                                                      const float* tsdf_weight, const double* color);

/* Scalable TSDF ray casting: the open blocks of a scalable TSDF handle rendered into cameras -- per pixel the z-depth,
 * the world point, the normal and the colour of the first surface a ray meets.  It is the operation of Open3D's
 * t.geometry.VoxelBlockGrid.ray_cast, restated for the blocks of "Scalable TSDF volume"; Open3D is not run and bit
 * parity with an Open3D binary is NOT claimed.  The text below IS the contract; tests/stsdf_raycast_reference.py
 * restates it in numpy and is the parity target of the host and GPU tests.  Every deliberate difference from "TSDF ray
 * casting" or from Open3D is marked DEPARTURE.  No product-add is fused, every sum is taken left to right as written,
 * every min and max is written as a comparison (so a NaN's path is stated), float32 divisions are correctly rounded.
 *
 * The view is the record teaser_tsdf_view_c of "TSDF ray casting" and is built as there with origin = 0: c_k as there
 * in double, o_f[k] = (float)c_k (the world coordinates of the centre), Rt_f, fx_f, fy_f, cx_f, cy_f, dmin_f, dmax_f,
 * wthr_f as there; vl_f = (float)vl, trunc_f = (float)sdf_trunc, ul_f = (float)ul.  There is no box and no clip:
 * t0 = dmin_f, t1 = dmax_f.  The host forms in double the step cap
 *   n_cap = min(2^20, floor(((double)dmax_f - (double)dmin_f) / (double)vl_f) + 2).
 * The ray of pixel (v, u) is that of "TSDF ray casting"; the point at t is o_f + t d and t is the z-depth.
 *
 * The march.  t = t0, t_prev = t0, f_prev = -1.0f.  At most n_cap steps; a ray that has taken them all is a MISS (every
 * step is at least vl_f long, so a ray that ends earlier by the cap than by t1 has met a rounding t + step == t; the cap
 * exists so that the loop ends whatever the floats do).  Each step, in order:
 *   1. MISS unless t <= t1  (a NaN misses).
 *   2. p_k = o_k + t d_k;  g_k = floorf(p_k / vl_f): the voxel of the sample on the global lattice.
 *   3. MISS when any g_k is NaN or not in [-2^24, 2^24), tested as a float before any conversion (DEPARTURE: out there
 *      float32 no longer resolves a voxel; the dense ray cast treats the outside of its box as unobserved and goes on).
 *   4. B_k = floorf(g_k / 16.0f);  l_k = g_k - 16.0f B_k.  Both are exact, B_k lies in [-2^20, 2^20) and l_k in [0, 16).
 *   5. Block B is OPEN: f = the tsdf and w = the weight of its voxel (l_0, l_1, l_2).  HIT when
 *      f_prev > 0.0f && w >= wthr_f && f <= 0.0f.  Otherwise t_prev = t, f_prev = f;  delta = f trunc_f;
 *      t = t + (delta < vl_f ? vl_f : delta).
 *   6. Block B is NOT open: nothing is observed there, f = w = 0, and the sample is never a hit (DEPARTURE: with
 *      weight_threshold <= 0 the dense rule ends a ray that leaves its box from a positive voxel; here absent space ends
 *      no ray).  t_prev = t, f_prev = 0, and the ray skips to the face it leaves the block by: for every axis k = 0, 1, 2
 *      in turn with d_k != 0.0f,
 *        face_k = (d_k > 0.0f ? B_k + 1.0f : B_k) ul_f;  e_k = (face_k - o_k) / d_k;
 *        t_exit = e_k for the first such axis, then t_exit = e_k < t_exit ? e_k : t_exit;
 *      t_next = t + vl_f;  t = t_exit > t_next ? t_exit : t_next;  with no such axis t = t_next.  The ray always advances
 *      by at least a voxel, so a rounding that lands it just short of the face costs one more step and no surface.
 *      (DEPARTURE: Open3D bounds the march of a tile of pixels by the depth range of the blocks projected into it; the
 *      skip reaches the same blocks ray by ray and needs no second pass.)
 * As in "TSDF ray casting", a surface met out of unobserved or absent space (f_prev = 0) is not a hit, and a camera that
 * starts behind a surface sees nothing until its ray has passed an observed positive voxel.  A block is looked up anew
 * only when B differs from the last sample's; the look-up is a function of B alone, so no bit depends on that.
 *
 * A hit.  t* = (t f_prev - t_prev f) / (f_prev - f) in float32;  depth = t*.  In double
 *   q_k = (double)o_k + (double)t* (double)d_k   (world coordinates);  vertex_k = q_k rounded to float32.
 * NEAR: every |q_k| <= (2^24 + 2) vl (double; a NaN is not near).  A hit that is not near has the normal and the
 * colour 0 (DEPARTURE; it keeps an enormous q from being converted to an integer).  Otherwise:
 *   normal: the normal rule of teaser_hip_stsdf_extract_point_cloud at q -- T on the GLOBAL lattice, a corner in a block
 *   that is not open has the value 0, g = 0.99 vl, the dense normalisation -- rounded to float32.
 *   colour (a volume with a colour type): the colour rule of "TSDF ray casting" over the eight corners of q on the
 *   global lattice, corner g + offset lying in block floor_div(g + offset, 16) at the local index
 *   (g + offset) - 16 floor_div(g + offset, 16): a corner COUNTS when its block is open and its voxel weight is != 0;
 *   the same weights, order and division; / 255.0 for RGB8 only; rounded to float32, a NaN (a Gray32 volume) stored as
 *   the quiet NaN 0x7fc00000.
 * A missed pixel is 0 in every output.  In a volume with no open block every pixel misses, the maps are zeros and no
 * voxel address is formed.
 *
 * teaser_hip_stsdf_ray_cast_views takes the arguments of teaser_hip_tsdf_ray_cast_views with the scalable handle: the
 * arrays of n_views host pointers, any of them or any entry NULL, the packed row-major float32 maps, hit_counts.  One
 * launch covers all pixels of all views of any mix of sizes (blocks of 16 x 16 pixels and a block map), one stream
 * synchronisation per call; the maps come back through the handle's page-locked buffer and only the requested ones are
 * computed and copied.  The directory's device copy is uploaded again only when blocks were opened or closed since the
 * last upload.  The call modifies neither the blocks nor the directory, is stream-ordered after earlier integrations on
 * the handle, uses no atomic of any kind and gives the same bits run after run and for any grouping of the views into
 * calls.  The refusals and their texts are those of teaser_hip_tsdf_ray_cast_views. */
TEASER_HIP_API int32_t teaser_hip_stsdf_ray_cast_views(teaser_hip_stsdf* stsdf, int32_t n_views,
                                                       const teaser_tsdf_view_c* views, float* const* depth,
                                                       float* const* vertex, float* const* normal, float* const* color,
                                                       int64_t* hit_counts);

/* Scalable TSDF triangle mesh: Open3D's ScalableTSDFVolume::ExtractTriangleMesh (marching cubes over the open blocks)
 * on a scalable TSDF handle.  The text below IS the contract.  It restates Open3D from memory; Open3D is not run and bit
 * parity with an Open3D binary is NOT claimed.  Every deliberate difference is marked DEPARTURE.
 * tests/stsdf_mesh_reference.py restates this text as Open3D's loop with a dict and is the parity target of the host and
 * GPU tests.  Everything is double arithmetic, no product-add is fused, every sum is taken left to right as written.
 *
 * Reused word for word from "TSDF volume" (the triangle mesh): shift, edge_shift, edge_to_vert, the tables (the same
 * SHA-256, the same teaser_hip_tsdf_mesh_tables), the ACTIVE rule, the triangle row (v[T[t]], v[T[t + 2]], v[T[t + 1]]),
 * int32 indices, coincident vertices with distinct indices and kept degenerate triangles.
 *
 * Lattice.  The global voxel is g = 16 b + l for the voxel l of block b.  A voxel of a block that is not open has
 * tsdf 0 and weight 0, so a cube with a corner in such a block is never ACTIVE.  Cube g is considered only when the
 * block of its base voxel g is open: Open3D never visits the others.  Corner i of cube g is voxel g + shift[i], wherever
 * that lies: a cube with a local index of 15 on some axis reads voxel 0 of the next block, and a cube may have its
 * corners in eight blocks.  There is no R - 1 rule.
 *
 * Visiting order (DEPARTURE: Open3D walks an unordered map of blocks, so its order differs from run to run).  Blocks are
 * visited in ascending (bx, by, bz), the order of the directory; inside a block the cubes in ascending (lx, ly, lz), x
 * outermost.  rank(cube) = (directory rank of its block, (lx 16 + ly) 16 + lz), compared lexicographically.
 *
 * Vertices.  The lattice edge with base voxel h along axis a carries a vertex when at least one of the four cubes
 * h - du e_u - dv e_v (u < v the other two axes, du, dv in {0, 1}) is ACTIVE and its end voxels differ in sign
 * (tsdf < 0.0f).  Its CREATOR is the ACTIVE cube of smallest rank among the four, its slot the edge's number inside the
 * creator.  Vertices are numbered in ascending (rank(creator), slot): the order in which the loop first meets them.
 *   The creator is NOT the dense rule carried over.  Take an x-edge whose base voxel has local y != 0 and local z = 0,
 *   and its cubes A = h - e_y - e_z, B = h - e_y, C = h - e_z, D = h.  Globally A < B < C < D, but A and C lie in block
 *   bz - 1 and come before B and D: by rank A < C < B < D.  With A inactive and B, C ACTIVE the dense rule names B and
 *   this contract names C.
 *   Position, with a, b = edge_to_vert[slot] in the creator: f0 = |(double)tsdf(a)|, f1 = |(double)tsdf(b)|;
 *   p_k = half + vl (double)h_k with h the GLOBAL base voxel of the edge (exact: |h_k| < 2^24) and half = vl 0.5;
 *   p_axis = p_axis + (f0 vl) / (f0 + f1).  The vertex is p: there is no origin, and this is NOT the point cloud's
 *   (half + vl x) + b ul -- Open3D forms the mesh vertex from the global edge index.
 *   Colour (a volume with a colour type): the dense mesh's rule -- c0, c1 the end voxels' colours, each / 255.0 first for
 *   RGB8; (f1 c0 + f0 c1) / (f0 + f1) per component; a NaN colour of a Gray32 volume is the quiet NaN.
 *   Vertex normals (the same EXTENSION as the dense mesh): when vertex_normals is given, the normal rule of the scalable
 *   point cloud evaluated at p: T on the global lattice, 0 in a block that is not open, g = 0.99 vl, the same
 *   normalisation.
 *
 * Triangles.  For every ACTIVE cube in rank order the dense rows, v[e] being the index of the vertex on the cube's edge e.
 *
 * The call follows teaser_hip_tsdf_extract_triangle_mesh.  vertex_count_out and triangle_count_out (both required)
 * receive the counts.  Both capacities 0 with vertices and triangles NULL returns the counts alone.  Otherwise vertices
 * has room for vertex_capacity x 3 doubles, vertex_colors (only for a volume with a colour type) and vertex_normals are
 * NULL or as large, triangles has room for triangle_capacity x 3 int32.  A capacity below its count is
 * TEASER_HIP_ERR_BAD_ARG: the message names both counts, both outputs hold them, and no row of either array is written.
 * Rows behind the counts are not written.  A vertex count above 2^31 - 1 is TEASER_HIP_ERR_BAD_ARG with the count in the
 * message.  A volume with no open block answers 0 / 0.  Scratch: 5 bytes per voxel of the open blocks (a byte and a
 * 32-bit record per cube) plus 8 bytes per column and 24 per block, sized from the block count the host holds, kept on
 * the handle and grown when the directory has grown; teaser_hip_stsdf_fill_scratch reaches it; a failed allocation is
 * TEASER_HIP_ERR_OOM and leaves the blocks and the directory intact.  One stream synchronisation per call.  Launches:
 * with no open block the two scans of the block totals alone; else cubes, count and the two scans -- four launches for
 * the counts -- and one more for each array with a capacity above 0.  The launch count depends on the data only through
 * whether a block is open.  There is no atomic of any kind: the same bits run after run, and the same bits whatever
 * order the blocks were opened in -- slots differ, ranks do not.  The call modifies neither the blocks nor the
 * directory. */
TEASER_HIP_API int32_t teaser_hip_stsdf_extract_triangle_mesh(teaser_hip_stsdf* stsdf, int64_t vertex_capacity,
                                                              double* vertices, double* vertex_colors,
                                                              double* vertex_normals, int64_t triangle_capacity,
                                                              int32_t* triangles, int64_t* vertex_count_out,
                                                              int64_t* triangle_count_out);

/* Ray casting scene: triangle meshes as the TARGET of queries -- the first surface a ray meets, whether anything lies
 * between two parameters of a ray, and the closest point of the surface to a point.  The interface follows Open3D's
 * t.geometry.RaycastingScene (add_triangles, cast_rays, test_occlusions, compute_closest_points, compute_distance,
 * create_rays_pinhole).  It restates Open3D from memory; Open3D and Embree are not run and bit parity with an Open3D or
 * Embree binary is NOT claimed.  The text below IS the contract; tests/scene_reference.py restates it in numpy, by
 * brute force over all triangles, and is the parity target of the host and GPU tests.
 *
 * Geometries.  teaser_hip_scene_add_triangles takes vertices (n_vertices x 3 float32) and triangles (n_triangles x 3
 * uint32 indices into them) and answers the geometry id 0, 1, 2, ... in geometry_id_out (may be NULL).  The GLOBAL INDEX g
 * of a triangle counts the triangles of all geometries in the order added, inside a geometry in the order given.  The
 * call makes the scene uncommitted and may follow queries; teaser_hip_scene_commit builds the search structure; a query
 * on an uncommitted scene builds first.  An empty mesh is a geometry without triangles.
 *
 * Arithmetic.  Everything below is in double on the float32 inputs.  No product-add is fused.  Every three-term sum is
 * (a + b) + c.  A cross product a x b is (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), both products of a component
 * rounded; a dot product is (a0 b0 + a1 b1) + a2 b2.
 *
 * The triangle.  e1 = v1 - v0;  e2 = v2 - v0;  n = e1 x e2.  The triangle is DEAD when n == (0, 0, 0): it is never
 * hit and never closest.
 *
 * Ray-triangle test.  A ray is (ox oy oz dx dy dz), d used as given (not normalised), so t counts in units of |d|.
 *   p = d x e2;  det = e1 . p;                         det == 0: miss
 *   inv = 1.0 / det;  s = o - v0;
 *   u = (s . p) inv;                                   miss unless u >= 0 && u <= 1
 *   q = s x e1;  v = (d . q) inv;                      miss unless v >= 0 && u + v <= 1
 *   t = (e2 . q) inv;                                  miss unless t >= 0 && t < +inf
 * The comparisons are written so that a NaN misses.  Both faces are hit; nothing is culled by orientation.  A ray with
 * d == (0, 0, 0) or a non-finite component misses everything; that is an outcome, not an error.
 *
 * teaser_hip_scene_cast_rays.  The winner of a ray is the minimum of (t, g), t compared in double.  On a hit:
 *   t_hit = (float)t;  primitive_uvs = ((float)u, (float)v);  primitive_normals = (float)(n_k / sqrt(n . n));
 *   geometry_ids = the winner's geometry;  primitive_ids = its index inside that geometry.
 * On a miss: t_hit = +inf, both ids 0xFFFFFFFF, uv and normal 0.  Every output pointer may be NULL.
 *
 * teaser_hip_scene_test_occlusions.  occluded[i] = 1 iff some triangle passes the test with tnear <= t && t <= tfar,
 * else 0.
 *
 * teaser_hip_scene_closest_points.  Per triangle Ericson, Real-Time Collision Detection 5.1.5,
 * ClosestPtPointTriangle, with a = v0, b = v1, c = v2, ab = e1, ac = e2, in the order of the book:
 *   ap = p - a;  d1 = ab . ap;  d2 = ac . ap;          d1 <= 0 && d2 <= 0:                  c* = a             (v, w) = (0, 0)
 *   bp = p - b;  d3 = ab . bp;  d4 = ac . bp;          d3 >= 0 && d4 <= d3:                 c* = b             (1, 0)
 *   vc = d1 d4 - d3 d2;            vc <= 0 && d1 >= 0 && d3 <= 0:  v = d1 / (d1 - d3);      c* = a + v ab      (v, 0)
 *   cp = p - c;  d5 = ab . cp;  d6 = ac . cp;          d6 >= 0 && d5 <= d6:                 c* = c             (0, 1)
 *   vb = d5 d2 - d1 d6;            vb <= 0 && d2 >= 0 && d6 <= 0:  w = d2 / (d2 - d6);      c* = a + w ac      (0, w)
 *   va = d3 d6 - d5 d4;            va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0:
 *                                  w = (d4 - d3) / ((d4 - d3) + (d5 - d6));                 c* = b + w (c - b) (1 - w, w)
 *   otherwise  denom = 1.0 / ((va + vb) + vc);  v = vb denom;  w = vc denom;               c* = (a + ab v) + ac w
 * the first rule that applies decides.  d2* = ((cx - px)^2 + (cy - py)^2) + (cz - pz)^2 with cx = c*_x - p_x formed
 * first.  A DEAD triangle and a triangle whose d2* is not < +inf are skipped.  The winner is the minimum of (d2*, g).
 *   distance = (float)sqrt(d2*);  closest = (float)c*;  primitive_uvs = ((float)v, (float)w), the weights of v1 and
 *   v2 as for rays;  primitive_normals and the ids as for rays.
 * Without a winner (no live triangle, or a point with a non-finite component): distance = +inf, both ids 0xFFFFFFFF,
 * everything else 0.
 *
 * Views.  One record teaser_scene_view_c per view; E = extrinsic, row-major 4 x 4 world to camera as in "TSDF ray
 * casting".  The ray of pixel (row v, column u), in double:
 *   a = (((double)u + pixel_offset) - cx) / fx;   b = (((double)v + pixel_offset) - cy) / fy;
 *   d_k = (E[0][k] a + E[1][k] b) + E[2][k];      o_k = c_k = -((E[0][k] E[0][3] + E[1][k] E[1][3]) + E[2][k] E[2][3])
 * (the centre exactly as "TSDF ray casting" forms it), both rounded to float32.  These float32 rays then go through the
 * ray contract above, so t_hit is the z-depth in the camera.  teaser_hip_scene_cast_views EQUALS
 * teaser_hip_scene_cast_rays on the rays these formulas give, bit for bit.  Each output is an array of n_views host
 * pointers; a whole array or any entry may be NULL.  The maps of a view are packed height x width (t_hit, the ids),
 * height x width x 2 (uv) and height x width x 3 (normals).  Views of any mix of sizes go into one call: one launch
 * covers all pixels of all views (blocks of 16 x 16 pixels and a block map); only the requested maps are computed and
 * copied.  A view with width or height 0 is legal.  pixel_offset 0.5 (the default, Open3D's create_rays_pinhole) looks
 * through pixel centres; 0 is the convention of "Depth frames".
 *
 * The search structure is NOT part of the contract.  Every output EQUALS what the definitions above give over ALL
 * triangles; the results are the same bits for any grouping of rays, points and views into calls, for any order of
 * queries, and run after run.  No floating-point atomic is used.  (How the structure keeps that promise, and the one
 * condition its argument needs -- a ray that lies within about 1e-8 rad of a triangle's plane, where the test above
 * divides rounding noise by rounding noise -- is DESIGN.md section 41.)  One stream synchronisation per query; a query
 * that has to build adds the build's.
 *
 * TEASER_HIP_ERR_BAD_ARG (the message names the argument; the handle stays usable): a NULL handle; a negative count; NULL
 * where a count is positive (vertices, triangles, rays, points, views, occluded); a non-finite vertex; a triangle index
 * >= n_vertices; more than 2^30 triangles in a scene; tnear or tfar NaN; of a view: width or height negative or above
 * 16384, fx or fy zero or not finite, cx, cy, the extrinsic or pixel_offset not finite, reserved != 0, more than
 * 2^31 - 1 blocks in one call.  Empty meshes, zero rays, zero points and zero views are legal.
 * TEASER_HIP_ERR_HIP with "visit cap": a traversal did not end within 4 n + 64 node visits (it cannot on a tree this
 * library built; the cap exists so that damaged memory ends in an error, not in a hang).
 *
 * Not offered: signed distance and occupancy, count_intersections / list_intersections, lines and other primitives,
 * refitting after vertex motion, a device-side hand-over to the odometry, mesh sampling. */
typedef struct teaser_scene_view_c {
  int32_t width, height;
  double fx, fy, cx, cy;
  double extrinsic[16]; /* row-major, world to camera */
  double pixel_offset;  /* default 0.5 */
  int64_t reserved;     /* must be 0 */
} teaser_scene_view_c;
#ifdef __cplusplus
static_assert(sizeof(teaser_scene_view_c) == 184, "teaser_scene_view_c is 184 bytes");
#else
_Static_assert(sizeof(teaser_scene_view_c) == 184, "teaser_scene_view_c is 184 bytes");
#endif
typedef struct teaser_hip_scene teaser_hip_scene;
/* device < 0: the current HIP device.  TEASER_HIP_ERR_NO_DEVICE without a GPU: there is no CPU path. */
TEASER_HIP_API int32_t teaser_hip_scene_create(int32_t device, teaser_hip_scene** out);
TEASER_HIP_API int32_t teaser_hip_scene_destroy(teaser_hip_scene* scene);
TEASER_HIP_API const char* teaser_hip_scene_last_error(const teaser_hip_scene* scene);
/* DIAGNOSTIC, as teaser_hip_icp_fill_scratch: every scratch and staging buffer; the triangles and the tree are state. */
TEASER_HIP_API int32_t teaser_hip_scene_fill_scratch(teaser_hip_scene* scene, int32_t byte, int64_t* bytes_out);
TEASER_HIP_API int32_t teaser_hip_scene_add_triangles(teaser_hip_scene* scene, const float* vertices, int64_t n_vertices,
                                                      const uint32_t* triangles, int64_t n_triangles,
                                                      uint32_t* geometry_id_out);
TEASER_HIP_API int32_t teaser_hip_scene_commit(teaser_hip_scene* scene);
TEASER_HIP_API int32_t teaser_hip_scene_triangle_count(const teaser_hip_scene* scene, int64_t* count_out);
TEASER_HIP_API int32_t teaser_hip_scene_cast_rays(teaser_hip_scene* scene, const float* rays, int64_t n, float* t_hit,
                                                  uint32_t* geometry_ids, uint32_t* primitive_ids, float* primitive_uvs,
                                                  float* primitive_normals);
TEASER_HIP_API int32_t teaser_hip_scene_test_occlusions(teaser_hip_scene* scene, const float* rays, int64_t n, double tnear,
                                                        double tfar, uint8_t* occluded);
TEASER_HIP_API int32_t teaser_hip_scene_closest_points(teaser_hip_scene* scene, const float* points, int64_t n,
                                                       float* closest, float* distance, uint32_t* geometry_ids,
                                                       uint32_t* primitive_ids, float* primitive_uvs,
                                                       float* primitive_normals);
/* Zeroes the record, sets the identity extrinsic and pixel_offset = 0.5. */
TEASER_HIP_API int32_t teaser_hip_scene_view_default(teaser_scene_view_c* view);
TEASER_HIP_API int32_t teaser_hip_scene_cast_views(teaser_hip_scene* scene, const teaser_scene_view_c* views,
                                                   int32_t n_views, float* const* t_hit, uint32_t* const* geometry_ids,
                                                   uint32_t* const* primitive_ids, float* const* primitive_uvs,
                                                   float* const* primitive_normals);

/* Page-locked host memory from the HIP runtime THIS library runs on.  teaser_hip_submit_batch(..., INPUT_HOST) moves
 * the points with one DMA copy per cloud, at PCIe speed only when the runtime knows the pages are locked.  A buffer
 * pinned by another HIP runtime instance in the same process (e.g. the one a Python framework bundles) is pageable
 * memory to this one and is staged through an internal bounce buffer: measured 0.87 instead of 0.64 ms per
 * 128 x 5 k step (profiles/r4u).  No counterpart in the reference (its inputs are Eigen matrices in pageable memory,
 * registration.h:576-577); the synchronous entries accept any host pointer. */
TEASER_HIP_API int32_t teaser_hip_host_alloc(size_t bytes, void** out);
TEASER_HIP_API int32_t teaser_hip_host_free(void* p);

/* Deterministic synthetic problem generator (the reference has none that is
 * seeded -- registration-test.cc:398-431 and teaser_cpp_ply.cc:21-40 use random_device).
 * Host-only (no GPU needed).  src/dst: 3 x n column-major; R row-major 9; t 3; inlier_mask n
 * bytes (1 = inlier); any output pointer except src/dst may be NULL. */
TEASER_HIP_API int32_t teaser_hip_synth_problem(uint64_t seed, int32_t n, double outlier_ratio,
                                 double noise_bound, double* src, double* dst, double* R,
                                 double* t, uint8_t* inlier_mask);

#ifdef __cplusplus
}
#endif
#endif /* TEASER_HIP_H_ */
