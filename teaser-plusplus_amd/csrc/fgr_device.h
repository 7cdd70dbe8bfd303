// fgr_device.h -- what the host side (fgr.hip) and the kernels (kernels_fgr.hip) of Fast Global Registration on
// correspondences share: the records both sides read, the launchers, and the arithmetic of one pair and of one step as
// one-lane functions.  The contract is written out in include/teaser_hip.h, "Fast Global Registration on
// correspondences"; the expression order here IS that contract (the build sets -ffp-contract=off).  The one-lane
// functions are also what tests/fgr_host_driver.cpp runs on the CPU, one lane at a time.
#pragma once

#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace thip {

constexpr int FGR_BLOCK = 256;        // lanes per workgroup, and points / pairs per block of the stated summation order
constexpr int FGR_SUMS = 27;          // upper triangle of A by rows (21), then g (6)
constexpr int FGR_MIN_CORR = 10;      // Open3D: fewer pairs are not optimised
constexpr int FGR_MAX_ITER = 1024;
// The resident route keeps a problem's records in LDS, 48 bytes a pair, in whole blocks of 256 pairs.  The bound is 12
// blocks (147 456 bytes beside about 4 KB of sums and state, inside the 160 KB a workgroup of a gfx950 CU may own); the
// default is 1 block (12 KB): the one workgroup of a resident problem walks its blocks one after the other, and from a
// few blocks up the streamed route, which spreads them over the device, was measured faster.
constexpr int FGR_RES_MAX_BLK = 12;
constexpr int FGR_RES_BOUND = FGR_RES_MAX_BLK * FGR_BLOCK;  // 3072
constexpr int FGR_RES_DEFAULT = FGR_BLOCK;                  // 256
constexpr int FGR_FLAG_FEW = 1, FGR_FLAG_ZERO_SCALE = 2;

struct FgrDesc {  // one problem
  int64_t src_off, dst_off, corr_off;     // its first point (in points) of either cloud and its first pair (in pairs)
  int64_t sblk_off, tblk_off, pblk_off;   // its first block of 256 source points, target points and pairs
  double div, maxd;                       // division_factor, maximum_correspondence_distance
  int32_t n_s, n_t, ncorr, n_iter;        // n_iter: the iterations this call runs
  int32_t abs_scale, decrease_mu, run, pad;  // run = 0: ncorr < 10
};

struct FgrState {  // what the device keeps of one problem, and what the host downloads
  double mean[6];  // mu_P, mu_Q
  double scale, scale_global, scale_start, mu;
  double trans[16];  // the optimised transform (moves the target records)
  double T[16];      // source -> target in the caller's frame
  double delta[12];  // the last step
  int32_t iterations, failed, flags, pad;
};

struct FgrLog {  // one iteration of one problem, for the stage call
  double mu, A[36], g[6], xi[6], trans[16];
  int32_t flag, pad;  // flag 1: the solve failed (delta = I)
};

struct FgrBufs {
  const FgrDesc* desc;
  FgrState* state;
  const double* src;
  const double* dst;
  const int32_t* corr;
  double* pairs;      // 6 per pair: p~, q
  double* cloud_sum;  // 3 per cloud block
  double* cloud_max;  // 1 per cloud block
  double* partials;   // FGR_SUMS per pair block (streamed route)
  FgrLog* log;        // [problem][log_stride], or NULL
  int32_t log_stride;
};

// means, scale, the state's start values and the pair records of every problem
void launch_fgr_normalise(hipStream_t s, int batch, int max_cloud_blk, int max_pair_blk, const FgrBufs& B);
// the resident route: every iteration of the problems idx[0 .. n) in one launch; keep: write the moved records back
hipError_t launch_fgr_resident(hipStream_t s, int n, const int32_t* idx, int max_blk, const FgrBufs& B, int keep);
// the streamed route, iteration itr of the problems idx[0 .. n): block partials, then finalize / solve / schedule
void launch_fgr_streamed_step(hipStream_t s, int n, const int32_t* idx, int max_blk, const FgrBufs& B, int itr);
// the streamed route: the records moved by the last step (the stage call reads them)
void launch_fgr_streamed_move(hipStream_t s, int n, const int32_t* idx, int max_blk, const FgrBufs& B);
// T of every problem from its trans, means and scale
void launch_fgr_finish(hipStream_t s, int batch, const FgrBufs& B);

#define FGR_HD __host__ __device__ inline

// The 27 terms of one pair: s (J0 J0^T + J1 J1^T + J2 J2^T) by rows of the upper triangle, then s (e0 J0 + e1 J1 + e2 J2).
FGR_HD void fgr_terms(const double* p, const double* q, double mu, double* v) {
  const double e0 = p[0] - q[0], e1 = p[1] - q[1], e2 = p[2] - q[2];
  const double t = mu / (((e0 * e0 + e1 * e1) + e2 * e2) + mu);
  const double s = t * t;
  const double q0 = q[0], q1 = q[1], q2 = q[2];
  v[0] = s * (q2 * q2 + q1 * q1);  // (0,0)
  v[1] = s * (0.0 - q1 * q0);      // (0,1)
  v[2] = s * (0.0 - q2 * q0);      // (0,2)
  v[3] = 0.0;                      // (0,3)
  v[4] = s * (0.0 - q2);           // (0,4)
  v[5] = s * q1;                   // (0,5)
  v[6] = s * (q2 * q2 + q0 * q0);  // (1,1)
  v[7] = s * (0.0 - q2 * q1);      // (1,2)
  v[8] = s * q2;                   // (1,3)
  v[9] = 0.0;                      // (1,4)
  v[10] = s * (0.0 - q0);          // (1,5)
  v[11] = s * (q1 * q1 + q0 * q0); // (2,2)
  v[12] = s * (0.0 - q1);          // (2,3)
  v[13] = s * q0;                  // (2,4)
  v[14] = 0.0;                     // (2,5)
  v[15] = s;                       // (3,3)
  v[16] = 0.0;                     // (3,4)
  v[17] = 0.0;                     // (3,5)
  v[18] = s;                       // (4,4)
  v[19] = 0.0;                     // (4,5)
  v[20] = s;                       // (5,5)
  v[21] = s * (e1 * q2 - e2 * q1);
  v[22] = s * (e2 * q0 - e0 * q2);
  v[23] = s * (e0 * q1 - e1 * q0);
  v[24] = s * (0.0 - e0);
  v[25] = s * (0.0 - e1);
  v[26] = s * (0.0 - e2);
}

// apply(U, x) of the ICP contract, in place; U: rows 0..2 of the 4 x 4
FGR_HD void fgr_apply(const double* U, double* x) {
  const double a = x[0], b = x[1], c = x[2];
  x[0] = ((U[0] * a + U[1] * b) + U[2] * c) + U[3];
  x[1] = ((U[4] * a + U[5] * b) + U[6] * c) + U[7];
  x[2] = ((U[8] * a + U[9] * b) + U[10] * c) + U[11];
}

// A xi = -g by LDL^T without pivoting: the recurrences of point-to-plane ICP (icp_plane_step in kernels_icp.hip, which
// is private to its translation unit and returns the step only; here xi and the flag are wanted as well).  tot: the 27
// sums.  Returns 0 and xi, or 1: a pivot not finite or not positive (xi = 0), or xi not finite.
FGR_HD int fgr_solve(const double* tot, double* xi) {
  double A[6][6], L[6][6], dd[6], y[6];
  int k = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    xi[r] = 0.0;
#pragma unroll
    for (int q = r; q < 6; ++q) {
      A[r][q] = tot[k];
      A[q][r] = tot[k];
      ++k;
    }
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double sj = A[j][j];
#pragma unroll
    for (int m = 0; m < j; ++m) sj -= L[j][m] * L[j][m] * dd[m];
    if (!isfinite(sj) || !(sj > 0.0)) return 1;
    dd[j] = sj;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = A[i][j];
#pragma unroll
      for (int m = 0; m < j; ++m) t -= L[i][m] * L[j][m] * dd[m];
      L[i][j] = t / sj;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double t = -tot[21 + i];
#pragma unroll
    for (int m = 0; m < i; ++m) t -= L[i][m] * y[m];
    y[i] = t;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) y[i] = y[i] / dd[i];
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double t = y[i];
#pragma unroll
    for (int m = i + 1; m < 6; ++m) t -= L[m][i] * xi[m];
    xi[i] = t;
  }
  int bad = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (!isfinite(xi[i])) bad = 1;
  return bad;
}

// One step from the 27 sums: the solve, delta, trans = delta trans, the schedule, the log record.
FGR_HD void fgr_step(const FgrDesc& D, FgrState& st, const double* tot, FgrLog* log) {
  double xi[6];
  const int bad = fgr_solve(tot, xi);
  double U[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  if (!bad) {
    const double ca = cos(xi[0]), sa = sin(xi[0]), cb = cos(xi[1]), sb = sin(xi[1]), cg = cos(xi[2]), sg = sin(xi[2]);
    U[0] = cg * cb;
    U[1] = cg * sb * sa - sg * ca;
    U[2] = cg * sb * ca + sg * sa;
    U[3] = xi[3];
    U[4] = sg * cb;
    U[5] = sg * sb * sa + cg * ca;
    U[6] = sg * sb * ca - cg * sa;
    U[7] = xi[4];
    U[8] = -sb;
    U[9] = cb * sa;
    U[10] = cb * ca;
    U[11] = xi[5];
  } else {
    st.failed += 1;
  }
  double T[12];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      T[4 * r + c] = ((U[4 * r] * st.trans[c] + U[4 * r + 1] * st.trans[4 + c]) + U[4 * r + 2] * st.trans[8 + c]) +
                     U[4 * r + 3] * st.trans[12 + c];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    st.trans[k] = T[k];
    st.delta[k] = U[k];
  }
  const double mu = st.mu;
  if (D.decrease_mu && st.iterations % 4 == 0 && mu > D.maxd) st.mu = mu / D.div;
  if (log) {
    FgrLog& R = log[st.iterations];
    R.mu = mu;
    int k = 0;
    for (int r = 0; r < 6; ++r)
      for (int q = r; q < 6; ++q) {
        R.A[6 * r + q] = tot[k];
        R.A[6 * q + r] = tot[k];
        ++k;
      }
    for (int i = 0; i < 6; ++i) {
      R.g[i] = tot[21 + i];
      R.xi[i] = xi[i];
    }
    for (int i = 0; i < 16; ++i) R.trans[i] = st.trans[i];
    R.flag = bad;
    R.pad = 0;
  }
  st.iterations += 1;
}

// The state before the first step, from the means (already in st) and the scale.
FGR_HD void fgr_start(const FgrDesc& D, FgrState& st, double scale) {
  st.scale = scale;
  st.scale_global = D.abs_scale ? 1.0 : scale;
  st.scale_start = D.abs_scale ? scale : 1.0;
  st.mu = st.scale_start;
  for (int k = 0; k < 16; ++k) st.trans[k] = st.T[k] = (k % 5 == 0) ? 1.0 : 0.0;
  for (int k = 0; k < 12; ++k) st.delta[k] = (k % 5 == 0) ? 1.0 : 0.0;
  st.iterations = 0;
  st.failed = 0;
  st.flags = (D.run ? 0 : FGR_FLAG_FEW) | (scale > 0.0 ? 0 : FGR_FLAG_ZERO_SCALE);
  st.pad = 0;
}

FGR_HD bool fgr_live(const FgrDesc& D, const FgrState& st) { return D.run && !(st.flags & FGR_FLAG_ZERO_SCALE); }

// sqrt((dx dx + dy dy) + dz dz) of a centred point
FGR_HD double fgr_norm(const double* x, const double* mean) {
  const double dx = x[0] - mean[0], dy = x[1] - mean[1], dz = x[2] - mean[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// The record of one pair: (P[i] - mu_P) / scale_global, (Q[j] - mu_Q) / scale_global; zeros when the scale is 0.
FGR_HD void fgr_record(const FgrState& st, const double* p, const double* q, double* rec) {
  const bool zero = (st.flags & FGR_FLAG_ZERO_SCALE) != 0;
  for (int k = 0; k < 3; ++k) {
    rec[k] = zero ? 0.0 : (p[k] - st.mean[k]) / st.scale_global;
    rec[3 + k] = zero ? 0.0 : (q[k] - st.mean[3 + k]) / st.scale_global;
  }
}

// M = [R | (t scale_global - R mu_Q) + mu_P] from trans = [R | t]; T = [R^T | 0 - R^T t_M].
FGR_HD void fgr_finish(FgrState& st) {
  const double* A = st.trans;
  double tm[3];
  for (int r = 0; r < 3; ++r) {
    const double rm = (A[4 * r] * st.mean[3] + A[4 * r + 1] * st.mean[4]) + A[4 * r + 2] * st.mean[5];
    tm[r] = (A[4 * r + 3] * st.scale_global - rm) + st.mean[r];
  }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) st.T[4 * r + c] = A[4 * c + r];
    st.T[4 * r + 3] = 0.0 - ((A[r] * tm[0] + A[4 + r] * tm[1]) + A[8 + r] * tm[2]);
  }
  st.T[12] = st.T[13] = st.T[14] = 0.0;
  st.T[15] = 1.0;
}

}  // namespace thip
