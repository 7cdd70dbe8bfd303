// kernels_icp.hip -- batched point-to-point ICP (Open3D's RegistrationICP with TransformationEstimationPointToPoint,
// with_scaling = false; the contract is written out in include/teaser_hip.h) for gfx950.
//
// Target index, built once per call: a uniform hash grid per problem, cell edge h slightly above r (so two points
// closer than r always sit in neighbouring cells despite the rounding of the cell coordinates), cells counted into
// a power-of-two bucket table of at least 2 n_t entries, a per-problem exclusive scan, then a fill.  Neither a hash
// collision nor the order inside a bucket can change a result: the match of a source point is the lexicographic
// minimum of (d2, j) over every target point of the 27 buckets around its cell that satisfies d2 < r r, and every
// target point closer than r lies in one of those buckets.  A bucket visited twice (two neighbour cells hashing
// to the same bucket) only repeats candidates.  A large r relative to the cloud degrades to brute force.
//
// One iteration = two launches: the correspondence kernel (problem, 256-point source chunk) applies the pending
// transform U to its points, writes them back, searches and writes the match per point and the block's partial
// of the centred sums; the finalize kernel (one workgroup per problem) adds the partials in block order, applies
// the stop rule, and computes the next U (Umeyama via svd_rot3) and T = U T.  A finished problem's blocks return
// at once.  No floating-point atomics: every sum has a fixed order, and the chunking depends on the problem alone,
// so a problem gives the same bits alone and inside any batch.
//
// Point-to-plane (IcpDesc::method = 1; contract in include/teaser_hip.h, "ICP refinement: point-to-plane"): the same
// search, then the target normal of the match is gathered ONCE per source point from the packed normals (the search
// visits tens of candidates per point and uses one normal, so normals are not carried through the bucket order) and
// the block's partial holds {count, sum d2, 21 upper-triangle entries of A = sum w J J^T, 6 entries of g = sum w r J}
// = kIcpPlaneSums values.  The correspondence and finalize kernels are templates on kPlane: <false> is the
// point-to-point code exactly as before, launched when a call has no point-to-plane problem; <true> has the wider
// partial and branches per block on the problem's method (uniform over the block), its point-to-point branch
// executing the same operations in the same order, so a point-to-point problem keeps its bits in a mixed batch.
//
// Generalized ICP (IcpDesc::method = 2; "ICP refinement: Generalized ICP" in include/teaser_hip.h): the template
// parameter is kMode = 0 (point-to-point only, the former <false>), 1 (point-to-plane present, the former <true>) or
// 2 (a Generalized-ICP problem present), each launched only for calls that need it; <0> and <1> compile to what they
// were.  <2> keeps the 29-value partial and the plane finalize; after the search it gathers the 6 + 6 packed
// upper-triangle covariance entries of the matched pair once, forms M = Ct + R Cs R^T with R the rotation block of
// the accumulated T (the transform the moved points X correspond to), W = adj(M) / det(M), and adds J^T W J and
// J^T W e with J = [-[x']x | I].  Its point and plane branches are those of <1>, operation for operation.
//
// Colored ICP (IcpDesc::method = 3; "ICP refinement: Colored ICP" in include/teaser_hip.h): kMode = 3, launched only
// for calls that hold a coloured problem.  It keeps the 29-value partial and the plane finalize and carries the branches
// of <2> operation for operation; the coloured branch gathers once per matched source point the target's normal, its
// {gradient, intensity} record and the source intensity (icp_color_device.h).  What it gathers from arrives in a trailing
// parameter pack that is empty for <0>, <1> and <2>, whose signatures and code are therefore what they were.
//
// Covariance estimation (icp_cov_kernel): the same grid built over the cloud itself, one point per lane, the max_nn
// smallest (d2, j) kept in a per-lane insertion-sorted list in LDS (slot-major, so the lanes of a wave hit distinct
// banks; a per-lane register array indexed at run time would go to scratch), then the sums in list order, a cyclic
// Jacobi iteration on the symmetric 3 x 3 and the output, all by that lane.
#include <math.h>

#include "icp_cov_device.h"
#include "icp_internal.h"
#include "svd3.h"  // svd_rot3 (shared with kernels_estimate.hip)

namespace thip {

__device__ __forceinline__ double icp_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sums v[0..NS) over the 256 threads of the block in a fixed order; the result is valid in thread k < NS as out
// (returned), for its own k.
template <int NS>
__device__ __forceinline__ double icp_block_sum(const double (&v)[NS], double (*s)[NS] /* LDS [4] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const double w = icp_wave_sum(v[k]);
    if (lane == 0) s[wave][k] = w;
  }
  __syncthreads();
  const int k = threadIdx.x;
  return k < NS ? (s[0][k] + s[1][k]) + (s[2][k] + s[3][k]) : 0.0;
}

// Open3D's RobustKernel::Weight(r); L2 never reaches this.
__device__ __forceinline__ double icp_kernel_weight(int kernel, double k, double r) {
  const double a = fabs(r);
  switch (kernel) {
    case kIcpKernelHuber: return a <= k ? 1.0 : k / a;
    case kIcpKernelCauchy: {
      const double q = r / k;
      return 1.0 / (1.0 + q * q);
    }
    case kIcpKernelGM: {
      const double s = k + r * r;
      return k / (s * s);
    }
    case kIcpKernelTukey: {
      const double q = r / k, u = 1.0 - q * q;
      return a <= k ? u * u : 0.0;
    }
    default: return 1.0;
  }
}

}  // namespace thip
#include "icp_color_device.h"  // icp_color_terms, behind icp_kernel_weight
namespace thip {

// ---- target index ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void icp_count_kernel(const IcpDesc* __restrict__ descs,
                                                        const int32_t* __restrict__ tblk_prob,
                                                        const double* __restrict__ q, int32_t* __restrict__ tbucket,
                                                        int32_t* __restrict__ bcount) {
  const int p = tblk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const int64_t j = (int64_t)((int)blockIdx.x - d.tblk_off) * 256 + threadIdx.x;
  if (j >= d.n_t) return;
  const double* x = q + 3 * (d.t_off + j);
  const int64_t b = icp_bucket(icp_cell(x[0], d.origin[0], d.inv_h), icp_cell(x[1], d.origin[1], d.inv_h),
                               icp_cell(x[2], d.origin[2], d.inv_h), d.tb_mask);
  tbucket[d.t_off + j] = (int32_t)b;
  atomicAdd(&bcount[d.b_off + b], 1);
}

__global__ __launch_bounds__(kIcpScanThreads) void icp_scan_kernel(const IcpDesc* __restrict__ descs,
                                                                   const int32_t* __restrict__ bcount,
                                                                   int32_t* __restrict__ bstart,
                                                                   int32_t* __restrict__ cursor) {
  __shared__ int32_t s[kIcpScanThreads];
  const IcpDesc& d = descs[blockIdx.x];
  if (d.n_t == 0) return;
  const int64_t tb = d.tb_mask + 1;
  const int64_t chunk = (tb + kIcpScanThreads - 1) / kIcpScanThreads;
  const int64_t lo0 = (int64_t)threadIdx.x * chunk;
  const int64_t lo = lo0 < tb ? lo0 : tb, hi = lo + chunk < tb ? lo + chunk : tb;
  int32_t sum = 0;
  for (int64_t k = lo; k < hi; ++k) sum += bcount[d.b_off + k];
  s[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < kIcpScanThreads; o <<= 1) {  // inclusive Hillis-Steele scan of the per-thread sums
    const int32_t add = threadIdx.x >= (unsigned)o ? s[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  int32_t run = (int32_t)d.t_off + s[threadIdx.x] - sum;  // packed position of the first entry of bucket lo
  for (int64_t k = lo; k < hi; ++k) {
    bstart[d.b_off + k] = run;
    cursor[d.b_off + k] = run;
    run += bcount[d.b_off + k];
  }
  if (threadIdx.x == 0) bstart[d.b_off + tb] = (int32_t)(d.t_off + d.n_t);
}

__global__ __launch_bounds__(256) void icp_fill_kernel(const IcpDesc* __restrict__ descs,
                                                       const int32_t* __restrict__ tblk_prob,
                                                       const double* __restrict__ q,
                                                       const int32_t* __restrict__ tbucket,
                                                       int32_t* __restrict__ cursor, double* __restrict__ qs,
                                                       int32_t* __restrict__ qj) {
  const int p = tblk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const int64_t j = (int64_t)((int)blockIdx.x - d.tblk_off) * 256 + threadIdx.x;
  if (j >= d.n_t) return;
  const int32_t pos = atomicAdd(&cursor[d.b_off + tbucket[d.t_off + j]], 1);  // order inside a bucket: irrelevant
  const double* x = q + 3 * (d.t_off + j);
  qs[3 * (int64_t)pos] = x[0];
  qs[3 * (int64_t)pos + 1] = x[1];
  qs[3 * (int64_t)pos + 2] = x[2];
  qj[pos] = (int32_t)j;
}

// ---- one iteration ----------------------------------------------------------------------------------------------
// What one Generalized-ICP correspondence adds to v[2..28]: nothing when det(M) is not finite or not > 0.
__device__ __forceinline__ void icp_gicp_terms(const double (&x)[3], const double (&q)[3], const double* T,
                                               const double* cs, const double* ct, double (&v)[kIcpPlaneSums]) {
  const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
  const double S[9] = {cs[0], cs[1], cs[2], cs[1], cs[3], cs[4], cs[2], cs[4], cs[5]};
  double B[9];  // R Cs
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) B[3 * r + c] = (R[3 * r] * S[c] + R[3 * r + 1] * S[3 + c]) + R[3 * r + 2] * S[6 + c];
#define THIP_RCR(r, c) ((B[3 * r] * R[3 * c] + B[3 * r + 1] * R[3 * c + 1]) + B[3 * r + 2] * R[3 * c + 2])
  const double m00 = ct[0] + THIP_RCR(0, 0), m01 = ct[1] + THIP_RCR(0, 1), m02 = ct[2] + THIP_RCR(0, 2),
               m11 = ct[3] + THIP_RCR(1, 1), m12 = ct[4] + THIP_RCR(1, 2), m22 = ct[5] + THIP_RCR(2, 2);
#undef THIP_RCR
  const double a00 = m11 * m22 - m12 * m12, a01 = m02 * m12 - m01 * m22, a02 = m01 * m12 - m02 * m11,
               a11 = m00 * m22 - m02 * m02, a12 = m01 * m02 - m00 * m12, a22 = m00 * m11 - m01 * m01;
  const double det = (m00 * a00 + m01 * a01) + m02 * a02;
  if (!isfinite(det) || !(det > 0.0)) return;
  const double W[9] = {a00 / det, a01 / det, a02 / det, a01 / det, a11 / det, a12 / det,
                       a02 / det, a12 / det, a22 / det};
  const double e0 = x[0] - q[0], e1 = x[1] - q[1], e2 = x[2] - q[2];
  double we[3], G[9];  // W e;  G = [x']x W (column c of G = x' x column c of W)
#pragma unroll
  for (int r = 0; r < 3; ++r) we[r] = (W[3 * r] * e0 + W[3 * r + 1] * e1) + W[3 * r + 2] * e2;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    G[c] = x[1] * W[6 + c] - x[2] * W[3 + c];
    G[3 + c] = x[2] * W[c] - x[0] * W[6 + c];
    G[6 + c] = x[0] * W[3 + c] - x[1] * W[c];
  }
  // upper triangle of A by rows: [x']x W [x']x^T (row r = x' x row r of G), then G, then W
  v[2] = x[1] * G[2] - x[2] * G[1];
  v[3] = x[2] * G[0] - x[0] * G[2];
  v[4] = x[0] * G[1] - x[1] * G[0];
  v[5] = G[0];
  v[6] = G[1];
  v[7] = G[2];
  v[8] = x[2] * G[3] - x[0] * G[5];
  v[9] = x[0] * G[4] - x[1] * G[3];
  v[10] = G[3];
  v[11] = G[4];
  v[12] = G[5];
  v[13] = x[0] * G[7] - x[1] * G[6];
  v[14] = G[6];
  v[15] = G[7];
  v[16] = G[8];
  v[17] = W[0];
  v[18] = W[1];
  v[19] = W[2];
  v[20] = W[4];
  v[21] = W[5];
  v[22] = W[8];
  v[23] = x[1] * we[2] - x[2] * we[1];
  v[24] = x[2] * we[0] - x[0] * we[2];
  v[25] = x[0] * we[1] - x[1] * we[0];
  v[26] = we[0];
  v[27] = we[1];
  v[28] = we[2];
}

__device__ __forceinline__ const IcpColorArgs& icp_color_args(const IcpColorArgs& a) { return a; }

template <int kMode, class... Color /* IcpColorArgs for kMode = 3, else nothing */>
__global__ __launch_bounds__(kIcpBlock) void icp_corr_kernel(const IcpDesc* __restrict__ descs,
                                                             const IcpState* __restrict__ state,
                                                             const int32_t* __restrict__ blk_prob,
                                                             double* __restrict__ X, const double* __restrict__ qs,
                                                             const int32_t* __restrict__ qj,
                                                             const int32_t* __restrict__ bstart,
                                                             const double* __restrict__ normals,
                                                             const double* __restrict__ cov_s,
                                                             const double* __restrict__ cov_t,
                                                             int32_t* __restrict__ match,
                                                             double* __restrict__ partials, const Color... color) {
  static_assert(sizeof...(Color) == (kMode == 3 ? 1 : 0), "the colour arguments go with mode 3 alone");
  constexpr bool kPlane = kMode >= 1;
  constexpr int NS = kPlane ? kIcpPlaneSums : kIcpSums;
  __shared__ double s[4][NS];
  const int p = blk_prob[blockIdx.x];
  if (state[p].done) return;  // uniform over the block
  const IcpDesc& d = descs[p];
  const int chunk = (int)blockIdx.x - d.blk_off;
  const int64_t i = (int64_t)chunk * kIcpBlock + threadIdx.x;
  double v[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) v[k] = 0.0;
  if (i < d.n_s) {
    const double* U = state[p].U;
    double* xp = X + 3 * (d.s_off + i);
    const double x0 = xp[0], x1 = xp[1], x2 = xp[2];
    double x[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) x[r] = ((U[4 * r] * x0 + U[4 * r + 1] * x1) + U[4 * r + 2] * x2) + U[4 * r + 3];
    xp[0] = x[0];
    xp[1] = x[1];
    xp[2] = x[2];
    int32_t bj = -1;
    double bd = 0.0, bq[3] = {0.0, 0.0, 0.0};
    if (d.n_t > 0) {
      const int64_t c0 = icp_cell(x[0], d.origin[0], d.inv_h), c1 = icp_cell(x[1], d.origin[1], d.inv_h),
                    c2 = icp_cell(x[2], d.origin[2], d.inv_h);
      const bool near = c0 >= -1 && c1 >= -1 && c2 >= -1 && c0 <= d.cmax[0] + 1 && c1 <= d.cmax[1] + 1 &&
                        c2 <= d.cmax[2] + 1;
      if (near) {
        const double r2 = d.r2;
        for (int dz = -1; dz <= 1; ++dz)
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int64_t b = d.b_off + icp_bucket(c0 + dx, c1 + dy, c2 + dz, d.tb_mask);
              const int32_t k1 = bstart[b + 1];
              for (int32_t k = bstart[b]; k < k1; ++k) {
                const double q0 = qs[3 * (int64_t)k], q1 = qs[3 * (int64_t)k + 1], q2 = qs[3 * (int64_t)k + 2];
                const double e0 = x[0] - q0, e1 = x[1] - q1, e2 = x[2] - q2;
                const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
                if (d2 < r2) {
                  const int32_t j = qj[k];
                  if (bj < 0 || d2 < bd || (d2 == bd && j < bj)) {
                    bj = j;
                    bd = d2;
                    bq[0] = q0;
                    bq[1] = q1;
                    bq[2] = q2;
                  }
                }
              }
            }
      }
    }
    match[d.s_off + i] = bj;
    if (bj >= 0) {
      double pc[3], qc[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        pc[r] = x[r] - d.centre[r];
        qc[r] = bq[r] - d.centre[r];
      }
      v[0] = 1.0;
      v[1] = bd;
      if (kPlane && d.method == kIcpMethodPlane) {  // uniform over the block
        const double* np = normals + 3 * (d.t_off + bj);
        const double n[3] = {np[0], np[1], np[2]};
        const double e0 = pc[0] - qc[0], e1 = pc[1] - qc[1], e2 = pc[2] - qc[2];
        const double res = (e0 * n[0] + e1 * n[1]) + e2 * n[2];
        const double w = d.kernel == kIcpKernelL2 ? 1.0 : icp_kernel_weight(d.kernel, d.kernel_k, res);
        double J[6];
        J[0] = pc[1] * n[2] - pc[2] * n[1];
        J[1] = pc[2] * n[0] - pc[0] * n[2];
        J[2] = pc[0] * n[1] - pc[1] * n[0];
        J[3] = n[0];
        J[4] = n[1];
        J[5] = n[2];
        const double wr = w * res;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          const double wj = w * J[r];
#pragma unroll
          for (int c = 0; c < 6; ++c)
            if (c >= r) v[2 + 6 * r - r * (r - 1) / 2 + (c - r)] = wj * J[c];  // upper triangle by rows
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) v[23 + r] = wr * J[r];
      } else if (kMode >= 2 && d.method == kIcpMethodGicp) {  // uniform over the block
        if constexpr (kMode >= 2)
          icp_gicp_terms(pc, qc, state[p].T, cov_s + 6 * (d.s_off + i), cov_t + 6 * (d.t_off + bj), v);
      } else if (kMode == 3 && d.method == kIcpMethodColor) {  // uniform over the block
        if constexpr (kMode == 3) {
          const IcpColorArgs& ca = icp_color_args(color...);
          const double* np = normals + 3 * (d.t_off + bj);
          const double n[3] = {np[0], np[1], np[2]};
          icp_color_terms(pc, qc, n, ca.rec_t + 4 * (d.t_off + bj), ca.int_s[d.s_off + i], ca.cd[p], d.kernel,
                          d.kernel_k, v);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          v[2 + r] = pc[r];
          v[5 + r] = qc[r];
#pragma unroll
          for (int c = 0; c < 3; ++c) v[8 + 3 * r + c] = pc[r] * qc[c];
        }
      }
    }
  }
  const double tot = icp_block_sum<NS>(v, s);
  if (threadIdx.x < NS) partials[(int64_t)blockIdx.x * NS + threadIdx.x] = tot;
}

// The point-to-plane step from the summed normal equations (tot[2..22]: upper triangle of A by rows, tot[23..28]: g):
// A xi = -g by LDL^T without pivoting, R = Rz(gamma) Ry(beta) Rx(alpha), U = [R | t' + c - R c].  U stays the
// identity when a pivot is not finite or not positive or xi is not finite.
__device__ void icp_plane_step(const double* tot, const double* c, double* U) {
  double A[6][6], L[6][6], dd[6], y[6], xi[6];
  int k = 2;
  for (int r = 0; r < 6; ++r)
    for (int q = r; q < 6; ++q) {
      A[r][q] = tot[k];
      A[q][r] = tot[k];
      ++k;
    }
  for (int j = 0; j < 6; ++j) {
    double sj = A[j][j];
    for (int m = 0; m < j; ++m) sj -= L[j][m] * L[j][m] * dd[m];
    if (!isfinite(sj) || !(sj > 0.0)) return;
    dd[j] = sj;
    for (int i = j + 1; i < 6; ++i) {
      double t = A[i][j];
      for (int m = 0; m < j; ++m) t -= L[i][m] * L[j][m] * dd[m];
      L[i][j] = t / sj;
    }
  }
  for (int i = 0; i < 6; ++i) {
    double t = -tot[23 + i];
    for (int m = 0; m < i; ++m) t -= L[i][m] * y[m];
    y[i] = t;
  }
  for (int i = 0; i < 6; ++i) y[i] = y[i] / dd[i];
  for (int i = 5; i >= 0; --i) {
    double t = y[i];
    for (int m = i + 1; m < 6; ++m) t -= L[m][i] * xi[m];
    xi[i] = t;
  }
  for (int i = 0; i < 6; ++i)
    if (!isfinite(xi[i])) return;
  const double ca = cos(xi[0]), sa = sin(xi[0]), cb = cos(xi[1]), sb = sin(xi[1]), cg = cos(xi[2]), sg = sin(xi[2]);
  const double R[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                       sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                       -sb,     cb * sa,                cb * ca};
  for (int r = 0; r < 3; ++r) {
    U[4 * r] = R[3 * r];
    U[4 * r + 1] = R[3 * r + 1];
    U[4 * r + 2] = R[3 * r + 2];
    U[4 * r + 3] = (xi[3 + r] + c[r]) - ((R[3 * r] * c[0] + R[3 * r + 1] * c[1]) + R[3 * r + 2] * c[2]);
  }
}

template <int kMode>
__global__ __launch_bounds__(256) void icp_finalize_kernel(const IcpDesc* __restrict__ descs,
                                                           IcpState* __restrict__ state,
                                                           const double* __restrict__ partials) {
  constexpr bool kPlane = kMode >= 1;
  constexpr int NS = kPlane ? kIcpPlaneSums : kIcpSums;
  __shared__ double s[4][NS];
  __shared__ double tot[NS];
  const int p = blockIdx.x;
  if (state[p].done) return;
  const IcpDesc& d = descs[p];
  double v[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) v[k] = 0.0;
  for (int b = threadIdx.x; b < d.nblk; b += 256) {
    const double* pb = partials + (int64_t)(d.blk_off + b) * NS;
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] += pb[k];
  }
  const double t = icp_block_sum<NS>(v, s);
  if (threadIdx.x < NS) tot[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x != 0) return;
  IcpState& st = state[p];
  const double cnt = tot[0];
  const double fitness = cnt > 0 ? cnt / (double)d.n_s : 0.0;
  const double rmse = cnt > 0 ? sqrt(tot[1] / cnt) : 0.0;
  const int first = st.phase == 0;
  const bool converged = !first && fabs(st.fitness - fitness) < d.rel_fitness && fabs(st.rmse - rmse) < d.rel_rmse;
  st.fitness = fitness;
  st.rmse = rmse;
  st.count = (int32_t)cnt;
  st.phase = 1;
  if (converged || st.iterations >= d.max_iteration) {
    st.done = 1;
    return;
  }
  // Umeyama without scaling on the sums centred on d.centre: H = sum p' q'^T - sum p' (sum q')^T / n
  double U[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  if (kPlane && (d.method == kIcpMethodPlane || (kMode >= 2 && d.method == kIcpMethodGicp) ||
                 (kMode == 3 && d.method == kIcpMethodColor))) {
    if (cnt > 0) icp_plane_step(tot, d.centre, U);  // Generalized and Colored ICP: the same 29 sums, the same solve
  } else if (cnt > 0) {
    double mp[3], mq[3], H[9], R[9];
    for (int r = 0; r < 3; ++r) {
      mp[r] = tot[2 + r] / cnt;
      mq[r] = tot[5 + r] / cnt;
    }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) H[3 * r + c] = tot[8 + 3 * r + c] - tot[2 + r] * mq[c];
    svd_rot3(H, R);
    double ap[3], aq[3];  // the means in the problem's own coordinates
    for (int r = 0; r < 3; ++r) {
      ap[r] = d.centre[r] + mp[r];
      aq[r] = d.centre[r] + mq[r];
    }
    for (int r = 0; r < 3; ++r) {
      U[4 * r] = R[3 * r];
      U[4 * r + 1] = R[3 * r + 1];
      U[4 * r + 2] = R[3 * r + 2];
      U[4 * r + 3] = aq[r] - ((R[3 * r] * ap[0] + R[3 * r + 1] * ap[1]) + R[3 * r + 2] * ap[2]);
    }
  }
  double T[16];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c)
      T[4 * r + c] = ((U[4 * r] * st.T[c] + U[4 * r + 1] * st.T[4 + c]) + U[4 * r + 2] * st.T[8 + c]) +
                     U[4 * r + 3] * st.T[12 + c];
  for (int c = 0; c < 4; ++c) T[12 + c] = st.T[12 + c];  // last row of U is 0 0 0 1
  for (int k = 0; k < 16; ++k) st.T[k] = T[k];
  for (int k = 0; k < 12; ++k) st.U[k] = U[k];
  st.iterations += 1;
}

__global__ __launch_bounds__(256) void icp_live_kernel(const IcpState* __restrict__ state, int batch,
                                                       int32_t* __restrict__ live) {
  __shared__ int32_t n;
  if (threadIdx.x == 0) n = 0;
  __syncthreads();
  int32_t c = 0;
  for (int p = threadIdx.x; p < batch; p += 256) c += state[p].done ? 0 : 1;
  if (c) atomicAdd(&n, c);
  __syncthreads();
  if (threadIdx.x == 0) *live = n;
}

// ---- covariance estimation ---------------------------------------------------------------------------------------
// The Jacobi rotation: icp_cov_device.h.  The list, the sums and the choice of the normal are also there as functions,
// for normal estimation; this kernel keeps them written out, because the factored form changes its register
// allocation (61 instead of 101 VGPRs, another schedule) and that form has no measurement behind it (DESIGN.md
// section 18).  The two forms are the same operations in the same order.
template <int CAP>
__global__ __launch_bounds__(kIcpCovBlock) void icp_cov_kernel(const IcpDesc* __restrict__ descs,
                                                              const IcpCovDesc* __restrict__ covs,
                                                              const int32_t* __restrict__ blk_prob,
                                                              const double* __restrict__ q,
                                                              const double* __restrict__ qs,
                                                              const int32_t* __restrict__ qj,
                                                              const int32_t* __restrict__ bstart,
                                                              double* __restrict__ out) {
  __shared__ double ld[CAP][kIcpCovBlock];   // slot-major: lane l owns ld[.][l]
  __shared__ int32_t lj[CAP][kIcpCovBlock];
  const int p = blk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const int lane = threadIdx.x;
  const int64_t i = (int64_t)((int)blockIdx.x - d.blk_off) * kIcpCovBlock + lane;
  if (i >= d.n_t) return;
  const int cap = covs[p].max_nn < CAP ? covs[p].max_nn : CAP;  // <= CAP: every list index below stays inside
  const double* xp = q + 3 * (d.t_off + i);
  const double x[3] = {xp[0], xp[1], xp[2]};
  const int64_t c0 = icp_cell(x[0], d.origin[0], d.inv_h), c1 = icp_cell(x[1], d.origin[1], d.inv_h),
                c2 = icp_cell(x[2], d.origin[2], d.inv_h);
  const double r2 = d.r2;
  // A bucket reached through two neighbour cells repeats its candidates; a repeated (d2, j) is recognised at its
  // place in the list (or is beyond a full list's last entry, like the first time) and is not inserted twice.
  int m = 0;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int64_t b = d.b_off + icp_bucket(c0 + dx, c1 + dy, c2 + dz, d.tb_mask);
        const int32_t k1 = bstart[b + 1];
        for (int32_t k = bstart[b]; k < k1; ++k) {
          const double e0 = x[0] - qs[3 * (int64_t)k], e1 = x[1] - qs[3 * (int64_t)k + 1],
                       e2 = x[2] - qs[3 * (int64_t)k + 2];
          const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
          if (!(d2 < r2)) continue;
          const int32_t j = qj[k];
          int pos = m;  // the number of kept entries below (d2, j)
          while (pos > 0) {
            const double pd = ld[pos - 1][lane];
            if (!(d2 < pd || (d2 == pd && j < lj[pos - 1][lane]))) break;
            --pos;
          }
          if (pos > 0 && ld[pos - 1][lane] == d2 && lj[pos - 1][lane] == j) continue;  // seen before
          if (pos == cap) continue;                                                    // not among the cap best
          if (m < cap) ++m;
          for (int t = m - 1; t > pos; --t) {  // t <= cap - 1 < CAP
            ld[t][lane] = ld[t - 1][lane];
            lj[t][lane] = lj[t - 1][lane];
          }
          ld[pos][lane] = d2;
          lj[pos][lane] = j;
        }
      }
  double nrm[3] = {0.0, 0.0, 0.0};
  double scale = 0.0;  // (1 - eps) when a normal exists: C = I - scale n n^T; fewer than 3 neighbours: the identity
  if (m >= 3) {
    double s1[3] = {0.0, 0.0, 0.0}, s2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < m; ++k) {  // ascending (d2, j)
      const double* yp = q + 3 * (d.t_off + lj[k][lane]);
      const double o0 = yp[0] - x[0], o1 = yp[1] - x[1], o2 = yp[2] - x[2];
      s1[0] += o0;
      s1[1] += o1;
      s1[2] += o2;
      s2[0] += o0 * o0;
      s2[1] += o0 * o1;
      s2[2] += o0 * o2;
      s2[3] += o1 * o1;
      s2[4] += o1 * o2;
      s2[5] += o2 * o2;
    }
    const double dm = (double)m, dm1 = (double)(m - 1);
    double a[6] = {(s2[0] - (s1[0] * s1[0]) / dm) / dm1, (s2[1] - (s1[0] * s1[1]) / dm) / dm1,
                   (s2[2] - (s1[0] * s1[2]) / dm) / dm1, (s2[3] - (s1[1] * s1[1]) / dm) / dm1,
                   (s2[4] - (s1[1] * s1[2]) / dm) / dm1, (s2[5] - (s1[2] * s1[2]) / dm) / dm1};
    double V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < 16; ++sweep) {
      bool rotated = icp_jacobi_rotate<0, 1, 2>(a, V);
      rotated |= icp_jacobi_rotate<0, 2, 1>(a, V);
      rotated |= icp_jacobi_rotate<1, 2, 0>(a, V);
      if (!rotated) break;
    }
    // the column of the smallest diagonal entry, the first one on a tie
    // (selected value by value: a selected column index would turn V into a scratch array)
    const bool k1 = a[3] < a[0];
    const double lam = k1 ? a[3] : a[0];
    const bool k2 = a[5] < lam;
    nrm[0] = k2 ? V[2] : (k1 ? V[1] : V[0]);
    nrm[1] = k2 ? V[5] : (k1 ? V[4] : V[3]);
    nrm[2] = k2 ? V[8] : (k1 ? V[7] : V[6]);
    const double len = sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
    nrm[0] = nrm[0] / len;
    nrm[1] = nrm[1] / len;
    nrm[2] = nrm[2] / len;
    scale = 1.0 - covs[p].eps;
  }
  double* o = out + 9 * (d.t_off + i);
  const double u0 = scale * nrm[0], u1 = scale * nrm[1], u2 = scale * nrm[2];
  const double c01 = 0.0 - u0 * nrm[1], c02 = 0.0 - u0 * nrm[2], c12 = 0.0 - u1 * nrm[2];
  o[0] = 1.0 - u0 * nrm[0];
  o[1] = c01;
  o[2] = c02;
  o[3] = c01;
  o[4] = 1.0 - u1 * nrm[1];
  o[5] = c12;
  o[6] = c02;
  o[7] = c12;
  o[8] = 1.0 - u2 * nrm[2];
}

// ---- normal estimation, hybrid search ------------------------------------------------------------------------------
// The search and the sums of icp_cov_kernel; the normal, the raw covariance and the eigenvalues are written instead
// of C (icp_normal_store).  A kernel of its own, so that icp_cov_kernel keeps its registers.
template <int CAP>
__global__ __launch_bounds__(kIcpCovBlock) void icp_normals_kernel(const IcpDesc* __restrict__ descs,
                                                                  const int32_t* __restrict__ blk_prob,
                                                                  const double* __restrict__ q,
                                                                  const double* __restrict__ qs,
                                                                  const int32_t* __restrict__ qj,
                                                                  const int32_t* __restrict__ bstart,
                                                                  const IcpNormalOut out) {
  __shared__ double ld[CAP][kIcpCovBlock];   // slot-major: lane l owns ld[.][l]
  __shared__ int32_t lj[CAP][kIcpCovBlock];
  const int p = blk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const IcpNormalDesc& nd = out.nd[p];
  const int lane = threadIdx.x;
  const int64_t i = (int64_t)((int)blockIdx.x - d.blk_off) * kIcpCovBlock + lane;
  if (i >= d.n_t) return;
  const int cap = nd.max_nn < CAP ? nd.max_nn : CAP;  // <= CAP: every list index stays inside
  const double* xp = q + 3 * (d.t_off + i);
  const double x[3] = {xp[0], xp[1], xp[2]};
  const int m = icp_hybrid_list<CAP>(ld, lj, lane, cap, d, x, qs, qj, bstart);
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (m >= 3) icp_list_cov(lj, lane, m, q + 3 * d.t_off, x, a);
  icp_normal_store(out, nd, i, x, m, a);
}

// ---- launchers ------------------------------------------------------------------------------------------------
void launch_icp_index(hipStream_t s, const IcpDesc* d_desc, const int32_t* d_tblk_prob, int n_tblk, int batch,
                      const double* d_q, int32_t* d_tbucket, int32_t* d_bcount, int32_t* d_bstart,
                      int32_t* d_cursor, double* d_qs, int32_t* d_qj) {
  if (n_tblk > 0)
    hipLaunchKernelGGL(icp_count_kernel, dim3(n_tblk), dim3(256), 0, s, d_desc, d_tblk_prob, d_q, d_tbucket,
                       d_bcount);
  hipLaunchKernelGGL(icp_scan_kernel, dim3(batch), dim3(kIcpScanThreads), 0, s, d_desc, d_bcount, d_bstart,
                     d_cursor);
  if (n_tblk > 0)
    hipLaunchKernelGGL(icp_fill_kernel, dim3(n_tblk), dim3(256), 0, s, d_desc, d_tblk_prob, d_q, d_tbucket,
                       d_cursor, d_qs, d_qj);
}

template <int kMode>
static void icp_iteration(hipStream_t s, const IcpDesc* d_desc, IcpState* d_state, const int32_t* d_blk_prob, int n_blk,
                          int batch, double* d_x, const double* d_qs, const int32_t* d_qj, const int32_t* d_bstart,
                          const double* d_normals, const double* d_cov_s, const double* d_cov_t, int32_t* d_match,
                          double* d_partials) {
  if (n_blk > 0)
    hipLaunchKernelGGL(icp_corr_kernel<kMode>, dim3(n_blk), dim3(kIcpBlock), 0, s, d_desc, d_state, d_blk_prob, d_x,
                       d_qs, d_qj, d_bstart, d_normals, d_cov_s, d_cov_t, d_match, d_partials);
  hipLaunchKernelGGL(icp_finalize_kernel<kMode>, dim3(batch), dim3(256), 0, s, d_desc, d_state, d_partials);
}

// mode: 0 no point-to-plane and no Generalized-ICP problem in the call; 1 a point-to-plane problem (the wider
// partials, the method read per block); 2 a Generalized-ICP problem
void launch_icp_iteration(hipStream_t s, const IcpDesc* d_desc, IcpState* d_state, const int32_t* d_blk_prob,
                          int n_blk, int batch, double* d_x, const double* d_qs, const int32_t* d_qj,
                          const int32_t* d_bstart, const double* d_normals, const double* d_cov_s,
                          const double* d_cov_t, int mode, int32_t* d_match, double* d_partials) {
  if (mode == 2)
    icp_iteration<2>(s, d_desc, d_state, d_blk_prob, n_blk, batch, d_x, d_qs, d_qj, d_bstart, d_normals, d_cov_s,
                     d_cov_t, d_match, d_partials);
  else if (mode == 1)
    icp_iteration<1>(s, d_desc, d_state, d_blk_prob, n_blk, batch, d_x, d_qs, d_qj, d_bstart, d_normals, d_cov_s,
                     d_cov_t, d_match, d_partials);
  else
    icp_iteration<0>(s, d_desc, d_state, d_blk_prob, n_blk, batch, d_x, d_qs, d_qj, d_bstart, d_normals, d_cov_s,
                     d_cov_t, d_match, d_partials);
}

void launch_icp_iteration_color(hipStream_t s, const IcpDesc* d_desc, IcpState* d_state, const int32_t* d_blk_prob,
                                int n_blk, int batch, double* d_x, const double* d_qs, const int32_t* d_qj,
                                const int32_t* d_bstart, const double* d_normals, const double* d_cov_s,
                                const double* d_cov_t, int32_t* d_match, double* d_partials, const IcpColorArgs& col) {
  if (n_blk > 0)
    hipLaunchKernelGGL((icp_corr_kernel<3, IcpColorArgs>), dim3(n_blk), dim3(kIcpBlock), 0, s, d_desc, d_state,
                       d_blk_prob, d_x, d_qs, d_qj, d_bstart, d_normals, d_cov_s, d_cov_t, d_match, d_partials, col);
  hipLaunchKernelGGL(icp_finalize_kernel<3>, dim3(batch), dim3(256), 0, s, d_desc, d_state, d_partials);
}

void launch_icp_covariances(hipStream_t s, const IcpDesc* d_desc, const IcpCovDesc* d_cov, const int32_t* d_blk_prob,
                            int n_blk, int max_nn, const double* d_q, const double* d_qs, const int32_t* d_qj,
                            const int32_t* d_bstart, double* d_out) {
  if (n_blk <= 0) return;
  if (max_nn <= kIcpCovSmallNN)  // the capacity only bounds the list: it never changes a result
    hipLaunchKernelGGL(icp_cov_kernel<kIcpCovSmallNN>, dim3(n_blk), dim3(kIcpCovBlock), 0, s, d_desc, d_cov,
                       d_blk_prob, d_q, d_qs, d_qj, d_bstart, d_out);
  else
    hipLaunchKernelGGL(icp_cov_kernel<kIcpCovMaxNN>, dim3(n_blk), dim3(kIcpCovBlock), 0, s, d_desc, d_cov, d_blk_prob,
                       d_q, d_qs, d_qj, d_bstart, d_out);
}

void launch_icp_normals_hybrid(hipStream_t s, const IcpDesc* d_desc, const IcpNormalDesc* d_nd,
                               const int32_t* d_blk_prob, int n_blk, int max_nn, const double* d_q, const double* d_qs,
                               const int32_t* d_qj, const int32_t* d_bstart, double* d_nrm, double* d_cov,
                               double* d_eig) {
  if (n_blk <= 0) return;
  const IcpNormalOut out = {d_nd, d_nrm, d_cov, d_eig};
  if (max_nn <= kIcpCovSmallNN)  // the capacity only bounds the list: it never changes a result
    hipLaunchKernelGGL(icp_normals_kernel<kIcpCovSmallNN>, dim3(n_blk), dim3(kIcpCovBlock), 0, s, d_desc, d_blk_prob,
                       d_q, d_qs, d_qj, d_bstart, out);
  else
    hipLaunchKernelGGL(icp_normals_kernel<kIcpCovMaxNN>, dim3(n_blk), dim3(kIcpCovBlock), 0, s, d_desc, d_blk_prob,
                       d_q, d_qs, d_qj, d_bstart, out);
}

void launch_icp_live(hipStream_t s, const IcpState* d_state, int batch, int32_t* d_live) {
  hipLaunchKernelGGL(icp_live_kernel, dim3(1), dim3(256), 0, s, d_state, batch, d_live);
}

}  // namespace thip
