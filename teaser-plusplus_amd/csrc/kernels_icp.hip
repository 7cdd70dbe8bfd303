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
#include <math.h>

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
template <bool kPlane>
__global__ __launch_bounds__(kIcpBlock) void icp_corr_kernel(const IcpDesc* __restrict__ descs,
                                                             const IcpState* __restrict__ state,
                                                             const int32_t* __restrict__ blk_prob,
                                                             double* __restrict__ X, const double* __restrict__ qs,
                                                             const int32_t* __restrict__ qj,
                                                             const int32_t* __restrict__ bstart,
                                                             const double* __restrict__ normals,
                                                             int32_t* __restrict__ match,
                                                             double* __restrict__ partials) {
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

template <bool kPlane>
__global__ __launch_bounds__(256) void icp_finalize_kernel(const IcpDesc* __restrict__ descs,
                                                           IcpState* __restrict__ state,
                                                           const double* __restrict__ partials) {
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
  if (kPlane && d.method == kIcpMethodPlane) {
    if (cnt > 0) icp_plane_step(tot, d.centre, U);
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

void launch_icp_iteration(hipStream_t s, const IcpDesc* d_desc, IcpState* d_state, const int32_t* d_blk_prob,
                          int n_blk, int batch, double* d_x, const double* d_qs, const int32_t* d_qj,
                          const int32_t* d_bstart, const double* d_normals, bool plane, int32_t* d_match,
                          double* d_partials) {
  if (plane) {  // at least one point-to-plane problem: the wider partials, the method read per block
    if (n_blk > 0)
      hipLaunchKernelGGL(icp_corr_kernel<true>, dim3(n_blk), dim3(kIcpBlock), 0, s, d_desc, d_state, d_blk_prob,
                         d_x, d_qs, d_qj, d_bstart, d_normals, d_match, d_partials);
    hipLaunchKernelGGL(icp_finalize_kernel<true>, dim3(batch), dim3(256), 0, s, d_desc, d_state, d_partials);
    return;
  }
  if (n_blk > 0)
    hipLaunchKernelGGL(icp_corr_kernel<false>, dim3(n_blk), dim3(kIcpBlock), 0, s, d_desc, d_state, d_blk_prob, d_x,
                       d_qs, d_qj, d_bstart, d_normals, d_match, d_partials);
  hipLaunchKernelGGL(icp_finalize_kernel<false>, dim3(batch), dim3(256), 0, s, d_desc, d_state, d_partials);
}

void launch_icp_live(hipStream_t s, const IcpState* d_state, int batch, int32_t* d_live) {
  hipLaunchKernelGGL(icp_live_kernel, dim3(1), dim3(256), 0, s, d_state, batch, d_live);
}

}  // namespace thip
