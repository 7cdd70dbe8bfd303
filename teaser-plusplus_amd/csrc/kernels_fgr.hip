// kernels_fgr.hip -- the kernels of Fast Global Registration on correspondences (contract: include/teaser_hip.h;
// design: DESIGN.md section 24).  FP64 throughout, -ffp-contract=off, no floating-point atomics.  Every sum is taken
// in the block order of the contract: 256 consecutive items a block, the 64 lanes of a wave by xor shuffles, the four
// waves as (w0 + w1) + (w2 + w3), and the block partials by thread t taking blocks t, t + 256, ... followed by the same
// block sum.  The resident and the streamed route call the same one-lane functions (fgr_device.h) in that order, so
// they give the same bits.
#include <hip/hip_runtime.h>

#include "fgr_device.h"

namespace thip {

namespace {

__device__ __forceinline__ double fgr_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double fgr_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// Sums v[0 .. N) over the 256 threads in the fixed order; valid in thread k < N for its own k.  The caller keeps a
// barrier between two uses of s.
template <int N>
__device__ __forceinline__ double fgr_block_sum(const double (&v)[N], double (*s)[N]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double w = fgr_wave_sum(v[k]);
    if (lane == 0) s[wave][k] = w;
  }
  __syncthreads();
  const int k = threadIdx.x;
  return k < N ? (s[0][k] + s[1][k]) + (s[2][k] + s[3][k]) : 0.0;
}

// The partials of nblk blocks (FGR_SUMS apart, in LDS or HBM) added by thread t = blocks t, t + 256, ...
__device__ __forceinline__ void fgr_gather_partials(const double* part, int nblk, double (&v)[FGR_SUMS]) {
#pragma unroll
  for (int k = 0; k < FGR_SUMS; ++k) v[k] = 0.0;
  for (int b = threadIdx.x; b < nblk; b += FGR_BLOCK) {
    const double* pb = part + (int64_t)b * FGR_SUMS;
#pragma unroll
    for (int k = 0; k < FGR_SUMS; ++k) v[k] += pb[k];
  }
}

}  // namespace

// ---- normalise ------------------------------------------------------------------------------------------------------
// grid (block of 256 points, problem, cloud): the block's coordinate sums
__global__ void __launch_bounds__(FGR_BLOCK) fgr_cloud_sum_kernel(FgrBufs B) {
  __shared__ double s[4][3];
  const FgrDesc D = B.desc[blockIdx.y];
  const int side = blockIdx.z;
  const int n = side ? D.n_t : D.n_s;
  if ((int64_t)blockIdx.x * FGR_BLOCK >= n) return;  // uniform
  const int64_t i = (int64_t)blockIdx.x * FGR_BLOCK + threadIdx.x;
  const double* x = (side ? B.dst + 3 * D.dst_off : B.src + 3 * D.src_off) + 3 * i;
  double v[3] = {0.0, 0.0, 0.0};
  if (i < n) {
    v[0] = x[0];
    v[1] = x[1];
    v[2] = x[2];
  }
  const double tot = fgr_block_sum<3>(v, s);
  if (threadIdx.x < 3) B.cloud_sum[3 * ((side ? D.tblk_off : D.sblk_off) + blockIdx.x) + threadIdx.x] = tot;
}

// grid (problem, cloud): the mean
__global__ void __launch_bounds__(FGR_BLOCK) fgr_cloud_mean_kernel(FgrBufs B) {
  __shared__ double s[4][3];
  const FgrDesc D = B.desc[blockIdx.x];
  const int side = blockIdx.y;
  const int n = side ? D.n_t : D.n_s;
  const int nblk = (n + FGR_BLOCK - 1) / FGR_BLOCK;
  const double* part = B.cloud_sum + 3 * (side ? D.tblk_off : D.sblk_off);
  double v[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblk; b += FGR_BLOCK) {
    v[0] += part[3 * (int64_t)b];
    v[1] += part[3 * (int64_t)b + 1];
    v[2] += part[3 * (int64_t)b + 2];
  }
  const double tot = fgr_block_sum<3>(v, s);
  if (threadIdx.x < 3) B.state[blockIdx.x].mean[3 * side + threadIdx.x] = tot / (double)n;
}

// grid (block of 256 points, problem, cloud): the block's largest centred norm
__global__ void __launch_bounds__(FGR_BLOCK) fgr_cloud_norm_kernel(FgrBufs B) {
  __shared__ double s[4];
  const FgrDesc D = B.desc[blockIdx.y];
  const int side = blockIdx.z;
  const int n = side ? D.n_t : D.n_s;
  if ((int64_t)blockIdx.x * FGR_BLOCK >= n) return;  // uniform
  const int64_t i = (int64_t)blockIdx.x * FGR_BLOCK + threadIdx.x;
  const double* x = (side ? B.dst + 3 * D.dst_off : B.src + 3 * D.src_off) + 3 * i;
  const double* mean = B.state[blockIdx.y].mean + 3 * side;
  double m = 0.0;
  if (i < n) m = fgr_norm(x, mean);
  m = fgr_wave_max(m);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    B.cloud_max[(side ? D.tblk_off : D.sblk_off) + blockIdx.x] = fmax(fmax(s[0], s[1]), fmax(s[2], s[3]));
}

// grid (problem): the scale and the state before the first step
__global__ void __launch_bounds__(FGR_BLOCK) fgr_scale_kernel(FgrBufs B) {
  __shared__ double s[4];
  const FgrDesc D = B.desc[blockIdx.x];
  const int nbs = (D.n_s + FGR_BLOCK - 1) / FGR_BLOCK, nbt = (D.n_t + FGR_BLOCK - 1) / FGR_BLOCK;
  double m = 0.0;
  for (int b = threadIdx.x; b < nbs; b += FGR_BLOCK) m = fmax(m, B.cloud_max[D.sblk_off + b]);
  for (int b = threadIdx.x; b < nbt; b += FGR_BLOCK) m = fmax(m, B.cloud_max[D.tblk_off + b]);
  m = fgr_wave_max(m);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) fgr_start(D, B.state[blockIdx.x], fmax(fmax(s[0], s[1]), fmax(s[2], s[3])));
}

// grid (block of 256 pairs, problem): the records
__global__ void __launch_bounds__(FGR_BLOCK) fgr_pack_kernel(FgrBufs B) {
  const FgrDesc D = B.desc[blockIdx.y];
  const int c = blockIdx.x * FGR_BLOCK + threadIdx.x;
  if (c >= D.ncorr) return;
  const int64_t i = B.corr[2 * (D.corr_off + c)], j = B.corr[2 * (D.corr_off + c) + 1];
  double rec[6];
  fgr_record(B.state[blockIdx.y], B.src + 3 * (D.src_off + i), B.dst + 3 * (D.dst_off + j), rec);
  double* out = B.pairs + 6 * (D.corr_off + c);
#pragma unroll
  for (int k = 0; k < 6; ++k) out[k] = rec[k];
}

// ---- the resident route ---------------------------------------------------------------------------------------------
// One workgroup per problem, every iteration inside.  The records sit in LDS coordinate by coordinate (lane i reads
// rec[c cap + i]: consecutive lanes, consecutive doubles), the state in LDS as well; thread 0 solves and the step
// reaches the other lanes through it.
__global__ void __launch_bounds__(FGR_BLOCK) fgr_resident_kernel(FgrBufs B, const int32_t* __restrict__ idx, int keep) {
  extern __shared__ double rec[];
  __shared__ double s[4][FGR_SUMS];
  __shared__ double part[FGR_RES_MAX_BLK * FGR_SUMS];
  __shared__ double tot[FGR_SUMS];
  __shared__ FgrState st;
  const int p = idx[blockIdx.x];
  const FgrDesc D = B.desc[p];
  const int tid = threadIdx.x;
  const int nblk = (D.ncorr + FGR_BLOCK - 1) / FGR_BLOCK;  // <= FGR_RES_MAX_BLK: the host chose the route
  const int cap = nblk * FGR_BLOCK;
  {
    const double* src = reinterpret_cast<const double*>(B.state + p);
    double* dst = reinterpret_cast<double*>(&st);
    for (int k = tid; k < (int)(sizeof(FgrState) / sizeof(double)); k += FGR_BLOCK) dst[k] = src[k];
  }
  double* pairs = B.pairs + 6 * D.corr_off;
  for (int i = tid; i < D.ncorr; i += FGR_BLOCK)
#pragma unroll
    for (int c = 0; c < 6; ++c) rec[c * cap + i] = pairs[6 * (int64_t)i + c];
  __syncthreads();
  if (!fgr_live(D, st)) return;  // uniform
  FgrLog* log = B.log ? B.log + (int64_t)p * B.log_stride : nullptr;
  for (int itr = 0; itr < D.n_iter; ++itr) {
    const double mu = st.mu;
    for (int b = 0; b < nblk; ++b) {
      const int i = b * FGR_BLOCK + tid;
      double v[FGR_SUMS];
#pragma unroll
      for (int k = 0; k < FGR_SUMS; ++k) v[k] = 0.0;
      if (i < D.ncorr) {
        const double pp[3] = {rec[i], rec[cap + i], rec[2 * cap + i]};
        const double qq[3] = {rec[3 * cap + i], rec[4 * cap + i], rec[5 * cap + i]};
        fgr_terms(pp, qq, mu, v);
      }
      const double t = fgr_block_sum<FGR_SUMS>(v, s);
      if (tid < FGR_SUMS) part[b * FGR_SUMS + tid] = t;
      __syncthreads();
    }
    {
      double v[FGR_SUMS];
      fgr_gather_partials(part, nblk, v);
      const double t = fgr_block_sum<FGR_SUMS>(v, s);
      if (tid < FGR_SUMS) tot[tid] = t;
    }
    __syncthreads();
    if (tid == 0) fgr_step(D, st, tot, log);
    __syncthreads();
    double U[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) U[k] = st.delta[k];
    for (int i = tid; i < D.ncorr; i += FGR_BLOCK) {
      double q[3] = {rec[3 * cap + i], rec[4 * cap + i], rec[5 * cap + i]};
      fgr_apply(U, q);
      rec[3 * cap + i] = q[0];
      rec[4 * cap + i] = q[1];
      rec[5 * cap + i] = q[2];
    }
    __syncthreads();
  }
  {
    double* dst = reinterpret_cast<double*>(B.state + p);
    const double* src = reinterpret_cast<const double*>(&st);
    for (int k = tid; k < (int)(sizeof(FgrState) / sizeof(double)); k += FGR_BLOCK) dst[k] = src[k];
  }
  if (keep)
    for (int i = tid; i < D.ncorr; i += FGR_BLOCK)
#pragma unroll
      for (int c = 3; c < 6; ++c) pairs[6 * (int64_t)i + c] = rec[c * cap + i];
}

// ---- the streamed route ---------------------------------------------------------------------------------------------
// grid (block of 256 pairs, streamed problem): moves its records by the previous step (itr > 0), then its partial
__global__ void __launch_bounds__(FGR_BLOCK) fgr_sums_kernel(FgrBufs B, const int32_t* __restrict__ idx, int itr) {
  __shared__ double s[4][FGR_SUMS];
  const int p = idx[blockIdx.y];
  const FgrDesc D = B.desc[p];
  if ((int)(blockIdx.x * FGR_BLOCK) >= D.ncorr || itr >= D.n_iter) return;  // uniform
  const FgrState& st = B.state[p];
  if (!fgr_live(D, st)) return;  // uniform
  const int i = blockIdx.x * FGR_BLOCK + threadIdx.x;
  double v[FGR_SUMS];
#pragma unroll
  for (int k = 0; k < FGR_SUMS; ++k) v[k] = 0.0;
  if (i < D.ncorr) {
    double* r = B.pairs + 6 * (D.corr_off + i);
    const double pp[3] = {r[0], r[1], r[2]};
    double qq[3] = {r[3], r[4], r[5]};
    if (itr > 0) {
      double U[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) U[k] = st.delta[k];
      fgr_apply(U, qq);
      r[3] = qq[0];
      r[4] = qq[1];
      r[5] = qq[2];
    }
    fgr_terms(pp, qq, st.mu, v);
  }
  const double t = fgr_block_sum<FGR_SUMS>(v, s);
  if (threadIdx.x < FGR_SUMS) B.partials[(D.pblk_off + blockIdx.x) * FGR_SUMS + threadIdx.x] = t;
}

// grid (streamed problem): adds the partials, solves, schedules
__global__ void __launch_bounds__(FGR_BLOCK) fgr_step_kernel(FgrBufs B, const int32_t* __restrict__ idx, int itr) {
  __shared__ double s[4][FGR_SUMS];
  __shared__ double tot[FGR_SUMS];
  const int p = idx[blockIdx.x];
  const FgrDesc D = B.desc[p];
  if (itr >= D.n_iter || !fgr_live(D, B.state[p])) return;  // uniform
  const int nblk = (D.ncorr + FGR_BLOCK - 1) / FGR_BLOCK;
  double v[FGR_SUMS];
  fgr_gather_partials(B.partials + D.pblk_off * FGR_SUMS, nblk, v);
  const double t = fgr_block_sum<FGR_SUMS>(v, s);
  if (threadIdx.x < FGR_SUMS) tot[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) fgr_step(D, B.state[p], tot, B.log ? B.log + (int64_t)p * B.log_stride : nullptr);
}

// grid (block of 256 pairs, streamed problem): the records moved by the last step
__global__ void __launch_bounds__(FGR_BLOCK) fgr_move_kernel(FgrBufs B, const int32_t* __restrict__ idx) {
  const int p = idx[blockIdx.y];
  const FgrDesc D = B.desc[p];
  const int i = blockIdx.x * FGR_BLOCK + threadIdx.x;
  const FgrState& st = B.state[p];
  if (i >= D.ncorr || D.n_iter <= 0 || !fgr_live(D, st)) return;
  double* r = B.pairs + 6 * (D.corr_off + i);
  double qq[3] = {r[3], r[4], r[5]};
  double U[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) U[k] = st.delta[k];
  fgr_apply(U, qq);
  r[3] = qq[0];
  r[4] = qq[1];
  r[5] = qq[2];
}

__global__ void __launch_bounds__(FGR_BLOCK) fgr_finish_kernel(FgrBufs B, int batch) {
  const int p = blockIdx.x * FGR_BLOCK + threadIdx.x;
  if (p < batch) fgr_finish(B.state[p]);
}

// ---- launchers ------------------------------------------------------------------------------------------------------
void launch_fgr_normalise(hipStream_t s, int batch, int max_cloud_blk, int max_pair_blk, const FgrBufs& B) {
  if (batch <= 0) return;
  hipLaunchKernelGGL(fgr_cloud_sum_kernel, dim3(max_cloud_blk, batch, 2), dim3(FGR_BLOCK), 0, s, B);
  hipLaunchKernelGGL(fgr_cloud_mean_kernel, dim3(batch, 2), dim3(FGR_BLOCK), 0, s, B);
  hipLaunchKernelGGL(fgr_cloud_norm_kernel, dim3(max_cloud_blk, batch, 2), dim3(FGR_BLOCK), 0, s, B);
  hipLaunchKernelGGL(fgr_scale_kernel, dim3(batch), dim3(FGR_BLOCK), 0, s, B);
  if (max_pair_blk > 0) hipLaunchKernelGGL(fgr_pack_kernel, dim3(max_pair_blk, batch), dim3(FGR_BLOCK), 0, s, B);
}

hipError_t launch_fgr_resident(hipStream_t s, int n, const int32_t* idx, int max_blk, const FgrBufs& B, int keep) {
  if (n <= 0) return hipSuccess;
  const size_t lds = sizeof(double) * 6 * FGR_BLOCK * (size_t)max_blk;
  if (lds > 48 * 1024) {  // above the size every launch may ask for: opt in, up to the bound
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fgr_resident_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(sizeof(double) * 6 * FGR_RES_BOUND));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(fgr_resident_kernel, dim3(n), dim3(FGR_BLOCK), lds, s, B, idx, keep);
  return hipSuccess;
}

void launch_fgr_streamed_step(hipStream_t s, int n, const int32_t* idx, int max_blk, const FgrBufs& B, int itr) {
  if (n <= 0 || max_blk <= 0) return;
  hipLaunchKernelGGL(fgr_sums_kernel, dim3(max_blk, n), dim3(FGR_BLOCK), 0, s, B, idx, itr);
  hipLaunchKernelGGL(fgr_step_kernel, dim3(n), dim3(FGR_BLOCK), 0, s, B, idx, itr);
}

void launch_fgr_streamed_move(hipStream_t s, int n, const int32_t* idx, int max_blk, const FgrBufs& B) {
  if (n <= 0 || max_blk <= 0) return;
  hipLaunchKernelGGL(fgr_move_kernel, dim3(max_blk, n), dim3(FGR_BLOCK), 0, s, B, idx);
}

void launch_fgr_finish(hipStream_t s, int batch, const FgrBufs& B) {
  if (batch <= 0) return;
  hipLaunchKernelGGL(fgr_finish_kernel, dim3((batch + FGR_BLOCK - 1) / FGR_BLOCK), dim3(FGR_BLOCK), 0, s, B, batch);
}

}  // namespace thip
