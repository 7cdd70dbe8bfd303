// kernels_ransac.hip -- the kernels of RANSAC registration on correspondences (contract: include/teaser_hip.h; design:
// DESIGN.md section 23).  FP64 throughout, -ffp-contract=off, no floating-point atomics: every per-trial record is
// stored by trial index, so the order in which the survivors are compacted cannot reach a result.
#include <hip/hip_runtime.h>

#include "ransac_device.h"

namespace thip {

// Pack: pair c of problem b -> {P[i_c], Q[j_c]}, 48 bytes, so that scoring streams one array.
__global__ void __launch_bounds__(RS_BLOCK) ransac_pack_kernel(const RsDesc* __restrict__ desc,
                                                               const double* __restrict__ src,
                                                               const double* __restrict__ dst,
                                                               const int32_t* __restrict__ corr,
                                                               double* __restrict__ pairs) {
  const RsDesc D = desc[blockIdx.y];
  const int c = blockIdx.x * RS_BLOCK + threadIdx.x;
  if (c >= D.ncorr) return;
  const int64_t i = corr[2 * (D.corr_off + c)], j = corr[2 * (D.corr_off + c) + 1];
  double* rec = pairs + 6 * (D.pair_off + c);
  for (int k = 0; k < 3; ++k) {
    rec[k] = src[3 * (D.src_off + i) + k];
    rec[3 + k] = dst[3 * (D.dst_off + j) + k];
  }
}

// Hypothesis: one lane per trial of the chunk.  T, the flags and a zero score go out by trial index; the lanes that
// passed their checkers are compacted per wave (a ballot and one integer atomic per wave).
__global__ void __launch_bounds__(RS_BLOCK) ransac_hypothesis_kernel(const RsDesc* __restrict__ desc,
                                                                     const double* __restrict__ pairs, RsSlot slot,
                                                                     int chunk, int64_t first) {
  const int b = blockIdx.y;
  const int n = slot.n[b];
  if ((int)(blockIdx.x * RS_BLOCK) >= n) return;  // uniform
  const RsDesc D = desc[b];
  const int t = blockIdx.x * RS_BLOCK + threadIdx.x;
  const int64_t at = (int64_t)b * chunk + t;
  int flags = 0;
  if (t < n) {
    int32_t smp[RS_MAX_N];
    double T[12];
    if (D.run) {
      flags = rs_hypothesis(D, pairs + 6 * D.pair_off, first + t, smp, T);
    } else {
      for (int k = 0; k < 12; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
      for (int k = 0; k < RS_MAX_N; ++k) smp[k] = -1;
    }
    for (int k = 0; k < 12; ++k) slot.T[12 * at + k] = T[k];
    slot.flags[at] = (uint8_t)flags;
    slot.count[at] = 0;
    slot.sum[at] = 0.0;
    if (slot.samples)
      for (int k = 0; k < RS_MAX_N; ++k) slot.samples[RS_MAX_N * at + k] = (D.run && k < D.ransac_n) ? smp[k] : -1;
  }
  const bool pass = (flags & RS_FLAG_SCORED) != 0;
  const uint64_t m = __ballot(pass);
  if (m == 0) return;  // wave-uniform
  const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const int leader = __ffsll((unsigned long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(slot.nsurv + b, __popcll(m));
  base = __shfl(base, leader);
  if (pass) {
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    slot.surv[(int64_t)b * chunk + base + rank] = t;
  }
}

// Score, the hot path: grid (tile of 256 surviving hypotheses, problem).  A lane holds its T in registers; the
// workgroup stages the pair records in LDS 256 at a time and every lane reads the same address (a broadcast).  A tile is
// one block of the stated summation order: its inlier d2 are added in input order, the block sums in block order.
__global__ void __launch_bounds__(RS_BLOCK) ransac_score_kernel(const RsDesc* __restrict__ desc,
                                                                const double* __restrict__ pairs, RsSlot slot,
                                                                int chunk) {
  __shared__ double rec[6 * RS_BLOCK];
  const int b = blockIdx.y;
  const int ns = slot.nsurv[b];
  if ((int)(blockIdx.x * RS_BLOCK) >= ns) return;  // uniform
  const RsDesc D = desc[b];
  const int idx = blockIdx.x * RS_BLOCK + threadIdx.x;
  const bool live = idx < ns;
  const int64_t at = (int64_t)b * chunk + (live ? slot.surv[(int64_t)b * chunk + idx] : 0);
  double T[12];
  for (int k = 0; k < 12; ++k) T[k] = slot.T[12 * at + k];
  const double* P = pairs + 6 * D.pair_off;
  int32_t count = 0;
  double sum = 0.0;
  for (int c0 = 0; c0 < D.ncorr; c0 += RS_BLOCK) {
    const int m = min(RS_BLOCK, D.ncorr - c0);
    __syncthreads();
    for (int k = threadIdx.x; k < 6 * m; k += RS_BLOCK) rec[k] = P[6 * (int64_t)c0 + k];
    __syncthreads();
    double bs = 0.0;
    for (int c = 0; c < m; ++c) {
      const double d2 = rs_pair_d2(T, rec + 6 * c);
      if (d2 < D.r2) {
        ++count;
        bs += d2;
      }
    }
    sum += bs;
  }
  if (live) {
    slot.count[at] = count;
    slot.sum[at] = sum;
  }
}

// Prefix: one workgroup per problem turns the chunk's (count, sum d2) records, in trial order, into the list of strict
// improvements over the best carried in, and carries the best out.  A lane owns a run of consecutive trials.
__global__ void __launch_bounds__(RS_BLOCK) ransac_prefix_kernel(RsSlot slot, int chunk, int64_t first, int skip) {
  __shared__ RsBest s_best[RS_BLOCK];
  __shared__ int s_cnt[RS_BLOCK];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = slot.n[b];
  const int seg = (n + RS_BLOCK - 1) / RS_BLOCK;
  const int lo = min(n, tid * seg), hi = min(n, lo + seg);
  const int64_t base = (int64_t)b * chunk;
  RsBest local;
  local.count = -1;  // below every record
  local.rmse = 0.0;
  local.pad = 0;
  for (int t = lo; t < hi; ++t) {
    if (!(slot.flags[base + t] & RS_FLAG_SCORED)) continue;
    const int32_t c = slot.count[base + t];
    const double rm = rs_rmse(c, slot.sum[base + t]);
    if (rs_better(c, rm, local)) {
      local.count = c;
      local.rmse = rm;
    }
  }
  s_best[tid] = local;
  __syncthreads();
  RsBest run = slot.best_in[b];
  for (int k = 0; k < tid; ++k)
    if (rs_better(s_best[k].count, s_best[k].rmse, run)) run = s_best[k];
  const RsBest start = run;
  int cnt = 0;
  for (int t = lo; t < hi; ++t) {
    if (!(slot.flags[base + t] & RS_FLAG_SCORED)) continue;
    const int32_t c = slot.count[base + t];
    const double rm = rs_rmse(c, slot.sum[base + t]);
    if (rs_better(c, rm, run)) {
      run.count = c;
      run.rmse = rm;
      ++cnt;
    }
  }
  s_cnt[tid] = cnt;
  __syncthreads();
  int off = 0;
  for (int k = 0; k < tid; ++k) off += s_cnt[k];
  if (tid == RS_BLOCK - 1) {  // the last lane has seen every record
    slot.n_imp[b] = off + cnt;
    run.pad = 0;
    slot.best_out[b] = run;
  }
  run = start;
  for (int t = lo; t < hi && cnt > 0; ++t) {
    if (!(slot.flags[base + t] & RS_FLAG_SCORED)) continue;
    const int32_t c = slot.count[base + t];
    const double sm = slot.sum[base + t];
    const double rm = rs_rmse(c, sm);
    if (!rs_better(c, rm, run)) continue;
    run.count = c;
    run.rmse = rm;
    const int pos = off - skip;
    ++off;
    if (pos < 0 || pos >= RS_LIST_CAP) continue;
    RsEntry* e = slot.entries + (int64_t)b * RS_LIST_CAP + pos;
    e->trial = first + t;
    e->sum = sm;
    for (int k = 0; k < 12; ++k) e->T[k] = slot.T[12 * (base + t) + k];
    e->count = c;
    e->pad = 0;
  }
}

void launch_ransac_pack(hipStream_t s, int batch, int max_corr, const RsDesc* desc, const double* src,
                        const double* dst, const int32_t* corr, double* pairs) {
  if (batch <= 0 || max_corr <= 0) return;
  hipLaunchKernelGGL(ransac_pack_kernel, dim3((max_corr + RS_BLOCK - 1) / RS_BLOCK, batch), dim3(RS_BLOCK), 0, s, desc,
                     src, dst, corr, pairs);
}

void launch_ransac_chunk(hipStream_t s, int batch, int chunk, int max_n, const RsDesc* desc, const double* pairs,
                         const RsSlot& slot, int64_t first) {
  if (batch <= 0 || max_n <= 0) return;
  const dim3 grid((max_n + RS_BLOCK - 1) / RS_BLOCK, batch);
  hipLaunchKernelGGL(ransac_hypothesis_kernel, grid, dim3(RS_BLOCK), 0, s, desc, pairs, slot, chunk, first);
  hipLaunchKernelGGL(ransac_score_kernel, grid, dim3(RS_BLOCK), 0, s, desc, pairs, slot, chunk);
}

void launch_ransac_prefix(hipStream_t s, int batch, int chunk, const RsSlot& slot, int64_t first, int32_t skip) {
  if (batch <= 0) return;
  hipLaunchKernelGGL(ransac_prefix_kernel, dim3(batch), dim3(RS_BLOCK), 0, s, slot, chunk, first, (int)skip);
}

}  // namespace thip
