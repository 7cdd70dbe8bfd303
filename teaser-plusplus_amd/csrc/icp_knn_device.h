// icp_knn_device.h -- what the exact k-nearest-neighbour searches on the hash grid of kernels_icp.hip share: the
// whole-cloud scan (the route of a query the ring kernels put on the worklist), what a search does with a query's
// neighbours, and the launch pair.  Self k-NN, statistical removal and k-NN normal estimation (kernels_outlier.hip)
// and the two-cloud k-NN search (kernels_search.hip) instantiate the scan; each file keeps its ring kernel written
// out (DESIGN.md section 17 says why, and has the walk, its bound and the merge).
//
// The data cloud of a problem is the "target" of its IcpDesc (n_t, t_off).  Two policy types say the rest:
//   Query: where query i of a problem lies.
//   Sink:  what becomes of a query's min(k, n_t) nearest neighbours in ascending (d2, j): `merged` takes element t of
//          the scan's merge (every lane sees it), `finish` is lane 0's end of that query, Sink::Acc is what a sink
//          carries from the one to the other.  The ring kernels read a sink's members themselves.
// The per-problem descriptor type (IcpKnnDesc, IcpSearchDesc) is a template argument: the scan reads k and out_off.
#pragma once

#include <math.h>

#include <type_traits>

#include "icp_cov_device.h"
#include "icp_internal.h"

namespace thip {

// The query is point i of the indexed cloud.
struct IcpKnnSelfQuery {
  const double* q;  // the packed clouds
  __device__ __forceinline__ const double* at(const IcpDesc& d, int64_t i) const { return q + 3 * (d.t_off + i); }
};

// The query is "source" point i of the problem, anywhere in space.
struct IcpKnnCloudQuery {
  const double* xq;  // the packed query sets
  __device__ __forceinline__ const double* at(const IcpDesc& d, int64_t i) const { return xq + 3 * (d.s_off + i); }
};

// Row i of the n x k outputs, padded with -1 / +inf (avg == nullptr), or the mean distance of statistical removal:
// the distances one at a time in ascending (d2, j), from 0.0.
struct IcpKnnListOut {
  static constexpr bool kNormals = false;
  int32_t* idx;
  double* d2;
  double* avg;
  struct Acc { double sum = 0.0; };

  template <class Desc>
  __device__ __forceinline__ void merged(Acc& acc, int lane, const IcpDesc&, const Desc& kd, int64_t i,
                                         const double* /*cloud*/, const double (&)[3], int t, double md,
                                         int32_t mj) const {
    if (avg) {
      acc.sum += sqrt(md);
    } else if (lane == 0) {
      const int64_t base = kd.out_off + i * kd.k;
      idx[base + t] = mj;
      d2[base + t] = md;
    }
  }

  template <class Desc>
  __device__ __forceinline__ void finish(const Acc& acc, const IcpDesc& d, const Desc& kd, int /*p*/, int64_t i,
                                         const double (&)[3], int want) const {
    if (avg) {
      avg[d.t_off + i] = acc.sum / (double)want;
    } else {
      const int64_t base = kd.out_off + i * kd.k;
      for (int t = want; t < kd.k; ++t) {
        idx[base + t] = -1;
        d2[base + t] = INFINITY;
      }
    }
  }
};

// The neighbours into the sums of the covariance contract, then the normal of point i (k-NN normal estimation: the
// query is a point of the cloud).  Every lane sees each merged element; lane 0 keeps the sums and stores.
struct IcpKnnNormalOut : IcpNormalOut {
  static constexpr bool kNormals = true;
  struct Acc { double s1[3] = {0.0, 0.0, 0.0}, s2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; };

  template <class Desc>
  __device__ __forceinline__ void merged(Acc& acc, int lane, const IcpDesc&, const Desc&, int64_t,
                                         const double* cloud /* first point of the cloud */, const double (&x)[3], int,
                                         double, int32_t mj) const {
    if (lane == 0) icp_cov_add(acc.s1, acc.s2, cloud + 3 * (int64_t)mj, x);  // mj < n_t: want <= n_t real entries exist
  }

  template <class Desc>
  __device__ __forceinline__ void finish(const Acc& acc, const IcpDesc&, const Desc&, int p, int64_t i,
                                         const double (&x)[3], int want) const {
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (want >= 3) icp_cov_finish(acc.s1, acc.s2, want, a);
    icp_normal_store(*this, nd[p], i, x, want, a);
  }
};

// The whole-cloud route: block (one wave) w, w + gridDim.x, ... of the worklist; every lane keeps the list of its
// stride of the data cloud q, and the 64 lists are merged by repeated wave-wide minima of (d2, j).  Only worklist
// entries exist for problems with n_t > 0.
template <int CAP, class Desc, class Query, class Sink>
__device__ __forceinline__ void icp_knn_scan(double (*ld)[kIcpCovBlock], int32_t (*lj)[kIcpCovBlock],
                                             const IcpDesc* __restrict__ descs, const Desc* __restrict__ kds,
                                             const Query& query, const double* __restrict__ q, const Sink& sink,
                                             const int32_t* __restrict__ work,
                                             const int32_t* __restrict__ work_count) {
  const int lane = threadIdx.x;
  const int32_t total = *work_count;
  for (int32_t w = blockIdx.x; w < total; w += gridDim.x) {  // uniform over the wave
    const int p = work[2 * (int64_t)w];
    const int64_t i = work[2 * (int64_t)w + 1];
    const IcpDesc& d = descs[p];
    const Desc& kd = kds[p];
    int want = kd.k < d.n_t ? kd.k : d.n_t;
    want = want < CAP ? want : CAP;
    const double* xp = query.at(d, i);
    const double x[3] = {xp[0], xp[1], xp[2]};
    const double* cloud = q + 3 * d.t_off;
    int m = 0;
    for (int64_t j = lane; j < d.n_t; j += kIcpCovBlock) {
      const double* yp = cloud + 3 * j;
      const double e0 = x[0] - yp[0], e1 = x[1] - yp[1], e2 = x[2] - yp[2];
      const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
      icp_knn_insert<CAP>(ld, lj, lane, want, m, d2, (int32_t)j);
    }
    // merge: the smallest head of the 64 lists, want times (want <= n_t entries exist; an index has one owner)
    int head = 0;
    typename Sink::Acc acc;
    for (int t = 0; t < want; ++t) {
      const double hd = head < m ? ld[head][lane] : INFINITY;
      const int32_t hj = head < m ? lj[head][lane] : INT32_MAX;
      double md = hd;
      int32_t mj = hj;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(md, o, 64);
        const int32_t oj = __shfl_xor(mj, o, 64);
        if (od < md || (od == md && oj < mj)) {
          md = od;
          mj = oj;
        }
      }
      if (head < m && mj == hj) ++head;
      sink.merged(acc, lane, d, kd, i, cloud, x, t, md, mj);
    }
    if (lane == 0) sink.finish(acc, d, kd, p, i, x, want);
  }
}

// The launch pair every k-NN launcher makes: `launch(cap, ring grid, scan grid)` with the list capacity as an
// integral constant, the small one when every k of the batch fits (the capacity only bounds the list: it never
// changes a result).  Nothing is launched for an empty batch.
template <class Launch>
void icp_knn_launch(int n_blk, int top_k, Launch&& launch) {
  if (n_blk <= 0) return;
  const dim3 ring(n_blk), scan(n_blk < kIcpKnnScanBlocks ? n_blk : kIcpKnnScanBlocks);
  if (top_k <= kIcpKnnSmall)
    launch(std::integral_constant<int, kIcpKnnSmall>{}, ring, scan);
  else
    launch(std::integral_constant<int, kIcpKnnMax>{}, ring, scan);
}

}  // namespace thip
