// What the host-only programs of the ICP handle's host files share (outlier_host_driver.cpp, normals_host_driver.cpp,
// keypoints_host_driver.cpp, icp_host_driver.cpp, outlier_kernel_emulation.cpp), included in front of the csrc/*.hip
// files of the translation unit: what tests/hip_stub leaves out for device source run one lane at a time, the index of
// kernels_icp.hip in plain loops, no-op stand-ins for the launchers of the iterations, and the programs' bookkeeping
// (expect, the bitwise comparison, the token reader of the case files).
// TEST INFRASTRUCTURE ONLY.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

inline hipError_t hipHostMalloc(void** p, size_t n) { return hipHostMalloc(p, n, 0u); }
thread_local stub_dim3_ blockIdx, threadIdx, gridDim, blockDim;
template <class T> T atomicAdd(T* p, T v) { T o = *p; *p += v; return o; }
#define __ballot(k) ((k) ? 1ull : 0ull)
#define __popcll(b) __builtin_popcountll(b)
template <class T> T __shfl_xor(T v, int, int) { return v; }
#define __forceinline__ inline

#include "icp_host.h"

namespace thip {

// the index of kernels_icp.hip (count, scan, fill), in plain loops: bucket starts, points and indices in bucket order
void launch_icp_index(hipStream_t, const IcpDesc* desc, const int32_t*, int, int batch, const double* q, int32_t*,
                      int32_t*, int32_t* bstart, int32_t*, double* qs, int32_t* qj) {
  for (int p = 0; p < batch; ++p) {
    const IcpDesc& d = desc[p];
    if (d.n_t == 0) continue;
    const int64_t tb = d.tb_mask + 1;
    std::vector<int32_t> start((size_t)tb + 1, 0), cur((size_t)tb, 0);
    std::vector<int64_t> bk((size_t)d.n_t);
    for (int j = 0; j < d.n_t; ++j) {
      const double* y = q + 3 * (d.t_off + j);
      bk[(size_t)j] = icp_bucket(icp_cell(y[0], d.origin[0], d.inv_h), icp_cell(y[1], d.origin[1], d.inv_h),
                                 icp_cell(y[2], d.origin[2], d.inv_h), d.tb_mask);
      start[(size_t)bk[(size_t)j] + 1]++;
    }
    for (int64_t b = 0; b < tb; ++b) start[(size_t)b + 1] += start[(size_t)b];
    for (int64_t b = 0; b <= tb; ++b) bstart[d.b_off + b] = (int32_t)d.t_off + start[(size_t)b];
    for (int j = d.n_t - 1; j >= 0; --j) {  // any order inside a bucket: the list is sorted by (d2, j)
      const int64_t pos = d.t_off + start[(size_t)bk[(size_t)j]] + cur[(size_t)bk[(size_t)j]]++;
      qj[pos] = j;
      for (int c = 0; c < 3; ++c) qs[3 * pos + c] = q[3 * (d.t_off + j) + c];
    }
  }
}

#ifndef ICP_HOST_PRELUDE_OWN_ICP_LAUNCHERS  // a program that defines it brings its own stand-ins for these two
void launch_icp_iteration(hipStream_t, const IcpDesc*, IcpState*, const int32_t*, int, int, double*, const double*,
                          const int32_t*, const int32_t*, const double*, const double*, const double*, int, int32_t*,
                          double*) {}
void launch_icp_covariances(hipStream_t, const IcpDesc*, const IcpCovDesc*, const int32_t*, int, int, const double*,
                            const double*, const int32_t*, const int32_t*, double*) {}
#endif
void launch_icp_live(hipStream_t, const IcpState*, int, int32_t* live) { *live = 0; }

}  // namespace thip

inline int g_bad = 0;
inline void expect(bool ok, const char* what, int c) {
  if (!ok) {
    std::fprintf(stderr, "case %d: %s\n", c, what);
    ++g_bad;
  }
}

// equal bits; with nan_equal every NaN equals every NaN (where the contract only says NaN)
inline bool same(const std::vector<double>& a, const std::vector<double>& b, bool nan_equal = false) {
  if (a.size() != b.size()) return false;
  for (size_t k = 0; k < a.size(); ++k) {
    if (nan_equal && std::isnan(a[k]) && std::isnan(b[k])) continue;
    if (memcmp(&a[k], &b[k], 8) != 0) return false;
  }
  return true;
}

// The next token of a case file as a number: decimal integers, hexadecimal floats, "nan", "inf".
inline double read_number(FILE* f) {
  char tok[64];
  if (std::fscanf(f, "%63s", tok) != 1) std::exit(2);
  return std::strtod(tok, nullptr);
}
template <class T>
void read_numbers(FILE* f, std::vector<T>& v, size_t cnt) {
  v.resize(cnt);
  for (T& x : v) x = (T)read_number(f);
}
