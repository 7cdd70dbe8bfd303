// host_common.h -- what the host sides of the handles share: the members and the error reporting every handle has
// (HandleBase), the create and destroy sequences (open_handle, close_handle), the one refusal every batched call words
// the same way (over_batch_limit), the finiteness checks and, for every handle but the solver's, the grow-only buffers
// (DevBuf, HostBuf), which free themselves when their handle goes, and the diagnostic fill of those buffers
// (fill_scratch, behind every teaser_hip_*_fill_scratch).  The cloud calls of the ICP handle build on it in
// icp_host.h, the packed calls of the RANSAC, plane, FGR and pose-graph handles in packed_call.h.  solver.hip derives its
// handle from HandleBase and opens it with open_handle, but keeps buffer types of its own under other names (SolverBuf,
// PinnedBuf: another growth rule, a hipError_t answer with a retry at the exact size, and a view mode) and its own
// teardown (lanes, finisher threads).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "teaser_hip.h"

namespace thip {

inline hipError_t device_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t pinned_alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }

// A buffer that only grows: a request above the capacity frees it and allocates a quarter more than asked for.  It
// frees itself with the handle it is a member of, before ~HandleBase destroys the stream; it is never copied.
template <hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*)>
struct GrowBuf {
  void* p = nullptr;
  size_t cap = 0;
  GrowBuf() = default;
  GrowBuf(const GrowBuf&) = delete;
  GrowBuf& operator=(const GrowBuf&) = delete;
  ~GrowBuf() { release(); }
  bool ensure(size_t bytes) {
    if (bytes <= cap) return true;
    release();
    const size_t want = std::max<size_t>(bytes + bytes / 4, 256);
    if (Alloc(&p, want) != hipSuccess) return false;
    cap = want;
    return true;
  }
  void release() {
    if (p) (void)Free(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};
struct DevBuf : GrowBuf<device_alloc, hipFree> {};
struct HostBuf : GrowBuf<pinned_alloc, hipHostFree> {};  // page-locked staging

// What every handle has.  A handle derives from it and adds its buffers; they go with the derived handle's members,
// the stream after them.
struct HandleBase {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  ~HandleBase() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

inline int32_t fail(HandleBase* h, int32_t status, const std::string& msg) {
  h->err = msg;
  return status;
}

inline int32_t hip_fail(HandleBase* h, hipError_t e, const char* what) {
  h->err = std::string(what) + ": " + hipGetErrorString(e);
  return TEASER_HIP_ERR_HIP;
}

inline std::string at(int b) { return " (problem " + std::to_string(b) + ")"; }

// Leaves the calling function with hip_fail(h, error, what) when a HIP call fails.
#define FCHK(h, call, what)                                 \
  do {                                                      \
    const hipError_t e_ = (call);                           \
    if (e_ != hipSuccess) return hip_fail((h), e_, (what)); \
  } while (0)

// The refusal of a batch above what a grid's y or z extent indexes (problems are indexed by blockIdx.y or blockIdx.z).
constexpr int32_t kMaxBatch = 65535;
inline int32_t over_batch_limit(HandleBase* h) {
  return fail(h, TEASER_HIP_ERR_UNSUPPORTED, "a batch holds at most 65535 problems; split larger batches across calls");
}

inline bool finite_all(const double* p, int64_t n) {
  for (int64_t k = 0; k < n; ++k)
    if (!std::isfinite(p[k])) return false;
  return true;
}
inline bool finite_points(const double* p, int64_t n) { return finite_all(p, 3 * n); }

// One piece of a handle's scratch: `bytes` at p, in device memory or in host memory (page-locked or a std::vector).
struct ScratchSpan {
  void* p;
  size_t bytes;
  bool on_device;
};
inline ScratchSpan span_of(const DevBuf& b) { return {b.p, b.cap, true}; }
inline ScratchSpan span_of(const HostBuf& b) { return {b.p, b.cap, false}; }

// teaser_hip_*_fill_scratch (diagnostic): sets every byte of the `count` spans to `byte` -- the device ones on the
// handle's stream, the host ones once the stream has drained, so that no copy still in flight reads or writes them --
// synchronises, and reports the device bytes.  Allocates and frees nothing; a span without memory counts 0.
inline int32_t fill_scratch(HandleBase* h, int32_t byte, const ScratchSpan* spans, int count, int64_t* bytes_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (byte < 0 || byte > 255) return fail(h, TEASER_HIP_ERR_BAD_ARG, "byte must lie in 0..255");
  if (!bytes_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "bytes_out must not be NULL");
  *bytes_out = 0;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  FCHK(h, hipStreamSynchronize(h->stream), "hipStreamSynchronize (fill_scratch)");
  int64_t total = 0;
  for (int k = 0; k < count; ++k) {
    const ScratchSpan& s = spans[k];
    if (!s.p || !s.bytes) continue;
    if (s.on_device) {
      FCHK(h, hipMemsetAsync(s.p, byte, s.bytes, h->stream), "hipMemsetAsync (fill_scratch)");
      total += (int64_t)s.bytes;
    } else {
      memset(s.p, byte, s.bytes);
    }
  }
  FCHK(h, hipStreamSynchronize(h->stream), "hipStreamSynchronize (fill_scratch)");
  *bytes_out = total;
  return TEASER_HIP_OK;
}

// teaser_hip_*_create: a handle of type H on `device` (< 0: the current device) with a non-blocking stream.
template <class H>
int32_t open_handle(int32_t device, H** out) {
  if (!out) return TEASER_HIP_ERR_BAD_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return TEASER_HIP_ERR_NO_DEVICE;
  if (device < 0 && hipGetDevice(&device) != hipSuccess) return TEASER_HIP_ERR_NO_DEVICE;
  if (device >= count) return TEASER_HIP_ERR_BAD_ARG;
  if (hipSetDevice(device) != hipSuccess) return TEASER_HIP_ERR_HIP;
  H* h = new H();
  h->device = device;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return TEASER_HIP_ERR_HIP;
  }
  *out = h;
  return TEASER_HIP_OK;
}

// teaser_hip_*_destroy: drains the stream, then ~H releases the buffers and ~HandleBase the stream.
template <class H>
int32_t close_handle(H* h) {
  if (!h) return TEASER_HIP_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return TEASER_HIP_OK;
}

}  // namespace thip
