// packed_call.h -- what the stand-alone handles whose calls pack a batch into one upload share on top of host_common.h
// (ransac.hip, plane.hip, fgr.hip, posegraph.hip): the offsets of a packed buffer (Pack), the head of a batched call
// (begin_call), the index check of a problem's correspondences (check_pairs), the seed rule (call_seed), the packing of
// per-problem rows one after the other (pack_rows) and the table of a handle's integer knobs (Knob, set_knob, get_knob).
// The per-cloud argument checks and the chunk planners stay with their handles: their refusals come in an order of
// their own.
#pragma once

#include <string.h>
#include <time.h>

#include <string>

#include "host_common.h"

namespace thip {

// Offsets of the sections of one packed buffer, each aligned to 256 bytes, and the typed pointer to a section.
struct Pack {
  size_t bytes = 0;
  size_t add(size_t n) {
    const size_t off = bytes;
    bytes += (n + 255) / 256 * 256;
    return off;
  }
  template <class T>
  static T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
  template <class T>
  static const T* at(const void* base, size_t off) { return reinterpret_cast<const T*>(static_cast<const char*>(base) + off); }
};

// The head of a batched call, up to and not including the empty batch: the caller checks its own arguments next and
// then returns TEASER_HIP_OK for batch == 0.  grid_limit: the call's kernels index problems by blockIdx.y or blockIdx.z.
inline int32_t begin_call(HandleBase* h, int32_t batch, bool grid_limit = true) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (batch < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "batch must be >= 0");
  if (grid_limit && batch > kMaxBatch) return over_batch_limit(h);
  return TEASER_HIP_OK;
}

// Problem b's correspondences (source index, target index) lie inside its clouds.
inline int32_t check_pairs(HandleBase* h, int b, const int32_t* corr, int32_t n_corr, int32_t n_src, int32_t n_dst) {
  for (int c = 0; c < n_corr; ++c) {
    if (corr[2 * c] < 0 || corr[2 * c] >= n_src)
      return fail(h, TEASER_HIP_ERR_BAD_ARG,
                  "corr: source index of pair " + std::to_string(c) + " is outside the cloud" + at(b));
    if (corr[2 * c + 1] < 0 || corr[2 * c + 1] >= n_dst)
      return fail(h, TEASER_HIP_ERR_BAD_ARG,
                  "corr: target index of pair " + std::to_string(c) + " is outside the cloud" + at(b));
  }
  return TEASER_HIP_OK;
}

// A problem's seed: 0 takes the clock, read once per call into the call's `clock_seed` (0 before the first read).
inline uint64_t call_seed(uint64_t seed, uint64_t& clock_seed) {
  if (seed != 0) return seed;
  if (clock_seed == 0) clock_seed = (uint64_t)time(nullptr);
  return clock_seed;
}

// The rows of `batch` problems one after the other at `to`: n[b] rows of row_bytes each from rows[b].  A descriptor's
// row offset is the running sum of n in batch order.
template <class T>
void pack_rows(void* to, int batch, const T* const* rows, const int32_t* n, size_t row_bytes) {
  char* p = static_cast<char*>(to);
  for (int b = 0; b < batch; ++b) {
    if (n[b] <= 0) continue;
    memcpy(p, rows[b], row_bytes * (size_t)n[b]);
    p += row_bytes * (size_t)n[b];
  }
}

// One integer knob of a handle of type H: its name, its range and its member.
template <class H>
struct Knob {
  const char* name;
  int64_t lo, hi;
  int64_t H::*value;
};

// teaser_hip_*_set_option: a value outside the range and an unknown or NULL name are refused with a message.
template <class H, size_t N>
int32_t set_knob(H* h, const Knob<H> (&knobs)[N], const char* name, int64_t value) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  for (const Knob<H>& k : knobs) {
    if (!name || strcmp(name, k.name) != 0) continue;
    if (value < k.lo || value > k.hi)
      return fail(h, TEASER_HIP_ERR_BAD_ARG,
                  std::string(k.name) + " must be in " + std::to_string(k.lo) + " .. " + std::to_string(k.hi));
    h->*k.value = value;
    return TEASER_HIP_OK;
  }
  return fail(h, TEASER_HIP_ERR_BAD_ARG, std::string("unknown option ") + (name ? name : "(NULL)"));
}

// teaser_hip_*_get_option: a failure leaves the handle's message and *value alone.
template <class H, size_t N>
int32_t get_knob(const H* h, const Knob<H> (&knobs)[N], const char* name, int64_t* value) {
  if (!h || !value || !name) return TEASER_HIP_ERR_BAD_ARG;
  for (const Knob<H>& k : knobs) {
    if (strcmp(name, k.name) != 0) continue;
    *value = h->*k.value;
    return TEASER_HIP_OK;
  }
  return TEASER_HIP_ERR_BAD_ARG;
}

}  // namespace thip
