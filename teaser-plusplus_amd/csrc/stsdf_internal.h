// stsdf_internal.h -- the handle of the scalable TSDF volume (stsdf.hip): the directory, which the host owns, and the slabs
// the blocks lie in.
#pragma once

#include <vector>

#include "stsdf_device.h"
#include "tsdf_internal.h"

struct teaser_hip_stsdf : thip::HandleBase {
  teaser_stsdf_volume_c vol;
  thip::TsdfGrid g;        // the block at the origin: R = 16, origin 0
  double ul = 0.0;         // the side of a block
  size_t block_bytes = 0;  // 32 KiB, 128 KiB with a colour type
  // The directory: the open blocks in ascending key order and the slot of each; slots are handed out in opening order,
  // so block k of slab s is slot first(s) + k and never moves.
  std::vector<uint64_t> keys;
  std::vector<int32_t> slots;
  std::vector<void*> slabs;  // slab 0: vol.initial_blocks blocks, every further one vol.slab_blocks
  double phase_ms[3] = {0.0, 0.0, 0.0};  // teaser_hip_stsdf_last_phases: the host's clock over the last integrate call
  bool dir_dirty = true;     // the device copy of the directory (dir) is behind keys / slots
  thip::DevBuf in, work, out, items, dir;
  thip::DevBuf mesh;  // the cube bytes, records and offsets of the triangle mesh (stsdf_mesh.hip): grown with the directory
  thip::HostBuf stage, back, istage;
  ~teaser_hip_stsdf() {
    for (void* p : slabs)
      if (p) (void)hipFree(p);
  }
};

namespace thip {

inline int64_t stsdf_capacity(const teaser_hip_stsdf* h) {
  if (h->slabs.empty()) return 0;
  return (int64_t)h->vol.initial_blocks + (int64_t)(h->slabs.size() - 1) * h->vol.slab_blocks;
}

inline char* stsdf_block_ptr(const teaser_hip_stsdf* h, int64_t slot) {
  const int64_t first = h->vol.initial_blocks;
  if (slot < first) return static_cast<char*>(h->slabs[0]) + (size_t)slot * h->block_bytes;
  const int64_t s = 1 + (slot - first) / h->vol.slab_blocks, k = (slot - first) % h->vol.slab_blocks;
  return static_cast<char*>(h->slabs[(size_t)s]) + (size_t)k * h->block_bytes;
}

// The directory's device copy, brought up to date when blocks were opened or closed since its last upload (stsdf.hip).
int32_t stsdf_sync_directory(teaser_hip_stsdf* h, StsdfDir* d);

}  // namespace thip
