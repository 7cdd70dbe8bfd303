// tsdf_internal.h -- what the host sides of the TSDF volume share (tsdf.hip: the handle, integration, the point clouds and
// the voxels; tsdf_mesh.hip: the triangle mesh): the handle and the views of its one volume.
#pragma once

#include "host_common.h"
#include "teaser_hip.h"
#include "tsdf_device.h"

struct teaser_hip_tsdf : thip::HandleBase {
  teaser_tsdf_volume_c vol;
  thip::TsdfGrid g;
  void* volume = nullptr;  // tsdf (n floats), weight (n floats), colour (3 n doubles), exactly sized
  size_t volume_bytes = 0;
  thip::DevBuf in, work, out;
  thip::DevBuf mesh;  // the cube bytes, cube records and column sums of the triangle mesh: allocated by its first call
  thip::HostBuf stage, back;
  ~teaser_hip_tsdf() {
    if (volume) (void)hipFree(volume);
  }
};

namespace thip {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

inline int64_t voxels(const teaser_hip_tsdf* h) { return (int64_t)h->g.R * h->g.R * h->g.R; }

inline TsdfFields fields(const teaser_hip_tsdf* h) {
  const int64_t n = voxels(h);
  char* p = static_cast<char*>(h->volume);
  TsdfFields v;
  v.tsdf = reinterpret_cast<float*>(p);
  v.weight = reinterpret_cast<float*>(p + 4 * (size_t)n);
  v.color = h->g.color_type != 0 ? reinterpret_cast<double*>(p + 8 * (size_t)n) : nullptr;
  v.n = n;
  return v;
}

}  // namespace thip
