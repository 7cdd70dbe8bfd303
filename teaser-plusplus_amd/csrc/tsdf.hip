// tsdf.hip -- host side of the TSDF volume (include/teaser_hip.h, "TSDF volume"): the handle, which owns ONE volume that
// never leaves the device, and the entry checks.  Kernels: kernels_tsdf.hip; device code: tsdf_device.h; design, bytes
// moved and the resource report: DESIGN.md section 32.
//
// Integration: the rows of every depth image (and of the colour images the volume's colour type reads) are packed without
// padding into one page-locked staging array and uploaded in one copy; then ceil(n_frames / kTsdfChunk) passes over the
// volume, one launch each, and one synchronisation.  Extraction: count, scan and write into a buffer of `capacity` rows
// (the write does nothing when the total exceeds it), the total and the rows copied back, one synchronisation; the host
// then hands over exactly `count` rows.  Neither the launches nor the synchronisation depend on the data.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "tsdf_internal.h"

using namespace thip;

namespace {

thread_local std::string g_create_error;  // what teaser_hip_tsdf_last_error(NULL) returns: create has no handle yet

int32_t refuse_create(const std::string& msg) {
  g_create_error = msg;
  return TEASER_HIP_ERR_BAD_ARG;
}

int32_t integrate(teaser_hip_tsdf* h, int32_t n_frames, const teaser_tsdf_frame_c* frames, const void* const* depth,
                  const void* const* color) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (n_frames < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_frames must be >= 0");
  if (n_frames == 0) return TEASER_HIP_OK;
  if (!frames) return fail(h, TEASER_HIP_ERR_BAD_ARG, "frames must not be NULL");
  const TsdfGrid& g = h->g;
  std::vector<TsdfFrame> fd;
  size_t in_bytes = 0;
  const int32_t rc = plan_frames(h, g, n_frames, frames, depth, color, fd, &in_bytes);
  if (rc != TEASER_HIP_OK) return rc;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  if (!h->in.ensure(std::max<size_t>(in_bytes, 16)) || !h->stage.ensure(std::max<size_t>(in_bytes, 16)))
    return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (TSDF frame buffers)");
  unsigned char* stage = h->stage.as<unsigned char>();
  stage_frames(g, n_frames, frames, depth, color, fd, stage);
  hipStream_t s = h->stream;
  if (in_bytes > 0) FCHK(h, hipMemcpyAsync(h->in.p, stage, in_bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync (frames)");
  const TsdfFields v = fields(h);
  for (int b0 = 0; b0 < n_frames; b0 += kTsdfChunk) {
    TsdfChunkArgs ck;
    memset(&ck, 0, sizeof(ck));
    ck.n = std::min(kTsdfChunk, n_frames - b0);
    ck.segments = tsdf_segments(g.R);
    for (int k = 0; k < ck.n; ++k) ck.f[k] = fd[(size_t)(b0 + k)];
    launch_tsdf_integrate(s, g, ck, h->in.as<unsigned char>(), v);
  }
  FCHK(h, hipGetLastError(), "kernel launch (TSDF integration)");
  FCHK(h, hipStreamSynchronize(s), "TSDF integration");
  return TEASER_HIP_OK;
}

// mode 0: the surface points; mode 1: the voxel cloud.
int32_t extract(teaser_hip_tsdf* h, int mode, int64_t capacity, double* points, double* normals, double* colors,
                int64_t* count_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (!count_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "count_out must not be NULL");
  if (capacity < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "capacity must be >= 0");
  if (capacity > 0 && !points) return fail(h, TEASER_HIP_ERR_BAD_ARG, "points must not be NULL with a capacity above 0");
  if (mode == 0 && colors && h->g.color_type == 0)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "colors is given for a volume without colour");
  const TsdfGrid& g = h->g;
  const int64_t plane = (int64_t)g.R * g.R;
  const int64_t cap = std::min<int64_t>(capacity, (mode == 0 ? 3 : 1) * voxels(h));  // no more rows can exist
  const bool want_n = cap > 0 && normals, want_c = cap > 0 && colors;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  const size_t o_counts = round_up(sizeof(int64_t) * (size_t)(plane + 1), 256);
  const size_t row = sizeof(double) * 3 * (size_t)cap;
  const size_t o_norm = round_up(sizeof(int64_t), 256) + row, o_col = o_norm + (want_n ? row : 0);
  const size_t o_end = o_col + (want_c ? row : 0);
  if (!h->work.ensure(o_counts + sizeof(int32_t) * (size_t)plane) || !h->out.ensure(o_end) || !h->back.ensure(o_end))
    return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (TSDF extraction buffers)");
  hipStream_t s = h->stream;
  const TsdfFields v = fields(h);
  int64_t* offsets = h->work.as<int64_t>();
  int32_t* counts = reinterpret_cast<int32_t*>(h->work.as<char>() + o_counts);
  char* out = h->out.as<char>();
  const size_t o_pts = round_up(sizeof(int64_t), 256);
  launch_tsdf_count(s, g, v, mode, counts, offsets);
  FCHK(h, hipMemcpyAsync(out, offsets + plane, sizeof(int64_t), hipMemcpyDeviceToDevice, s), "hipMemcpyAsync (count)");
  if (cap > 0)
    launch_tsdf_write(s, g, v, mode, offsets, cap, reinterpret_cast<double*>(out + o_pts),
                      want_n ? reinterpret_cast<double*>(out + o_norm) : nullptr,
                      want_c ? reinterpret_cast<double*>(out + o_col) : nullptr);
  FCHK(h, hipGetLastError(), "kernel launch (TSDF extraction)");
  FCHK(h, hipMemcpyAsync(h->back.p, out, cap > 0 ? o_end : sizeof(int64_t), hipMemcpyDeviceToHost, s),
       "hipMemcpyAsync (TSDF extraction)");
  FCHK(h, hipStreamSynchronize(s), "TSDF extraction");
  const char* back = h->back.as<char>();
  int64_t count = 0;
  memcpy(&count, back, sizeof(count));
  *count_out = count;
  if (capacity == 0 && !points) return TEASER_HIP_OK;  // the count alone
  if (count > capacity)
    return fail(h, TEASER_HIP_ERR_BAD_ARG,
                "capacity " + std::to_string(capacity) + " is below the count " + std::to_string(count));
  const size_t bytes = sizeof(double) * 3 * (size_t)count;
  if (bytes > 0) {
    memcpy(points, back + o_pts, bytes);
    if (want_n) memcpy(normals, back + o_norm, bytes);
    if (want_c) memcpy(colors, back + o_col, bytes);
  }
  return TEASER_HIP_OK;
}

}  // namespace

extern "C" {

int32_t teaser_hip_tsdf_volume_default(teaser_tsdf_volume_c* v) {
  if (!v) return TEASER_HIP_ERR_BAD_ARG;
  memset(v, 0, sizeof(*v));
  v->length = 4.0;
  v->sdf_trunc = 0.04;
  v->resolution = 512;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_tsdf_create(const teaser_tsdf_volume_c* vol, int32_t device, teaser_hip_tsdf** out) {
  g_create_error.clear();
  if (!out) return refuse_create("out must not be NULL");
  *out = nullptr;
  if (!vol) return refuse_create("volume must not be NULL");
  if (vol->resolution < 1 || vol->resolution > kTsdfMaxR) return refuse_create("resolution must lie in [1, 1024]");
  if (!std::isfinite(vol->length) || !(vol->length > 0.0)) return refuse_create("length must be finite and > 0");
  if (!std::isfinite(vol->sdf_trunc) || !(vol->sdf_trunc > 0.0)) return refuse_create("sdf_trunc must be finite and > 0");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(vol->origin[k])) return refuse_create("origin must be finite");
  if (vol->color_type < 0 || vol->color_type > 2) return refuse_create("color_type must be 0 (none), 1 (RGB8) or 2 (Gray32)");
  if (vol->reserved != 0) return refuse_create("reserved must be 0");
  teaser_hip_tsdf* h = nullptr;
  const int32_t rc = open_handle(device, &h);
  if (rc != TEASER_HIP_OK) return rc;
  h->vol = *vol;
  TsdfGrid& g = h->g;
  memset(&g, 0, sizeof(g));
  g.R = vol->resolution, g.color_type = vol->color_type;
  g.vl = vol->length / (double)vol->resolution;
  g.half = g.vl * 0.5;
  g.vl_f = (float)g.vl;
  g.half_f = g.vl_f * 0.5f;
  g.trunc_f = (float)vol->sdf_trunc;
  g.inv_f = 1.0f / g.trunc_f;
  for (int k = 0; k < 3; ++k) g.origin[k] = vol->origin[k], g.org_f[k] = (float)vol->origin[k];
  const size_t n = (size_t)voxels(h);
  h->volume_bytes = (g.color_type != 0 ? 32 : 8) * n;
  if (hipMalloc(&h->volume, h->volume_bytes) != hipSuccess) {
    g_create_error = "allocation failed (TSDF volume of " + std::to_string(h->volume_bytes) + " bytes)";
    h->volume = nullptr;
    close_handle(h);
    return TEASER_HIP_ERR_OOM;
  }
  if (hipMemsetAsync(h->volume, 0, h->volume_bytes, h->stream) != hipSuccess ||
      hipStreamSynchronize(h->stream) != hipSuccess) {
    close_handle(h);
    g_create_error = "hipMemsetAsync failed (TSDF volume)";
    return TEASER_HIP_ERR_HIP;
  }
  *out = h;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_tsdf_destroy(teaser_hip_tsdf* h) { return close_handle(h); }
const char* teaser_hip_tsdf_last_error(const teaser_hip_tsdf* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int32_t teaser_hip_tsdf_fill_scratch(teaser_hip_tsdf* h, int32_t byte, int64_t* bytes_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  // not h->volume: the volume is the handle's state
  const ScratchSpan spans[] = {span_of(h->in),   span_of(h->work),  span_of(h->out),
                               span_of(h->mesh), span_of(h->stage), span_of(h->back)};
  return fill_scratch(h, byte, spans, 6, bytes_out);
}

int32_t teaser_hip_tsdf_reset(teaser_hip_tsdf* h) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  FCHK(h, hipMemsetAsync(h->volume, 0, h->volume_bytes, h->stream), "hipMemsetAsync (TSDF volume)");
  FCHK(h, hipStreamSynchronize(h->stream), "TSDF reset");
  return TEASER_HIP_OK;
}

int32_t teaser_hip_tsdf_integrate_batch(teaser_hip_tsdf* h, int32_t n_frames, const teaser_tsdf_frame_c* frames,
                                        const void* const* depth, const void* const* color) {
  return integrate(h, n_frames, frames, depth, color);
}

int32_t teaser_hip_tsdf_extract_point_cloud(teaser_hip_tsdf* h, int64_t capacity, double* points, double* normals,
                                            double* colors, int64_t* count_out) {
  return extract(h, 0, capacity, points, normals, colors, count_out);
}

int32_t teaser_hip_tsdf_extract_voxel_point_cloud(teaser_hip_tsdf* h, int64_t capacity, double* points, double* colors,
                                                  int64_t* count_out) {
  return extract(h, 1, capacity, points, nullptr, colors, count_out);
}

int32_t teaser_hip_tsdf_download(teaser_hip_tsdf* h, float* tsdf_weight, double* color) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (!tsdf_weight && !color) return fail(h, TEASER_HIP_ERR_BAD_ARG, "tsdf_weight and color are both NULL");
  if (color && h->g.color_type == 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "color is given for a volume without colour");
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  const size_t n = (size_t)voxels(h);
  if (!h->out.ensure((color ? 24 : 8) * n)) return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (TSDF download buffer)");
  const TsdfFields v = fields(h);
  hipStream_t s = h->stream;
  if (tsdf_weight) {  // the one buffer serves both parts, in stream order
    launch_tsdf_export(s, h->g, v, h->out.as<float>(), nullptr);
    FCHK(h, hipMemcpyAsync(tsdf_weight, h->out.p, 8 * n, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (TSDF download)");
  }
  if (color) {
    launch_tsdf_export(s, h->g, v, nullptr, h->out.as<double>());
    FCHK(h, hipMemcpyAsync(color, h->out.p, 24 * n, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (TSDF download)");
  }
  FCHK(h, hipGetLastError(), "kernel launch (TSDF download)");
  FCHK(h, hipStreamSynchronize(s), "TSDF download");
  return TEASER_HIP_OK;
}

int32_t teaser_hip_tsdf_upload(teaser_hip_tsdf* h, const float* tsdf_weight, const double* color) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (!tsdf_weight && !color) return fail(h, TEASER_HIP_ERR_BAD_ARG, "tsdf_weight and color are both NULL");
  if (color && h->g.color_type == 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "color is given for a volume without colour");
  const size_t n = (size_t)voxels(h);
  if (tsdf_weight)
    for (size_t k = 0; k < 2 * n; ++k)
      if (!std::isfinite(tsdf_weight[k])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "tsdf_weight has a non-finite value");
  if (color)
    for (size_t k = 0; k < 3 * n; ++k)
      if (!std::isfinite(color[k]) && !(h->g.color_type == 2 && std::isnan(color[k])))  // Gray32 may hold NaN
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "color has a non-finite value");
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  if (!h->out.ensure((color ? 24 : 8) * n)) return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (TSDF upload buffer)");
  const TsdfFields v = fields(h);
  hipStream_t s = h->stream;
  if (tsdf_weight) {
    FCHK(h, hipMemcpyAsync(h->out.p, tsdf_weight, 8 * n, hipMemcpyHostToDevice, s), "hipMemcpyAsync (TSDF upload)");
    launch_tsdf_import(s, h->g, v, h->out.as<float>(), nullptr);
  }
  if (color) {
    FCHK(h, hipMemcpyAsync(h->out.p, color, 24 * n, hipMemcpyHostToDevice, s), "hipMemcpyAsync (TSDF upload)");
    launch_tsdf_import(s, h->g, v, nullptr, h->out.as<double>());
  }
  FCHK(h, hipGetLastError(), "kernel launch (TSDF upload)");
  FCHK(h, hipStreamSynchronize(s), "TSDF upload");
  return TEASER_HIP_OK;
}

}  // extern "C"
