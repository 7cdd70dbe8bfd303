// tsdf_raycast.hip -- host side of the ray cast of the TSDF volume (include/teaser_hip.h, "TSDF ray casting"): the entry
// checks, the cameras, the layout of a call and its one round trip.  Kernel: kernels_tsdf_raycast.hip; device code:
// tsdf_raycast_device.h; the checks, records and layout it shares with the scalable volume's ray cast:
// tsdf_raycast_host.h; design, bounds and the resource report: DESIGN.md section 35.
//
// A call: the view records and the block map go up in one copy; one launch over the blocks of all views writes the
// blocks' hit counts and the requested maps of every pixel into one buffer; one copy brings that buffer back into the
// handle's page-locked buffer, one synchronisation, and the host hands every map to its caller's array and adds the
// counts.  Neither the launch nor the synchronisation depends on the data.
#include "tsdf_raycast_host.h"

using namespace thip;

extern "C" {

int32_t teaser_hip_tsdf_view_default(teaser_tsdf_view_c* w) {
  if (!w) return TEASER_HIP_ERR_BAD_ARG;
  memset(w, 0, sizeof(*w));
  for (int k = 0; k < 4; ++k) w->extrinsic[5 * k] = 1.0;
  w->depth_min = 0.1;
  w->depth_max = 3.0;
  w->weight_threshold = 3.0;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_tsdf_ray_cast_views(teaser_hip_tsdf* h, int32_t n_views, const teaser_tsdf_view_c* views,
                                       float* const* depth, float* const* vertex, float* const* normal,
                                       float* const* color, int64_t* hit_counts) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (n_views < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_views must be >= 0");
  if (n_views == 0) return TEASER_HIP_OK;
  if (!views) return fail(h, TEASER_HIP_ERR_BAD_ARG, "views must not be NULL");
  const TsdfGrid& g = h->g;
  RayPlan p;
  const int32_t rc = ray_plan(h, g.color_type, g.origin, n_views, views, color, hit_counts, &p);
  if (rc != TEASER_HIP_OK) return rc;
  if (p.n_blocks == 0) return TEASER_HIP_OK;  // no pixel
  ray_layout(n_views, depth, vertex, normal, color, &p);
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  if (!h->in.ensure(p.in_bytes) || !h->stage.ensure(p.in_bytes) || !h->out.ensure(p.o_end) || !h->back.ensure(p.o_end))
    return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (TSDF ray cast buffers)");
  ray_stage(p, h->stage.as<char>());
  hipStream_t s = h->stream;
  FCHK(h, hipMemcpyAsync(h->in.p, h->stage.p, p.in_bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync (TSDF views)");
  TsdfRayArgs a;
  memset(&a, 0, sizeof(a));
  a.views = h->in.as<TsdfRayView>();
  a.blk_view = reinterpret_cast<const int32_t*>(h->in.as<char>() + p.o_map_in);
  a.out = reinterpret_cast<float*>(h->out.as<char>() + p.o_maps);
  a.blk_hits = h->out.as<int32_t>();
  a.L_f = (float)h->vol.length;
  launch_tsdf_raycast(s, g, fields(h), a, (int32_t)p.n_blocks);
  FCHK(h, hipGetLastError(), "kernel launch (TSDF ray cast)");
  FCHK(h, hipMemcpyAsync(h->back.p, h->out.p, p.o_end, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (TSDF ray cast)");
  FCHK(h, hipStreamSynchronize(s), "TSDF ray cast");
  ray_hand_out(p, h->back.as<char>(), depth, vertex, normal, color, hit_counts);
  return TEASER_HIP_OK;
}

}  // extern "C"
