// stsdf_raycast.hip -- host side of the ray cast of the scalable TSDF volume (include/teaser_hip.h, "Scalable TSDF ray
// casting"): the entry checks, the cameras, the layout of a call and its one round trip.  Kernel:
// kernels_stsdf_raycast.hip; device code: stsdf_raycast_device.h; the checks, records and layout are the dense ray
// cast's (tsdf_raycast_host.h); design, bounds and the resource report: DESIGN.md section 38.
//
// A call: the directory's device copy is brought up to date if blocks were opened since it was made
// (stsdf_sync_directory); the view records and the block map go up in one copy; one launch over the blocks of all views
// writes the blocks' hit counts and the requested maps of every pixel into one buffer; one copy brings that buffer back
// into the handle's page-locked buffer, one synchronisation, and the host hands every map to its caller's array and adds
// the counts.  Neither the launch nor the synchronisation depends on the data.  The buffers are those the other calls of
// the handle use (in, stage, out, back), which teaser_hip_stsdf_fill_scratch covers.
#include "stsdf_internal.h"
#include "stsdf_raycast_device.h"
#include "tsdf_raycast_host.h"

using namespace thip;

extern "C" {

int32_t teaser_hip_stsdf_ray_cast_views(teaser_hip_stsdf* h, int32_t n_views, const teaser_tsdf_view_c* views,
                                        float* const* depth, float* const* vertex, float* const* normal,
                                        float* const* color, int64_t* hit_counts) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (n_views < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_views must be >= 0");
  if (n_views == 0) return TEASER_HIP_OK;
  if (!views) return fail(h, TEASER_HIP_ERR_BAD_ARG, "views must not be NULL");
  const TsdfGrid& g = h->g;
  RayPlan p;
  const double origin[3] = {0.0, 0.0, 0.0};
  const int32_t rc = ray_plan(h, g.color_type, origin, n_views, views, color, hit_counts, &p);
  if (rc != TEASER_HIP_OK) return rc;
  if (p.n_blocks == 0) return TEASER_HIP_OK;  // no pixel
  for (TsdfRayView& d : p.rec) {  // the step cap, in double: the loop ends whatever the floats do
    const double steps = floor(((double)d.dmax - (double)d.dmin) / (double)g.vl_f) + 2.0;
    d.n_cap = steps < (double)kStsdfRayMaxSteps ? (int32_t)steps : kStsdfRayMaxSteps;  // a NaN takes the cap
  }
  ray_layout(n_views, depth, vertex, normal, color, &p);
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  // every allocation first: once the directory's upload is enqueued nothing below returns without the synchronisation
  // but a failed HIP call, so no later call finds that copy still reading the staging buffer
  if (!h->in.ensure(p.in_bytes) || !h->stage.ensure(p.in_bytes) || !h->out.ensure(p.o_end) || !h->back.ensure(p.o_end))
    return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (scalable TSDF ray cast buffers)");
  StsdfDir dir;
  const int32_t rc_dir = stsdf_sync_directory(h, &dir);
  if (rc_dir != TEASER_HIP_OK) return rc_dir;
  ray_stage(p, h->stage.as<char>());
  hipStream_t s = h->stream;
  FCHK(h, hipMemcpyAsync(h->in.p, h->stage.p, p.in_bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync (scalable TSDF views)");
  StsdfRayArgs a;
  memset(&a, 0, sizeof(a));
  a.views = h->in.as<TsdfRayView>();
  a.blk_view = reinterpret_cast<const int32_t*>(h->in.as<char>() + p.o_map_in);
  a.out = reinterpret_cast<float*>(h->out.as<char>() + p.o_maps);
  a.blk_hits = h->out.as<int32_t>();
  a.ul_f = (float)h->ul;
  launch_stsdf_raycast(s, g, dir, a, (int32_t)p.n_blocks);
  FCHK(h, hipGetLastError(), "kernel launch (scalable TSDF ray cast)");
  FCHK(h, hipMemcpyAsync(h->back.p, h->out.p, p.o_end, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (scalable TSDF ray cast)");
  FCHK(h, hipStreamSynchronize(s), "scalable TSDF ray cast");
  ray_hand_out(p, h->back.as<char>(), depth, vertex, normal, color, hit_counts);
  return TEASER_HIP_OK;
}

}  // extern "C"
