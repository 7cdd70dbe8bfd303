// tsdf_mesh.hip -- host side of the triangle mesh of the TSDF volume (include/teaser_hip.h, "TSDF volume", the triangle
// mesh): the entry checks, the scratch on the handle and the one round trip.  Kernels: kernels_tsdf_mesh.hip; device
// code and the tables: tsdf_mesh_device.h; design, bounds and the resource report: DESIGN.md section 34.
//
// A call: cubes, count and scan; the two totals land in front of the output buffer; then the vertex pass and the
// triangle pass into buffers of the capacities given (each does nothing when a total exceeds its capacity or a vertex
// index would not fit int32), the totals and the rows copied back, one synchronisation; the host then hands over exactly
// the counted rows.  Neither the launches nor the synchronisation depend on the data.
#include <string.h>

#include <algorithm>
#include <string>

#include "tsdf_internal.h"
#include "tsdf_mesh_device.h"

using namespace thip;

extern "C" {

int32_t teaser_hip_tsdf_extract_triangle_mesh(teaser_hip_tsdf* h, int64_t vertex_capacity, double* vertices,
                                              double* vertex_colors, double* vertex_normals, int64_t triangle_capacity,
                                              int32_t* triangles, int64_t* vertex_count_out, int64_t* triangle_count_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (!vertex_count_out || !triangle_count_out)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "vertex_count_out and triangle_count_out must not be NULL");
  if (vertex_capacity < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "vertex_capacity must be >= 0");
  if (triangle_capacity < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "triangle_capacity must be >= 0");
  if (vertex_capacity > 0 && !vertices)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "vertices must not be NULL with a vertex_capacity above 0");
  if (triangle_capacity > 0 && !triangles)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "triangles must not be NULL with a triangle_capacity above 0");
  if (vertex_colors && h->g.color_type == 0)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "vertex_colors is given for a volume without colour");
  const TsdfGrid& g = h->g;
  const int64_t n = voxels(h), plane = (int64_t)g.R * g.R;
  const int64_t vcap = std::min<int64_t>(vertex_capacity, 3 * n), tcap = std::min<int64_t>(triangle_capacity, 5 * n);
  const bool want_c = vcap > 0 && vertex_colors, want_n = vcap > 0 && vertex_normals;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  // scratch: a byte and a record per voxel, two sums and two offsets per column
  const size_t o_records = round_up((size_t)n, 256), o_counts = o_records + round_up(sizeof(uint32_t) * (size_t)n, 256);
  const size_t o_offsets = o_counts + round_up(sizeof(int32_t) * 2 * (size_t)plane, 256);
  const size_t scratch = o_offsets + sizeof(int64_t) * 2 * (size_t)(plane + 1);
  // output: the totals, the vertex rows, their colours and normals, the triangle rows
  const size_t row = sizeof(double) * 3 * (size_t)vcap;
  const size_t o_vert = round_up(2 * sizeof(int64_t), 256), o_col = o_vert + row, o_norm = o_col + (want_c ? row : 0);
  const size_t o_tri = o_norm + (want_n ? row : 0), o_end = o_tri + sizeof(int32_t) * 3 * (size_t)tcap;
  if (!h->mesh.ensure(scratch) || !h->out.ensure(o_end) || !h->back.ensure(o_end))
    return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (TSDF triangle mesh buffers)");
  hipStream_t s = h->stream;
  const TsdfFields v = fields(h);
  unsigned char* cubes = h->mesh.as<unsigned char>();
  uint32_t* records = reinterpret_cast<uint32_t*>(h->mesh.as<char>() + o_records);
  int32_t* counts = reinterpret_cast<int32_t*>(h->mesh.as<char>() + o_counts);
  int64_t* offsets = reinterpret_cast<int64_t*>(h->mesh.as<char>() + o_offsets);
  char* out = h->out.as<char>();
  int64_t* totals = reinterpret_cast<int64_t*>(out);
  launch_tsdf_mesh_cubes(s, g, v, cubes);
  launch_tsdf_mesh_count(s, g, cubes, records, counts, offsets, totals);
  if (vcap > 0)
    launch_tsdf_mesh_vertices(s, g, v, cubes, records, offsets, totals, vcap, tcap, reinterpret_cast<double*>(out + o_vert),
                              want_c ? reinterpret_cast<double*>(out + o_col) : nullptr,
                              want_n ? reinterpret_cast<double*>(out + o_norm) : nullptr);
  if (tcap > 0)
    launch_tsdf_mesh_triangles(s, g, cubes, records, offsets, totals, vcap, tcap, reinterpret_cast<int32_t*>(out + o_tri));
  FCHK(h, hipGetLastError(), "kernel launch (TSDF triangle mesh)");
  FCHK(h, hipMemcpyAsync(h->back.p, out, vcap > 0 || tcap > 0 ? o_end : 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s),
       "hipMemcpyAsync (TSDF triangle mesh)");
  FCHK(h, hipStreamSynchronize(s), "TSDF triangle mesh");
  const char* back = h->back.as<char>();
  int64_t count[2] = {0, 0};
  memcpy(count, back, sizeof(count));
  *vertex_count_out = count[0];
  *triangle_count_out = count[1];
  if (count[0] > 2147483647)
    return fail(h, TEASER_HIP_ERR_BAD_ARG,
                "the vertex count " + std::to_string(count[0]) + " is above 2147483647, the largest int32 index");
  if (vertex_capacity == 0 && !vertices && triangle_capacity == 0 && !triangles) return TEASER_HIP_OK;  // the counts alone
  if (count[0] > vertex_capacity || count[1] > triangle_capacity)
    return fail(h, TEASER_HIP_ERR_BAD_ARG,
                "a capacity is below its count: vertex_capacity " + std::to_string(vertex_capacity) + ", vertex count " +
                    std::to_string(count[0]) + "; triangle_capacity " + std::to_string(triangle_capacity) +
                    ", triangle count " + std::to_string(count[1]));
  const size_t bytes = sizeof(double) * 3 * (size_t)count[0];
  if (bytes > 0) {
    memcpy(vertices, back + o_vert, bytes);
    if (want_c) memcpy(vertex_colors, back + o_col, bytes);
    if (want_n) memcpy(vertex_normals, back + o_norm, bytes);
  }
  if (count[1] > 0) memcpy(triangles, back + o_tri, sizeof(int32_t) * 3 * (size_t)count[1]);
  return TEASER_HIP_OK;
}

int32_t teaser_hip_tsdf_mesh_tables(int32_t edge_table[256], int8_t tri_table[4096]) {
  if (!edge_table || !tri_table) return TEASER_HIP_ERR_BAD_ARG;
  for (int c = 0; c < 256; ++c) edge_table[c] = tsdf_edge_mask(c);
  memcpy(tri_table, kTsdfTriTable, sizeof(kTsdfTriTable));
  return TEASER_HIP_OK;
}

}  // extern "C"
