// stsdf_mesh.hip -- host side of the triangle mesh of the scalable TSDF volume (include/teaser_hip.h, "Scalable TSDF
// triangle mesh"): the entry checks, the scratch on the handle and the one round trip.  Kernels: kernels_stsdf_mesh.hip;
// device code: stsdf_mesh_device.h; design, bounds and the resource report: DESIGN.md section 39.
//
// A call over n open blocks: with n = 0 the two scans alone (they write the two zeros); else cubes, count, the two scans
// of the block totals, and then the vertex pass and the triangle pass into buffers of the capacities given (each does
// nothing when a total exceeds its capacity or a vertex index would not fit int32), so 4 launches for the counts alone
// and 6 for the rows.  The totals land in front of the output buffer and come back with the rows, one synchronisation;
// the host then hands over exactly the counted rows.  The launches depend on the data only through whether a block is
// open.
#include <string.h>

#include <algorithm>
#include <string>

#include "stsdf_internal.h"
#include "stsdf_mesh_device.h"

using namespace thip;

extern "C" {

int32_t teaser_hip_stsdf_extract_triangle_mesh(teaser_hip_stsdf* h, int64_t vertex_capacity, double* vertices,
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
  const int64_t nb = (int64_t)h->keys.size(), n = nb * kStsdfVoxels;
  // no more rows can exist: a vertex lies on an edge whose base voxel is in an open block, a cube has at most 5 triangles
  const int64_t vcap = std::min<int64_t>(vertex_capacity, 3 * n), tcap = std::min<int64_t>(triangle_capacity, 5 * n);
  const bool want_c = vcap > 0 && vertex_colors, want_n = vcap > 0 && vertex_normals;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  // scratch: a byte and a record per voxel, two offsets per column, two totals and two offsets per block
  const size_t blocks = (size_t)std::max<int64_t>(nb, 1);
  const size_t o_records = round_up(blocks * kStsdfVoxels, 256);
  const size_t o_colv = o_records + sizeof(uint32_t) * blocks * kStsdfVoxels;
  const size_t o_colt = o_colv + sizeof(int32_t) * blocks * kStsdfCols;
  const size_t o_blkv = o_colt + sizeof(int32_t) * blocks * kStsdfCols;
  const size_t o_blkt = o_blkv + round_up(sizeof(int32_t) * blocks, 256);
  const size_t o_offv = o_blkt + round_up(sizeof(int32_t) * blocks, 256);
  const size_t o_offt = o_offv + round_up(sizeof(int64_t) * (blocks + 1), 256);
  const size_t scratch = o_offt + sizeof(int64_t) * (blocks + 1);
  // output: the totals, the vertex rows, their colours and normals, the triangle rows
  const size_t row = sizeof(double) * 3 * (size_t)vcap;
  const size_t o_vert = round_up(2 * sizeof(int64_t), 256), o_col = o_vert + row, o_norm = o_col + (want_c ? row : 0);
  const size_t o_tri = o_norm + (want_n ? row : 0), o_end = o_tri + sizeof(int32_t) * 3 * (size_t)tcap;
  if (!h->mesh.ensure(scratch) || !h->out.ensure(o_end) || !h->back.ensure(o_end))
    return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (scalable TSDF triangle mesh buffers)");
  StsdfDir d;
  const int32_t rc = stsdf_sync_directory(h, &d);
  if (rc != TEASER_HIP_OK) return rc;
  hipStream_t s = h->stream;
  char* w = h->mesh.as<char>();
  StsdfMeshScratch m;
  m.cubes = reinterpret_cast<unsigned char*>(w);
  m.records = reinterpret_cast<uint32_t*>(w + o_records);
  m.column_vertices = reinterpret_cast<int32_t*>(w + o_colv);
  m.column_triangles = reinterpret_cast<int32_t*>(w + o_colt);
  m.block_vertices = reinterpret_cast<int32_t*>(w + o_blkv);
  m.block_triangles = reinterpret_cast<int32_t*>(w + o_blkt);
  m.vertex_offsets = reinterpret_cast<int64_t*>(w + o_offv);
  m.triangle_offsets = reinterpret_cast<int64_t*>(w + o_offt);
  char* out = h->out.as<char>();
  if (nb > 0) {
    launch_stsdf_mesh_cubes(s, d, m.cubes);
    launch_stsdf_mesh_count(s, d, m);
  }
  launch_tsdf_scan(s, m.block_vertices, nb, m.vertex_offsets);
  launch_tsdf_scan(s, m.block_triangles, nb, m.triangle_offsets);
  FCHK(h, hipMemcpyAsync(out, m.vertex_offsets + nb, sizeof(int64_t), hipMemcpyDeviceToDevice, s),
       "hipMemcpyAsync (vertex count)");
  FCHK(h, hipMemcpyAsync(out + sizeof(int64_t), m.triangle_offsets + nb, sizeof(int64_t), hipMemcpyDeviceToDevice, s),
       "hipMemcpyAsync (triangle count)");
  if (vcap > 0)
    launch_stsdf_mesh_vertices(s, h->g, d, m, vcap, tcap, reinterpret_cast<double*>(out + o_vert),
                               want_c ? reinterpret_cast<double*>(out + o_col) : nullptr,
                               want_n ? reinterpret_cast<double*>(out + o_norm) : nullptr);
  if (tcap > 0) launch_stsdf_mesh_triangles(s, d, m, vcap, tcap, reinterpret_cast<int32_t*>(out + o_tri));
  FCHK(h, hipGetLastError(), "kernel launch (scalable TSDF triangle mesh)");
  FCHK(h, hipMemcpyAsync(h->back.p, out, vcap > 0 || tcap > 0 ? o_end : 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s),
       "hipMemcpyAsync (scalable TSDF triangle mesh)");
  FCHK(h, hipStreamSynchronize(s), "scalable TSDF triangle mesh");
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

}  // extern "C"
