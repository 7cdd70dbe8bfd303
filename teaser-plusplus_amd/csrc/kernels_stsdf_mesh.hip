// kernels_stsdf_mesh.hip -- the triangle mesh of the scalable TSDF volume for gfx950 (include/teaser_hip.h, "Scalable
// TSDF triangle mesh"; device code: stsdf_mesh_device.h; host side: stsdf_mesh.hip; design, bounds and the resource
// report: DESIGN.md section 39).
//
// As in kernels_stsdf.hip a workgroup of 256 is one open block and a thread is a column (x, y) walking z over the block's
// [z][x][y] planes.  cubes: eight lanes look up the blocks b + {0, 1}^3 and leave their addresses in LDS; a column
// carries the sign and weight bits of the layer below in a register and writes one byte per cube.  count: 27 lanes look
// up the blocks b + {-1, 0, 1}^3, the workgroup loads the block's cube bytes with a one-cube halo into LDS (an absent
// block gives zeros), and the creator of every crossed edge of an ACTIVE cube is decided there by comparing ranks; the
// columns' sums are scanned in LDS.  The block totals are scanned by launch_tsdf_scan.  vertices and triangles: a column
// writes its rows from block offset + column offset; a vertex index comes from the bytes, the records and the offsets
// -- no hash, no sort, no atomic.  For vertex normals the open blocks among the 27 round the workgroup's are a directory
// of their own in LDS, so that the trilinear rule's look-ups search at most 27 keys there.
#include "stsdf_mesh_device.h"

namespace thip {

namespace {

// The exclusive sum of `mine` over the 256 columns in s (LDS); *total = the whole sum.
__device__ __forceinline__ int32_t column_scan(int32_t* s, int col, int32_t mine, int32_t* total) {
  s[col] = mine;
  __syncthreads();
  for (int o = 1; o < kStsdfCols; o <<= 1) {  // inclusive Hillis-Steele scan
    const int32_t add = col >= o ? s[col - o] : 0;
    __syncthreads();
    s[col] += add;
    __syncthreads();
  }
  *total = s[kStsdfCols - 1];
  const int32_t before = s[col] - mine;
  __syncthreads();  // s is free again
  return before;
}

// The block's cube bytes with their halo, and the entries of the 27 blocks they come from.
__device__ __forceinline__ void load_halo(const StsdfDir& d, int e, const unsigned char* __restrict__ cubes, int32_t* around,
                                          unsigned char* halo) {
  const int col = (int)threadIdx.x;
  if (col < kStsdfAround) around[col] = stsdf_mesh_around_entry(d, e, col);
  __syncthreads();
  for (int k = col; k < kStsdfHaloBytes; k += kStsdfCols) halo[k] = stsdf_mesh_halo_byte(cubes, around, k);
  __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(kStsdfCols) void stsdf_mesh_cubes_kernel(const StsdfDir d, unsigned char* __restrict__ cubes) {
  __shared__ char* near[kStsdfNear];
  const int e = (int)blockIdx.x, col = (int)threadIdx.x;
  if (col < kStsdfNear) near[col] = stsdf_mesh_near_block(d, e, col);
  __syncthreads();
  stsdf_mesh_column_cubes(near, col / kStsdfU, col % kStsdfU, cubes + (int64_t)e * kStsdfVoxels);
}

__global__ __launch_bounds__(kStsdfCols) void stsdf_mesh_count_kernel(const StsdfDir d, const StsdfMeshScratch m) {
  __shared__ int32_t around[kStsdfAround];
  __shared__ unsigned char halo[kStsdfHaloBytes];
  __shared__ int32_t sum[kStsdfCols];
  const int e = (int)blockIdx.x, col = (int)threadIdx.x;
  load_halo(d, e, m.cubes, around, halo);
  int32_t nv, nt, all_v, all_t;
  stsdf_mesh_column_count(halo, col / kStsdfU, col % kStsdfU, m.records + (int64_t)e * kStsdfVoxels, &nv, &nt);
  m.column_vertices[(int64_t)e * kStsdfCols + col] = column_scan(sum, col, nv, &all_v);
  m.column_triangles[(int64_t)e * kStsdfCols + col] = column_scan(sum, col, nt, &all_t);
  if (col == 0) {
    m.block_vertices[e] = all_v;
    m.block_triangles[e] = all_t;
  }
}

__global__ __launch_bounds__(kStsdfCols) void stsdf_mesh_vertices_kernel(const TsdfGrid g, const StsdfDir d,
                                                                         const StsdfMeshScratch m,
                                                                         const int64_t vertex_capacity,
                                                                         const int64_t triangle_capacity,
                                                                         double* __restrict__ vertices,
                                                                         double* __restrict__ colors,
                                                                         double* __restrict__ normals) {
  __shared__ char* near[kStsdfNear];
  __shared__ int32_t around[kStsdfAround];
  __shared__ uint64_t local_keys[kStsdfAround];
  __shared__ char* local_base[kStsdfAround];
  __shared__ int32_t local_n;
  const int e = (int)blockIdx.x, col = (int)threadIdx.x;
  // the same for every thread of the block
  if (!stsdf_mesh_fits(m.vertex_offsets, m.triangle_offsets, d.n, vertex_capacity, triangle_capacity)) return;
  if (m.vertex_offsets[e + 1] == m.vertex_offsets[e]) return;
  if (col < kStsdfNear) near[col] = stsdf_mesh_near_block(d, e, col);
  if (normals) {  // the blocks a normal can reach, as a directory in LDS: no search of the whole one per corner
    if (col >= 64 && col < 64 + kStsdfAround) around[col - 64] = stsdf_mesh_around_entry(d, e, col - 64);
    __syncthreads();
    if (col == 0) local_n = stsdf_mesh_local_directory(d, around, local_keys, local_base);
  }
  __syncthreads();
  StsdfDir dn = d;
  if (normals) dn.keys = local_keys, dn.base = local_base, dn.n = local_n;
  int b[3];
  stsdf_unkey(d.keys[e], b);
  const int64_t row = m.vertex_offsets[e] + (int64_t)m.column_vertices[(int64_t)e * kStsdfCols + col];
  stsdf_mesh_column_vertices(g, dn, b, near, m.cubes + (int64_t)e * kStsdfVoxels, m.records + (int64_t)e * kStsdfVoxels, row,
                             col / kStsdfU, col % kStsdfU, vertices, colors, normals);
}

__global__ __launch_bounds__(kStsdfCols) void stsdf_mesh_triangles_kernel(const StsdfDir d, const StsdfMeshScratch m,
                                                                          const int64_t vertex_capacity,
                                                                          const int64_t triangle_capacity,
                                                                          int32_t* __restrict__ triangles) {
  __shared__ int32_t around[kStsdfAround];
  __shared__ unsigned char halo[kStsdfHaloBytes];
  const int e = (int)blockIdx.x, col = (int)threadIdx.x;
  // the same for every thread of the block
  if (!stsdf_mesh_fits(m.vertex_offsets, m.triangle_offsets, d.n, vertex_capacity, triangle_capacity)) return;
  if (m.triangle_offsets[e + 1] == m.triangle_offsets[e]) return;
  load_halo(d, e, m.cubes, around, halo);
  const int64_t row = m.triangle_offsets[e] + (int64_t)m.column_triangles[(int64_t)e * kStsdfCols + col];
  stsdf_mesh_column_triangles(halo, around, m.records, m.column_vertices, m.vertex_offsets, row, col / kStsdfU,
                              col % kStsdfU, triangles);
}

void launch_stsdf_mesh_cubes(hipStream_t s, const StsdfDir& d, unsigned char* d_cubes) {
  hipLaunchKernelGGL(stsdf_mesh_cubes_kernel, dim3((unsigned)d.n), dim3(kStsdfCols), 0, s, d, d_cubes);
}

void launch_stsdf_mesh_count(hipStream_t s, const StsdfDir& d, const StsdfMeshScratch& m) {
  hipLaunchKernelGGL(stsdf_mesh_count_kernel, dim3((unsigned)d.n), dim3(kStsdfCols), 0, s, d, m);
}

void launch_stsdf_mesh_vertices(hipStream_t s, const TsdfGrid& g, const StsdfDir& d, const StsdfMeshScratch& m,
                                int64_t vertex_capacity, int64_t triangle_capacity, double* d_vertices, double* d_colors,
                                double* d_normals) {
  hipLaunchKernelGGL(stsdf_mesh_vertices_kernel, dim3((unsigned)d.n), dim3(kStsdfCols), 0, s, g, d, m, vertex_capacity,
                     triangle_capacity, d_vertices, d_colors, d_normals);
}

void launch_stsdf_mesh_triangles(hipStream_t s, const StsdfDir& d, const StsdfMeshScratch& m, int64_t vertex_capacity,
                                 int64_t triangle_capacity, int32_t* d_triangles) {
  hipLaunchKernelGGL(stsdf_mesh_triangles_kernel, dim3((unsigned)d.n), dim3(kStsdfCols), 0, s, d, m, vertex_capacity,
                     triangle_capacity, d_triangles);
}

}  // namespace thip
