// stsdf_mesh_device.h -- the per-cube rules of the triangle mesh of the scalable TSDF volume (include/teaser_hip.h,
// "Scalable TSDF triangle mesh"; kernels: kernels_stsdf_mesh.hip, host side: stsdf_mesh.hip, design: DESIGN.md section
// 39): the layers of a cube column that runs on into the blocks b + {0, 1}^3, a block's cube bytes with the one-cube halo
// of its 26 neighbours, the rank of a cube, which cube creates the vertex of a lattice edge, what a column counts, and the
// vertex and triangle rows a column writes.  The tables, the edge mask and the byte of a cube are those of
// tsdf_mesh_device.h; the directory look-up, a block's fields and the normal are those of stsdf_device.h.  Nothing here
// uses a wave operation or declares LDS, so tests/stsdf_mesh_host_driver.cpp runs this very source in serial loops.
//
// Every block other than the workgroup's own is reached through a pointer or a directory entry that may say "absent";
// each is tested before every load.
#pragma once

#include "stsdf_device.h"
#include "tsdf_mesh_device.h"

namespace thip {

constexpr int kStsdfHalo = kStsdfU + 2;                              // a block's cubes and one cube on either side
constexpr int kStsdfHaloBytes = kStsdfHalo * kStsdfHalo * kStsdfHalo;  // 5 832
constexpr int kStsdfNear = 8;                                        // the blocks b + {0, 1}^3
constexpr int kStsdfAround = 27;                                     // the blocks b + {-1, 0, 1}^3

// The number the edge along `axis` with base voxel c + du e_u + dv e_v has in cube c (u < v the other two axes).
constexpr int8_t kStsdfEdgeSlot[3][2][2] = {{{0, 4}, {2, 6}}, {{3, 7}, {1, 5}}, {{8, 11}, {9, 10}}};

// Where block (bx, by, bz) stands in the directory; -1 when it is not open (or outside the index range).
__host__ __device__ __forceinline__ int32_t stsdf_mesh_find_entry(const StsdfDir& d, int64_t bx, int64_t by, int64_t bz) {
  const int64_t L = -(int64_t)kStsdfBias, H = kStsdfBias;
  if (bx < L || bx >= H || by < L || by >= H || bz < L || bz >= H) return -1;
  const uint64_t key = stsdf_key((int)bx, (int)by, (int)bz);
  int lo = 0, hi = d.n;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (d.keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < d.n && d.keys[lo] == key ? lo : -1;
}

// Block b + (k >> 2 & 1, k >> 1 & 1, k & 1) of directory entry e, k = 0 .. 7; NULL when it is not open.
__host__ __device__ __forceinline__ char* stsdf_mesh_near_block(const StsdfDir& d, int e, int k) {
  if (k == 0) return d.base[e];
  int b[3];
  stsdf_unkey(d.keys[e], b);
  return stsdf_find(d, (int64_t)b[0] + ((k >> 2) & 1), (int64_t)b[1] + ((k >> 1) & 1), (int64_t)b[2] + (k & 1));
}

// The entry of block b + (k / 9 - 1, k / 3 % 3 - 1, k % 3 - 1) of directory entry e, k = 0 .. 26; -1 when it is not open.
__host__ __device__ __forceinline__ int32_t stsdf_mesh_around_entry(const StsdfDir& d, int e, int k) {
  if (k == 13) return e;
  int b[3];
  stsdf_unkey(d.keys[e], b);
  return stsdf_mesh_find_entry(d, (int64_t)b[0] + (k / 9 - 1), (int64_t)b[1] + ((k / 3) % 3 - 1), (int64_t)b[2] + (k % 3 - 1));
}

// The open blocks among the 27 of around[] as a directory of their own, in ascending key order (the order of around[]);
// returns their number.  The normal of a vertex of block b reads voxels with local indices in [-1, 18] only (a vertex
// lies within [0, 16] voxels of the block's corner and the rule steps 0.99 of a voxel to either side), so stsdf_find
// over these at most 27 keys finds what it finds in the whole directory, in five steps instead of log2(n).
__host__ __device__ __forceinline__ int32_t stsdf_mesh_local_directory(const StsdfDir& d, const int32_t* around,
                                                                       uint64_t* keys, char** base) {
  int32_t n = 0;
  for (int k = 0; k < kStsdfAround; ++k) {
    if (around[k] < 0) continue;
    keys[n] = d.keys[around[k]];
    base[n] = d.base[around[k]];
    ++n;
  }
  return n;
}

// Which of the 27 blocks the cube or voxel with the local index (x, y, z) in [-1, 16]^3 lies in.
__host__ __device__ __forceinline__ int stsdf_mesh_around(int x, int y, int z) {
  return (((x >> 4) + 1) * 3 + ((y >> 4) + 1)) * 3 + ((z >> 4) + 1);
}

// Layer z (0 .. 16) of the four voxel columns round cube column (x, y) of a block, in the order of corners 0 .. 3: bits
// 0 .. 3 tsdf < 0.0f, bits 4 .. 7 weight != 0.  near[k] are the blocks b + {0, 1}^3; a voxel of a block that is not open
// has tsdf 0 and weight 0.
__host__ __device__ __forceinline__ int stsdf_mesh_layer(char* const* near, int x, int y, int z) {
  int bits = 0;
  for (int i = 0; i < 4; ++i) {
    const int vx = x + tsdf_corner_x(i), vy = y + tsdf_corner_y(i);
    const char* base = near[((vx >> 4) << 2) | ((vy >> 4) << 1) | (z >> 4)];
    if (!base) continue;
    const float* tsdf = reinterpret_cast<const float*>(base);
    const int64_t at = tsdf_index(kStsdfU, vx & 15, vy & 15, z & 15);
    bits |= (tsdf[at] < 0.0f ? 1 : 0) << i;
    bits |= (tsdf[kStsdfVoxels + at] != 0.0f ? 16 : 0) << i;
  }
  return bits;
}

// The cubes pass of column (x, y) of a block: the bytes of its sixteen cubes, at cubes[(z 16 + x) 16 + y].
__host__ __device__ __forceinline__ void stsdf_mesh_column_cubes(char* const* near, int x, int y, unsigned char* cubes) {
  int lower = stsdf_mesh_layer(near, x, y, 0);
  for (int z = 0; z < kStsdfU; ++z) {
    const int upper = stsdf_mesh_layer(near, x, y, z + 1);
    cubes[tsdf_index(kStsdfU, x, y, z)] = tsdf_cube_byte(lower, upper);
    lower = upper;
  }
}

// Where cube (x, y, z), each in [-1, 16], lies in the halo.
__host__ __device__ __forceinline__ int stsdf_mesh_halo_at(int x, int y, int z) {
  return ((z + 1) * kStsdfHalo + (x + 1)) * kStsdfHalo + (y + 1);
}

// Byte k of a block's halo: the byte of the cube there, 0 in a block that is not open.  cubes holds 4096 bytes per
// directory entry; around[27] are the entries of the blocks b + {-1, 0, 1}^3.
__host__ __device__ __forceinline__ unsigned char stsdf_mesh_halo_byte(const unsigned char* cubes, const int32_t* around,
                                                                       int k) {
  const int z = k / (kStsdfHalo * kStsdfHalo) - 1, x = (k / kStsdfHalo) % kStsdfHalo - 1, y = k % kStsdfHalo - 1;
  const int32_t entry = around[stsdf_mesh_around(x, y, z)];
  if (entry < 0) return 0;
  return cubes[(int64_t)entry * kStsdfVoxels + tsdf_index(kStsdfU, x & 15, y & 15, z & 15)];
}

// rank(cube) among the cubes of the 27 blocks: the blocks in ascending (bx, by, bz) -- the order of the directory --
// and (lx 16 + ly) 16 + lz inside.
__host__ __device__ __forceinline__ int stsdf_mesh_rank(int x, int y, int z) {
  return stsdf_mesh_around(x, y, z) * kStsdfVoxels + (((x & 15) * kStsdfU + (y & 15)) * kStsdfU + (z & 15));
}

// The CREATOR of the vertex on edge i (crossed) of the ACTIVE cube (x, y, z) of a block: the ACTIVE cube of smallest
// rank among the four that contain the edge, and the number the edge has there.
__host__ __device__ __forceinline__ void stsdf_mesh_creator(const unsigned char* halo, int x, int y, int z, int i, int* c,
                                                            int* slot) {
  const int a = kTsdfEdgeCorner[i][0], axis = kTsdfEdgeAxis[i];
  const int h[3] = {x + tsdf_corner_x(a), y + tsdf_corner_y(a), z + tsdf_corner_z(a)};  // the base voxel of the edge
  const int u = axis == 0 ? 1 : 0, v = axis == 2 ? 1 : 2;
  int best = 0x7fffffff;
  c[0] = x, c[1] = y, c[2] = z, *slot = i;
  for (int du = 0; du < 2; ++du)
    for (int dv = 0; dv < 2; ++dv) {
      int q[3] = {h[0], h[1], h[2]};
      q[u] -= du, q[v] -= dv;  // in [-1, 16]: the halo has it
      if (halo[stsdf_mesh_halo_at(q[0], q[1], q[2])] == 0) continue;
      const int r = stsdf_mesh_rank(q[0], q[1], q[2]);
      if (r < best) best = r, c[0] = q[0], c[1] = q[1], c[2] = q[2], *slot = kStsdfEdgeSlot[axis][du][dv];
    }
}

// The slots the ACTIVE cube (x, y, z) creates: the crossed edges it is the creator of.
__host__ __device__ __forceinline__ int stsdf_mesh_created(const unsigned char* halo, int x, int y, int z, int cube_index) {
  const int crossed = tsdf_edge_mask(cube_index);
  int created = 0;
  for (int i = 0; i < 12; ++i) {
    if (!((crossed >> i) & 1)) continue;
    int c[3], slot;
    stsdf_mesh_creator(halo, x, y, z, i, c, &slot);
    if (c[0] == x && c[1] == y && c[2] == z) created |= 1 << i;
  }
  return created;
}

// The count pass of column (x, y) of a block: per ACTIVE cube the record (created slots << 16) | (vertices the column's
// earlier cubes create, at most 12 x 16); *n_vertices and *n_triangles are the column's sums.  records: the block's 4096.
__host__ __device__ __forceinline__ void stsdf_mesh_column_count(const unsigned char* halo, int x, int y, uint32_t* records,
                                                                 int32_t* n_vertices, int32_t* n_triangles) {
  int32_t nv = 0, nt = 0;
  for (int z = 0; z < kStsdfU; ++z) {
    const int cube_index = halo[stsdf_mesh_halo_at(x, y, z)];
    if (cube_index == 0) continue;
    const int created = stsdf_mesh_created(halo, x, y, z, cube_index);
    records[tsdf_index(kStsdfU, x, y, z)] = ((uint32_t)created << 16) | (uint32_t)nv;
    nv += __builtin_popcount((unsigned)created);
    nt += tsdf_cube_triangles(cube_index);
  }
  *n_vertices = nv;
  *n_triangles = nt;
}

// The vertex on edge i of cube (x, y, z) of block b: position and, where the pointers are given, colour and normal.  The
// position is formed from the global voxel index 16 b + l of the edge's base voxel; no origin is added.  d is the
// directory the normal searches: the whole one or stsdf_mesh_local_directory's.
__host__ __device__ __forceinline__ void stsdf_mesh_vertex(const TsdfGrid& g, const StsdfDir& d, const int* b,
                                                           char* const* near, int x, int y, int z, int i, double* vertex,
                                                           double* color, double* normal) {
  const int ca = kTsdfEdgeCorner[i][0], cb = kTsdfEdgeCorner[i][1], axis = kTsdfEdgeAxis[i];
  const int va[3] = {x + tsdf_corner_x(ca), y + tsdf_corner_y(ca), z + tsdf_corner_z(ca)};
  const int vb[3] = {x + tsdf_corner_x(cb), y + tsdf_corner_y(cb), z + tsdf_corner_z(cb)};
  char* base0 = near[((va[0] >> 4) << 2) | ((va[1] >> 4) << 1) | (va[2] >> 4)];
  char* base1 = near[((vb[0] >> 4) << 2) | ((vb[1] >> 4) << 1) | (vb[2] >> 4)];
  const int64_t at0 = tsdf_index(kStsdfU, va[0] & 15, va[1] & 15, va[2] & 15);
  const int64_t at1 = tsdf_index(kStsdfU, vb[0] & 15, vb[1] & 15, vb[2] & 15);
  const double f0 = base0 ? __builtin_fabs((double)reinterpret_cast<const float*>(base0)[at0]) : 0.0;
  const double f1 = base1 ? __builtin_fabs((double)reinterpret_cast<const float*>(base1)[at1]) : 0.0;
  const double den = f0 + f1;
  double p[3];
  for (int k = 0; k < 3; ++k) p[k] = g.half + g.vl * (double)(kStsdfU * b[k] + va[k]);
  const double step = (f0 * g.vl) / den;
  for (int k = 0; k < 3; ++k)
    if (k == axis) p[k] = p[k] + step;
  for (int k = 0; k < 3; ++k) vertex[k] = p[k];
  if (color) {
    const double* col0 = base0 ? stsdf_fields(base0, g.color_type).color : nullptr;
    const double* col1 = base1 ? stsdf_fields(base1, g.color_type).color : nullptr;
    for (int k = 0; k < 3; ++k) {
      double c0 = col0 ? col0[k * kStsdfVoxels + at0] : 0.0, c1 = col1 ? col1[k * kStsdfVoxels + at1] : 0.0;
      if (g.color_type == 1) c0 = c0 / 255.0, c1 = c1 / 255.0;
      const double c = (f1 * c0 + f0 * c1) / den;
      color[k] = g.color_type == 2 ? rgbd_canonical(c) : c;
    }
  }
  if (normal) stsdf_normal_at(g, d, b, reinterpret_cast<const float*>(near[0]), p, normal);
}

// Whether rows may be written: both totals fit their capacities and a vertex index fits int32.
__host__ __device__ __forceinline__ bool stsdf_mesh_fits(const int64_t* vertex_offsets, const int64_t* triangle_offsets,
                                                         int32_t n_blocks, int64_t vertex_capacity,
                                                         int64_t triangle_capacity) {
  const int64_t totals[2] = {vertex_offsets[n_blocks], triangle_offsets[n_blocks]};
  return tsdf_mesh_fits(totals, vertex_capacity, triangle_capacity);
}

// The vertex pass of column (x, y) of block b: its created vertices from `row`, cubes by z, slots ascending.  cubes and
// records: the block's 4096; d: the directory the normals search.
__host__ __device__ __forceinline__ void stsdf_mesh_column_vertices(const TsdfGrid& g, const StsdfDir& d, const int* b,
                                                                    char* const* near, const unsigned char* cubes,
                                                                    const uint32_t* records, int64_t row, int x, int y,
                                                                    double* vertices, double* colors, double* normals) {
  for (int z = 0; z < kStsdfU; ++z) {
    const int64_t at = tsdf_index(kStsdfU, x, y, z);
    if (cubes[at] == 0) continue;
    const uint32_t record = records[at];
    int64_t r = row + (int64_t)(record & 0xffffu);
    for (int i = 0; i < 12; ++i) {
      if (!((record >> (16 + i)) & 1u)) continue;
      stsdf_mesh_vertex(g, d, b, near, x, y, z, i, vertices + 3 * r, colors ? colors + 3 * r : nullptr,
                        normals ? normals + 3 * r : nullptr);
      ++r;
    }
  }
}

// The index of the vertex on edge i (crossed) of the ACTIVE cube (x, y, z) of a block: the creator's block offset, the
// creator's column offset, the creator's count within its column and the rank of the slot among the slots the creator
// creates.  records: 4096 per directory entry; column_offsets: 256 per directory entry.
__host__ __device__ __forceinline__ int32_t stsdf_mesh_vertex_index(const unsigned char* halo, const int32_t* around,
                                                                    const uint32_t* records, const int32_t* column_offsets,
                                                                    const int64_t* vertex_offsets, int x, int y, int z,
                                                                    int i) {
  int c[3], slot;
  stsdf_mesh_creator(halo, x, y, z, i, c, &slot);
  const int32_t entry = around[stsdf_mesh_around(c[0], c[1], c[2])];
  if (entry < 0) return 0;  // never: an ACTIVE cube lies in an open block
  const int lx = c[0] & 15, ly = c[1] & 15, lz = c[2] & 15;
  const uint32_t record = records[(int64_t)entry * kStsdfVoxels + tsdf_index(kStsdfU, lx, ly, lz)];
  const uint32_t before = (record >> 16) & ((1u << slot) - 1u);
  return (int32_t)(vertex_offsets[entry] + (int64_t)column_offsets[(int64_t)entry * kStsdfCols + lx * kStsdfU + ly] +
                   (int64_t)(record & 0xffffu) + __builtin_popcount(before));
}

// The triangle pass of column (x, y) of a block: the rows of its cubes by z from `row`, each row
// (v[T[t]], v[T[t + 2]], v[T[t + 1]]).
__host__ __device__ __forceinline__ void stsdf_mesh_column_triangles(const unsigned char* halo, const int32_t* around,
                                                                     const uint32_t* records,
                                                                     const int32_t* column_offsets,
                                                                     const int64_t* vertex_offsets, int64_t row, int x,
                                                                     int y, int32_t* triangles) {
  for (int z = 0; z < kStsdfU; ++z) {
    const int cube_index = halo[stsdf_mesh_halo_at(x, y, z)];
    if (cube_index == 0) continue;
    const int8_t* T = kTsdfTriTable + cube_index * 16;
    for (int t = 0; t < 15 && T[t] >= 0; t += 3) {
      triangles[3 * row] = stsdf_mesh_vertex_index(halo, around, records, column_offsets, vertex_offsets, x, y, z, T[t]);
      triangles[3 * row + 1] = stsdf_mesh_vertex_index(halo, around, records, column_offsets, vertex_offsets, x, y, z, T[t + 2]);
      triangles[3 * row + 2] = stsdf_mesh_vertex_index(halo, around, records, column_offsets, vertex_offsets, x, y, z, T[t + 1]);
      ++row;
    }
  }
}

// The scratch of a mesh call, all on the handle: per voxel of the open blocks one byte and one 32-bit record (5 bytes),
// per column two int32 offsets, per block two int32 totals and two int64 offsets (one more of each for the grand totals).
struct StsdfMeshScratch {
  unsigned char* cubes;      // n x 4096
  uint32_t* records;         // n x 4096
  int32_t* column_vertices;  // n x 256: the vertices the block's earlier columns create
  int32_t* column_triangles;
  int32_t* block_vertices;   // n: the vertices the block creates
  int32_t* block_triangles;
  int64_t* vertex_offsets;   // n + 1: the exclusive sums of the block totals, the grand total last
  int64_t* triangle_offsets;
};

// ---- launchers (kernels_stsdf_mesh.hip; tests/stsdf_mesh_host_driver.cpp has serial stand-ins) ----
// The bytes of the cubes of every open block.  d.n >= 1.
void launch_stsdf_mesh_cubes(hipStream_t s, const StsdfDir& d, unsigned char* d_cubes);
// The records of the ACTIVE cubes, the columns' exclusive offsets inside their blocks and the blocks' totals.  d.n >= 1.
void launch_stsdf_mesh_count(hipStream_t s, const StsdfDir& d, const StsdfMeshScratch& m);
// The vertex rows and the triangle rows, unless stsdf_mesh_fits says no (then nothing is written).  d_colors and
// d_normals may be NULL.  d.n >= 1.
void launch_stsdf_mesh_vertices(hipStream_t s, const TsdfGrid& g, const StsdfDir& d, const StsdfMeshScratch& m,
                                int64_t vertex_capacity, int64_t triangle_capacity, double* d_vertices, double* d_colors,
                                double* d_normals);
void launch_stsdf_mesh_triangles(hipStream_t s, const StsdfDir& d, const StsdfMeshScratch& m, int64_t vertex_capacity,
                                 int64_t triangle_capacity, int32_t* d_triangles);

}  // namespace thip
