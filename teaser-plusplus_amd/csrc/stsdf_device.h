// stsdf_device.h -- the rules of the scalable TSDF volume that do not depend on the launch shape (include/teaser_hip.h,
// "Scalable TSDF volume"; kernels: kernels_stsdf.hip, host side: stsdf.hip, design: DESIGN.md section 37): the key of a
// block, the blocks a depth sample touches, a block as the dense volume it is, the directory look-up, and the surface
// rows, points, colours and normals that cross block faces.  A block's voxels are integrated by the functions of
// tsdf_device.h unchanged.  Nothing here uses a wave operation or LDS, so tests/stsdf_host_driver.cpp runs this very
// source in serial loops.
//
// The library is compiled with -ffp-contract=off: no product-add is fused, and every sum is written out left to right.
#pragma once

#include "tsdf_device.h"

namespace thip {

constexpr int kStsdfU = 16;                          // voxels along a block's side
constexpr int kStsdfCols = kStsdfU * kStsdfU;        // columns of a block: the threads of its workgroup
constexpr int kStsdfVoxels = kStsdfCols * kStsdfU;   // voxels of a block
constexpr int kStsdfBias = 1 << 20;                  // a block index lies in [-2^20, 2^20)
constexpr uint64_t kStsdfNoKey = ~0ull;              // a depth sample that touches nothing
constexpr int kStsdfMaxFrames = 65535;               // frames of one call: blockIdx.y of the touch pass
static_assert(kStsdfCols == kTsdfBlock, "a block's columns are one workgroup of the dense kernels' size");

// One block of one pass: `mask` has bit k set when frame k of the pass touches the block.
struct StsdfItem {
  uint64_t key;
  char* base;
  uint32_t mask;
  uint32_t pad;
};

// The directory as the kernels see it: the open blocks in ascending key order and where each lies.
struct StsdfDir {
  const uint64_t* keys;
  char* const* base;
  int32_t n;
};

// Ascending keys are ascending (bx, by, bz).
__host__ __device__ __forceinline__ uint64_t stsdf_key(int bx, int by, int bz) {
  return ((uint64_t)(bx + kStsdfBias) << 42) | ((uint64_t)(by + kStsdfBias) << 21) | (uint64_t)(bz + kStsdfBias);
}
__host__ __device__ __forceinline__ void stsdf_unkey(uint64_t key, int* b) {
  b[0] = (int)((key >> 42) & 0x1fffff) - kStsdfBias;
  b[1] = (int)((key >> 21) & 0x1fffff) - kStsdfBias;
  b[2] = (int)(key & 0x1fffff) - kStsdfBias;
}

// The blocks the finite or non-finite point p touches: false when none.  Otherwise *key is the block (lo_x, lo_y, lo_z)
// after clipping to the index range and *ext holds hi_a - lo_a (0 .. 3) in bits 2a, 2a + 1.  *clipped: at least one
// block of the point lies outside the index range.
__host__ __device__ __forceinline__ bool stsdf_touch(const double* p, double trunc, double ul, uint64_t* key,
                                                     uint32_t* ext, bool* clipped) {
  *clipped = false;
  for (int a = 0; a < 3; ++a)
    if (!rgbd_finite(p[a])) return false;
  const double L = -(double)kStsdfBias, H = (double)(kStsdfBias - 1);
  int lo_i[3];
  uint32_t e = 0;
  bool empty = false;
  for (int a = 0; a < 3; ++a) {
    const double lo = __builtin_floor((p[a] - trunc) / ul), hi = __builtin_floor((p[a] + trunc) / ul);
    if (lo < L || hi > H) *clipped = true;
    const double lo_c = lo < L ? L : lo, hi_c = hi > H ? H : hi;
    if (lo_c > hi_c) {
      empty = true;
      continue;
    }
    int n = (int)(hi_c - lo_c);
    n = n > 3 ? 3 : n;  // sdf_trunc <= ul: hi - lo <= 3 inside the index range
    lo_i[a] = (int)lo_c;
    e |= (uint32_t)n << (2 * a);
  }
  if (empty) return false;
  *key = stsdf_key(lo_i[0], lo_i[1], lo_i[2]);
  *ext = e;
  return true;
}

// Sampled pixel t of frame f (row-major over the visited pixels): what stsdf_touch says of its point; false also for
// an invalid depth sample.  The rows of the depth image lie packed at f.depth_off, all of them (the TSDF frame's layout).
__host__ __device__ __forceinline__ bool stsdf_touch_pixel(const IcpFrameDesc& f, const unsigned char* in, int t,
                                                           double trunc, double ul, uint64_t* key, uint32_t* ext,
                                                           bool* clipped) {
  *clipped = false;
  const int i = (t / f.nj) * f.stride, j = (t - (t / f.nj) * f.nj) * f.stride;
  const unsigned char* row = in + f.depth_off + (int64_t)i * f.width * rgbd_depth_bytes(f.depth_format);
  const float zf = rgbd_depth(f, row, j);
  if (!rgbd_valid(zf)) return false;
  double p[3];
  rgbd_point(f, i, j, zf, p);
  return stsdf_touch(p, trunc, ul, key, ext, clipped);
}

// Block b as the dense volume it is: g0 is the block at the origin.
__host__ __device__ __forceinline__ TsdfGrid stsdf_block_grid(const TsdfGrid& g0, double ul, const int* b) {
  TsdfGrid g = g0;
  for (int k = 0; k < 3; ++k) {
    g.origin[k] = (double)b[k] * ul;
    g.org_f[k] = (float)g.origin[k];
  }
  return g;
}

// A block's memory is a dense volume's: tsdf, weight, then three planes of colour, each in the [z][x][y] layout.
__host__ __device__ __forceinline__ TsdfFields stsdf_fields(char* base, int color_type) {
  TsdfFields v;
  v.tsdf = reinterpret_cast<float*>(base);
  v.weight = v.tsdf + kStsdfVoxels;
  v.color = color_type != 0 ? reinterpret_cast<double*>(base + 8 * (size_t)kStsdfVoxels) : nullptr;
  v.n = kStsdfVoxels;
  return v;
}

// Where block (bx, by, bz) lies; NULL when it is not open (or outside the index range).
__host__ __device__ __forceinline__ char* stsdf_find(const StsdfDir& d, int64_t bx, int64_t by, int64_t bz) {
  const int64_t L = -(int64_t)kStsdfBias, H = kStsdfBias;
  if (bx < L || bx >= H || by < L || by >= H || bz < L || bz >= H) return nullptr;
  const uint64_t key = stsdf_key((int)bx, (int)by, (int)bz);
  int lo = 0, hi = d.n;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (d.keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < d.n && d.keys[lo] == key ? d.base[lo] : nullptr;
}

// Whether the usable voxel (x, y, z) (value f0) of a block with fields v gives a row along axis i.  up[i] is the block
// b + e_i (NULL: absent).  Then *v1 are the fields the neighbour lies in, *at1 its index and *f1 its value.
__host__ __device__ __forceinline__ bool stsdf_surface_row(const TsdfGrid& g, const TsdfFields& v, char* const* up, int x,
                                                           int y, int z, int i, float f0, TsdfFields* v1, int64_t* at1,
                                                           float* f1) {
  int n[3] = {x + (i == 0), y + (i == 1), z + (i == 2)};
  *v1 = v;
  if (n[i] == kStsdfU) {
    if (!up[i]) return false;
    *v1 = stsdf_fields(up[i], g.color_type);
    n[i] = 0;
  }
  *at1 = tsdf_index(kStsdfU, n[0], n[1], n[2]);
  *f1 = v1->tsdf[*at1];
  return tsdf_usable(v1->weight[*at1], *f1) && f0 * *f1 < 0.0f;
}

// The rows voxel (x, y, z) gives: 0 .. 3 (mode 0, the surface) or 0 .. 1 (mode 1, the voxel cloud).
__host__ __device__ __forceinline__ int stsdf_voxel_rows(const TsdfGrid& g, const TsdfFields& v, char* const* up, int mode,
                                                         int x, int y, int z) {
  const int64_t at0 = tsdf_index(kStsdfU, x, y, z);
  const float f0 = v.tsdf[at0];
  if (!tsdf_usable(v.weight[at0], f0)) return 0;
  if (mode == 1) return 1;
  int rows = 0;
  for (int i = 0; i < 3; ++i) {
    TsdfFields v1;
    int64_t at1;
    float f1;
    if (stsdf_surface_row(g, v, up, x, y, z, i, f0, &v1, &at1, &f1)) ++rows;
  }
  return rows;
}

// T(q) on the global lattice (q in world coordinates): the dense form, a corner in an absent block has the value 0.
// b and own are the block the caller works in and its tsdf plane: most corners lie there and need no look-up.
__host__ __device__ __forceinline__ double stsdf_trilinear(const TsdfGrid& g, const StsdfDir& d, const int* b,
                                                           const float* own, const double* q) {
  int64_t idx[3];
  double r[3];
  for (int k = 0; k < 3; ++k) {
    const double a = q[k] / g.vl - 0.5, fl = __builtin_floor(a);
    r[k] = a - fl;
    idx[k] = (int64_t)fl;  // |q| < 2^21 ul: no overflow
  }
  double sum = 0.0;
  for (int corner = 0; corner < 8; ++corner) {
    const int ox = corner >> 2, oy = (corner >> 1) & 1, oz = corner & 1;
    const int64_t cx = idx[0] + ox, cy = idx[1] + oy, cz = idx[2] + oz;
    const int64_t bx = cx >> 4, by = cy >> 4, bz = cz >> 4;  // floor division by kStsdfU
    const float* plane = own;
    if (bx != b[0] || by != b[1] || bz != b[2]) plane = reinterpret_cast<const float*>(stsdf_find(d, bx, by, bz));
    const float f = plane ? plane[tsdf_index(kStsdfU, (int)(cx & 15), (int)(cy & 15), (int)(cz & 15))] : 0.0f;
    const double term = (((ox ? r[0] : 1.0 - r[0]) * (oy ? r[1] : 1.0 - r[1])) * (oz ? r[2] : 1.0 - r[2])) * (double)f;
    sum = corner == 0 ? term : sum + term;
  }
  return sum;
}

// The normal at p (world coordinates): the dense rule over stsdf_trilinear.
__host__ __device__ __forceinline__ void stsdf_normal_at(const TsdfGrid& g, const StsdfDir& d, const int* b,
                                                         const float* own, const double* p, double* normal) {
  const double gstep = 0.99 * g.vl;
  double n[3];
  for (int k = 0; k < 3; ++k) {
    double hi[3] = {p[0], p[1], p[2]}, lo[3] = {p[0], p[1], p[2]};
    hi[k] = p[k] + gstep;
    lo[k] = p[k] - gstep;
    n[k] = stsdf_trilinear(g, d, b, own, hi) - stsdf_trilinear(g, d, b, own, lo);
  }
  const double s = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  if (s > 0.0) {
    const double len = __builtin_sqrt(s);
    for (int k = 0; k < 3; ++k) n[k] = n[k] / len;
  }
  for (int k = 0; k < 3; ++k) normal[k] = n[k];
}

// The surface point between voxel (x, y, z) (value f0) of block b (grid g, fields v) and its neighbour along i (fields
// v1, index at1, value f1): the point and, where the pointers are given, the normal and the colour.
__host__ __device__ __forceinline__ void stsdf_surface_point(const TsdfGrid& g, const StsdfDir& d, const int* b,
                                                             const TsdfFields& v, const TsdfFields& v1, int x, int y, int z,
                                                             int i, float f0, int64_t at1, float f1, double* point,
                                                             double* normal, double* color) {
  const float r0 = __builtin_fabsf(f0), r1 = __builtin_fabsf(f1);
  const double den = (double)(r0 + r1);
  double p[3] = {(g.half + g.vl * (double)x) + g.origin[0], (g.half + g.vl * (double)y) + g.origin[1],
                 (g.half + g.vl * (double)z) + g.origin[2]};
  const double p1 = p[i] + g.vl;
  p[i] = (p[i] * (double)r1 + p1 * (double)r0) / den;
  for (int k = 0; k < 3; ++k) point[k] = p[k];
  if (color) {
    const int64_t at0 = tsdf_index(kStsdfU, x, y, z);
    for (int k = 0; k < 3; ++k) {
      double c = (v.color[k * v.n + at0] * (double)r1 + v1.color[k * v1.n + at1] * (double)r0) / den;
      if (g.color_type == 1) c = c / 255.0;
      color[k] = g.color_type == 2 ? rgbd_canonical(c) : c;
    }
  }
  if (normal) stsdf_normal_at(g, d, b, v.tsdf, p, normal);
}

// The rows of column (x, y) of directory entry e, written from `row` on; returns the row after the last.
__host__ __device__ __forceinline__ int64_t stsdf_write_column(const TsdfGrid& g0, double ul, const StsdfDir& d, int e,
                                                               char* const* up, int mode, int x, int y, int64_t row,
                                                               double* points, double* normals, double* colors) {
  int b[3];
  stsdf_unkey(d.keys[e], b);
  const TsdfGrid g = stsdf_block_grid(g0, ul, b);
  const TsdfFields v = stsdf_fields(d.base[e], g.color_type);
  for (int z = 0; z < kStsdfU; ++z) {
    const int64_t at0 = tsdf_index(kStsdfU, x, y, z);
    const float f0 = v.tsdf[at0];
    if (!tsdf_usable(v.weight[at0], f0)) continue;
    if (mode == 1) {
      tsdf_voxel_point(g, x, y, z, f0, points + 3 * row, colors ? colors + 3 * row : nullptr);
      ++row;
      continue;
    }
    for (int i = 0; i < 3; ++i) {
      TsdfFields v1;
      int64_t at1;
      float f1;
      if (!stsdf_surface_row(g, v, up, x, y, z, i, f0, &v1, &at1, &f1)) continue;
      stsdf_surface_point(g, d, b, v, v1, x, y, z, i, f0, at1, f1, points + 3 * row, normals ? normals + 3 * row : nullptr,
                          colors ? colors + 3 * row : nullptr);
      ++row;
    }
  }
  return row;
}

// The blocks b + e_i of directory entry e.
__host__ __device__ __forceinline__ void stsdf_up_blocks(const StsdfDir& d, int e, char** up) {
  int b[3];
  stsdf_unkey(d.keys[e], b);
  for (int i = 0; i < 3; ++i) up[i] = stsdf_find(d, (int64_t)b[0] + (i == 0), (int64_t)b[1] + (i == 1), (int64_t)b[2] + (i == 2));
}

// ---- launchers (kernels_stsdf.hip; tests/stsdf_host_driver.cpp has serial stand-ins) ----
// The touch pass: for sampled pixel t of frame k, keys[f.point_off + t] = the clipped lo block of its point (kStsdfNoKey:
// none) and vals[...] = k << 6 | ext; *oor grows by the samples with a block outside the index range (zeroed by the caller).
void launch_stsdf_touch(hipStream_t s, const IcpFrameDesc* d_frames, int n_frames, int max_vis, const unsigned char* d_in,
                        double trunc, double ul, uint64_t* d_keys, uint32_t* d_vals, unsigned long long* d_oor);
// The distinct (key, val) pairs of the n candidates in ascending (key, val) order, kStsdfNoKey dropped; *d_count is
// their number.  d_keys and d_vals end up sorted; tmp_*, head and pos are scratch of n entries each.
size_t stsdf_unique_temp_bytes(int64_t n);
hipError_t launch_stsdf_unique(hipStream_t s, int64_t n, void* d_temp, size_t temp_bytes, uint64_t* d_keys, uint32_t* d_vals,
                               uint64_t* d_tmp_keys, uint32_t* d_tmp_vals, int32_t* d_head, int32_t* d_pos,
                               uint64_t* d_ukeys, uint32_t* d_uvals, int32_t* d_count);
// One pass: the frames of ck whose bit an item's mask has, in order, applied to the item's block.
void launch_stsdf_integrate(hipStream_t s, const TsdfGrid& g0, double ul, const TsdfChunkArgs& ck, const unsigned char* d_in,
                            const StsdfItem* d_items, int n_items);
// counts[e 256 + x 16 + y] = the rows of the column, totals[e] = those of the block, offsets = the exclusive sum of the
// totals with the grand total at offsets[d.n].
void launch_stsdf_count(hipStream_t s, const TsdfGrid& g0, const StsdfDir& d, int mode, int32_t* d_counts,
                        int32_t* d_totals, int64_t* d_offsets);
// The rows, blocks in directory order and columns in (x, y) order inside, unless the total exceeds capacity.
void launch_stsdf_write(hipStream_t s, const TsdfGrid& g0, double ul, const StsdfDir& d, int mode, const int32_t* d_counts,
                        const int64_t* d_offsets, int64_t capacity, double* d_points, double* d_normals, double* d_colors);
// Between n blocks (d_base[k]) and Open3D's voxel order: tw is n x 4096 x 2 floats, color n x 4096 x 3 doubles.
void launch_stsdf_export(hipStream_t s, int color_type, char* const* d_base, int n, float* d_tw, double* d_color);
void launch_stsdf_import(hipStream_t s, int color_type, char* const* d_base, int n, const float* d_tw, const double* d_color);

}  // namespace thip
