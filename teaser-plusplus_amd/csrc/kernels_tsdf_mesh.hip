// kernels_tsdf_mesh.hip -- the triangle mesh of the TSDF volume for gfx950 (include/teaser_hip.h, "TSDF volume", the
// triangle mesh; device code: tsdf_mesh_device.h; host side: tsdf_mesh.hip; design, bounds and the resource report:
// DESIGN.md section 34).
//
// As in kernels_tsdf.hip a thread is a column (x, y) walking z and the volumes lie as [z][x][y] planes, so the lanes of a
// wave touch consecutive addresses at every step.  cubes: a column carries the sign and weight bits of the layer below
// in a register, reads the four voxels of the layer above and writes one byte per cube.  count: a column reads its own
// bytes and, at an ACTIVE cube only, the bytes of the nine earlier cubes that may have created one of its vertices; it
// writes the cube's record and sums its vertices and triangles.  scan: one block, both exclusive sums.  vertices and
// triangles: a column writes its rows from its offsets; the volume is read only at the edges that carry a vertex, and a
// vertex index comes from the bytes, the records and the offsets -- no hash, no sort, no atomic.  That is the order in
// which Open3D's serial loop first meets the vertices and emits the triangles.
#include "tsdf_mesh_device.h"

namespace thip {

namespace {

__device__ __forceinline__ bool mesh_column(const TsdfGrid& g, int* x, int* y) {
  const int64_t col = (int64_t)blockIdx.x * kTsdfBlock + threadIdx.x;
  if (col >= (int64_t)g.R * g.R) return false;
  *x = (int)(col / g.R);
  *y = (int)(col - (int64_t)*x * g.R);
  return true;
}

inline dim3 mesh_grid(const TsdfGrid& g) {
  return dim3((unsigned)(((int64_t)g.R * g.R + kTsdfBlock - 1) / kTsdfBlock));
}

}  // namespace

__global__ __launch_bounds__(kTsdfBlock) void tsdf_mesh_cubes_kernel(const TsdfGrid g, const TsdfFields v,
                                                                     unsigned char* __restrict__ cubes) {
  int x, y;
  if (!mesh_column(g, &x, &y)) return;
  tsdf_mesh_column_cubes(g, v, x, y, cubes);
}

__global__ __launch_bounds__(kTsdfBlock) void tsdf_mesh_count_kernel(const TsdfGrid g,
                                                                     const unsigned char* __restrict__ cubes,
                                                                     uint32_t* __restrict__ records,
                                                                     int32_t* __restrict__ counts) {
  int x, y;
  if (!mesh_column(g, &x, &y)) return;
  const int64_t plane = (int64_t)g.R * g.R, col = (int64_t)x * g.R + y;
  int32_t nv, nt;
  tsdf_mesh_column_count(cubes, g.R, x, y, records, &nv, &nt);
  counts[col] = nv;
  counts[plane + col] = nt;
}

// One block.  For the vertex sums (a = 0) and the triangle sums (a = 1): offsets[c] = the sum over the columns in front
// of c, offsets[n_cols] = totals[a] = the whole sum.
__global__ __launch_bounds__(kTsdfScanThreads) void tsdf_mesh_scan_kernel(const int32_t* __restrict__ counts,
                                                                          const int64_t n_cols,
                                                                          int64_t* __restrict__ offsets,
                                                                          int64_t* __restrict__ totals) {
  __shared__ int64_t s[kTsdfScanThreads];
  const int64_t chunk = (n_cols + kTsdfScanThreads - 1) / kTsdfScanThreads;
  const int64_t lo0 = (int64_t)threadIdx.x * chunk;
  const int64_t lo = lo0 < n_cols ? lo0 : n_cols, hi = lo + chunk < n_cols ? lo + chunk : n_cols;
  for (int a = 0; a < 2; ++a) {
    const int32_t* cnt = counts + a * n_cols;
    int64_t* off = offsets + a * (n_cols + 1);
    int64_t sum = 0;
    for (int64_t k = lo; k < hi; ++k) sum += cnt[k];
    __syncthreads();  // the sums of the pass before are read
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < kTsdfScanThreads; o <<= 1) {  // inclusive Hillis-Steele scan of the per-thread sums
      const int64_t add = threadIdx.x >= (unsigned)o ? s[threadIdx.x - o] : 0;
      __syncthreads();
      s[threadIdx.x] += add;
      __syncthreads();
    }
    int64_t run = s[threadIdx.x] - sum;
    for (int64_t k = lo; k < hi; ++k) {
      off[k] = run;
      run += cnt[k];
    }
    if (threadIdx.x == kTsdfScanThreads - 1) off[n_cols] = totals[a] = s[threadIdx.x];
  }
}

__global__ __launch_bounds__(kTsdfBlock) void tsdf_mesh_vertices_kernel(
    const TsdfGrid g, const TsdfFields v, const unsigned char* __restrict__ cubes, const uint32_t* __restrict__ records,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ totals, const int64_t vertex_capacity,
    const int64_t triangle_capacity, double* __restrict__ vertices, double* __restrict__ colors,
    double* __restrict__ normals) {
  int x, y;
  if (!mesh_column(g, &x, &y) || !tsdf_mesh_fits(totals, vertex_capacity, triangle_capacity)) return;
  tsdf_mesh_column_vertices(g, v, cubes, records, offsets, x, y, vertices, colors, normals);
}

__global__ __launch_bounds__(kTsdfBlock) void tsdf_mesh_triangles_kernel(
    const TsdfGrid g, const unsigned char* __restrict__ cubes, const uint32_t* __restrict__ records,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ totals, const int64_t vertex_capacity,
    const int64_t triangle_capacity, int32_t* __restrict__ triangles) {
  int x, y;
  if (!mesh_column(g, &x, &y) || !tsdf_mesh_fits(totals, vertex_capacity, triangle_capacity)) return;
  const int64_t plane = (int64_t)g.R * g.R;
  tsdf_mesh_column_triangles(cubes, records, offsets, offsets + plane + 1, g.R, x, y, triangles);
}

void launch_tsdf_mesh_cubes(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, unsigned char* d_cubes) {
  hipLaunchKernelGGL(tsdf_mesh_cubes_kernel, mesh_grid(g), dim3(kTsdfBlock), 0, s, g, v, d_cubes);
}

void launch_tsdf_mesh_count(hipStream_t s, const TsdfGrid& g, const unsigned char* d_cubes, uint32_t* d_records,
                            int32_t* d_counts, int64_t* d_offsets, int64_t* d_totals) {
  hipLaunchKernelGGL(tsdf_mesh_count_kernel, mesh_grid(g), dim3(kTsdfBlock), 0, s, g, d_cubes, d_records, d_counts);
  hipLaunchKernelGGL(tsdf_mesh_scan_kernel, dim3(1), dim3(kTsdfScanThreads), 0, s, d_counts, (int64_t)g.R * g.R, d_offsets,
                     d_totals);
}

void launch_tsdf_mesh_vertices(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, const unsigned char* d_cubes,
                               const uint32_t* d_records, const int64_t* d_offsets, const int64_t* d_totals,
                               int64_t vertex_capacity, int64_t triangle_capacity, double* d_vertices, double* d_colors,
                               double* d_normals) {
  hipLaunchKernelGGL(tsdf_mesh_vertices_kernel, mesh_grid(g), dim3(kTsdfBlock), 0, s, g, v, d_cubes, d_records, d_offsets,
                     d_totals, vertex_capacity, triangle_capacity, d_vertices, d_colors, d_normals);
}

void launch_tsdf_mesh_triangles(hipStream_t s, const TsdfGrid& g, const unsigned char* d_cubes, const uint32_t* d_records,
                                const int64_t* d_offsets, const int64_t* d_totals, int64_t vertex_capacity,
                                int64_t triangle_capacity, int32_t* d_triangles) {
  hipLaunchKernelGGL(tsdf_mesh_triangles_kernel, mesh_grid(g), dim3(kTsdfBlock), 0, s, g, d_cubes, d_records, d_offsets,
                     d_totals, vertex_capacity, triangle_capacity, d_triangles);
}

}  // namespace thip
