// Geometry of the K1 fix-up's region arena (kernels_graph.hip: "group items of the chunk's flagged lane-tiles" in
// tim_graph_mfma3_kernel, tim_fixup_group_kernel).  Plain C++ with no device intrinsic, every function
// __host__ __device__ under hipcc: K1, the fix-up, the host's arena sizing and a host program
// (tests/test_fixup_regions_host.py) evaluate the SAME code.
//
// A REGION is one count word + 63 group items.  K1 writes one region per CELL (row tile I, column chunk Xc): the
// items a wave flagged in the 64 rows of tile I against the 8 column tiles 8 Xc .. 8 Xc + 7.  Only the cells that
// reach the upper triangle exist (8 Xc + 7 >= I, i.e. Xc >= first_chunk(I)); they are stored row tile after row
// tile -- a triangular prefix, not a T x n_chunks rectangle, which would double the arena (55 -> 103 MB per lane at
// 64 x 10 k) for cells nobody owns -- so the regions of one row tile are CONSECUTIVE: the fix-up's wave of tile I
// walks cell(I, first_chunk(I)) .. cell(I, n_chunks - 1) as one run of 512-byte loads.  The index depends on the
// batch's largest problem only (T = its tile count), never on the launch geometry of K1 (column chunks per block,
// XCD remap, triangular block enumeration): every geometry fills the same arena.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FXR_HD __host__ __device__ __forceinline__
#else
#define FXR_HD inline
#endif

namespace fxr {

constexpr int kRegionWords = 64;  // 8-byte words of a region: one 64-lane load
constexpr int kRegionItems = kRegionWords - 1;
constexpr int kChunkTiles = 8;    // column tiles of a chunk (= kMfmaColTiles)
constexpr int kRowTiles = 4;      // row tiles of a K1 block, one per wave (= kMfmaRowTiles)

FXR_HD int n_chunks(int T) { return (T + kChunkTiles - 1) / kChunkTiles; }
// the first chunk that reaches row tile I's diagonal
FXR_HD int first_chunk(int I) { return I / kChunkTiles; }
// cells of the row tiles 0 .. I - 1 of a problem grid with nch chunks (8 row tiles share a first chunk)
FXR_HD int64_t row_base(int I, int nch) {
  const int64_t a = I / kChunkTiles, b = I % kChunkTiles;
  return kChunkTiles * (a * nch - a * (a - 1) / 2) + b * (nch - a);
}
FXR_HD bool is_cell(int I, int Xc, int T) { return I >= 0 && I < T && Xc >= first_chunk(I) && Xc < n_chunks(T); }
// index of cell (I, Xc) among the cells of one problem; T = tiles of the batch's LARGEST problem (the stride)
FXR_HD int64_t cell(int I, int Xc, int T) { return row_base(I, n_chunks(T)) + (Xc - first_chunk(I)); }
FXR_HD int64_t cells(int T) { return row_base(T, n_chunks(T)); }
// the arena: 8-byte words per problem, and the word offset of a region
FXR_HD int64_t arena_words(int T) { return cells(T) * kRegionWords; }
FXR_HD int64_t region_offset(int prob, int T, int I, int Xc) { return ((int64_t)prob * cells(T) + cell(I, Xc, T)) * kRegionWords; }

// K1's launch grid for T tiles and `chunks` column chunks per block: a block = kRowTiles row tiles x chunks column
// chunks; column group X has min(gyr, 2 chunks (X + 1)) row groups (those that touch the upper triangle)
FXR_HD int row_groups(int T) { return (T + kRowTiles - 1) / kRowTiles; }
FXR_HD int blocks(int T, int chunks) {
  const int ct = kChunkTiles * chunks, gxc = (T + ct - 1) / ct, gyr = row_groups(T);
  int nblk = 0;
  for (int X = 0; X < gxc; ++X) nblk += gyr < 2 * chunks * (X + 1) ? gyr : 2 * chunks * (X + 1);
  return nblk;
}
// K1's block decode: blockIdx.x of a grid of nb blocks -> (row group Ig, column group X).  Workgroups go to the 8
// XCDs round robin in dispatch order, so the blocks of one XCD take CONSECUTIVE logical indices (kernels_graph.hip);
// the logical index then enumerates the column groups' row groups.  Wave w of the block owns the cells
// (kRowTiles Ig + w, X chunks + c), c = 0 .. chunks - 1, that exist.
FXR_HD void decode_block(int bx, int nb, int gyr, int chunks, int* Ig_out, int* X_out) {
  const int c = bx & 7, q = nb >> 3, rem = nb & 7;
  int Ig = c * q + (c < rem ? c : rem) + (bx >> 3), X = 0;
  for (;;) {
    const int rows = gyr < 2 * chunks * (X + 1) ? gyr : 2 * chunks * (X + 1);
    if (Ig < rows) break;
    Ig -= rows;
    ++X;
  }
  *Ig_out = Ig;
  *X_out = X;
}

}  // namespace fxr
