// The GROUP item of the K1 fix-up's worklist (kernels_graph.hip: the harvest behind tim_graph_mfma3_kernel's loop
// writes them, tim_fixup_group_kernel resolves them).  Plain C++ with no device intrinsic, every function
// __host__ __device__ under hipcc: K1, the fix-up and a host program (tests/test_fixup_item_host.py) evaluate the
// SAME code.
//
// An item names 16 pairs of ONE column: (row0 + row_of(q), col), q = 0 .. 15, row_of(q) = (q & 3) + 8 (q >> 2) -- the
// rows a lane of a 32 x 32 MFMA tile holds (row0 = 64 I + 32 rt + 4 h).  It also CARRIES the filter's 16 provisional
// bits of those pairs: the fix-up flips what disagrees with the reference predicate, and the only other place the 16
// bits sit together is the transposed word (bitmap row `col`, word I), which the upper-triangle route of K1 does not
// store.
//   bit 63      group flag
//   bits 48-62  zero
//   bits 32-47  provisional bits, bit 32 + q = pair q
//   bits 16-31  row0
//   bits  0-15  col
// (The problem an item belongs to is the grid row of the launch that reads it.)
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FXI_HD __host__ __device__ __forceinline__
#else
#define FXI_HD inline
#endif

namespace fxi {

constexpr unsigned long long kGroupFlag = 1ull << 63;

// row offset of pair q inside the item's 32-row half tile (before the lane half's 4 h)
FXI_HD int row_of(int q) { return (q & 3) + 8 * (q >> 2); }

// The 16 provisional bits of lane half h (0, 1) in row half rt (0, 1), out of the column's transposed word
// (bit r = row 64 I + r): rows 32 rt + 4 h + {0..3, 8..11, 16..19, 24..27}.
FXI_HD unsigned int gather_bits(uint64_t tword, int rt, int h) {
  const unsigned int x = (unsigned int)(tword >> (32 * rt + 4 * h));  // (4 h + 27 <= 31: all 16 bits are in reach)
  return (x & 0xfu) | ((x >> 4) & 0xf0u) | ((x >> 8) & 0xf00u) | ((x >> 12) & 0xf000u);
}

FXI_HD unsigned long long pack(unsigned int row0, unsigned int col, unsigned int bits16) {
  return kGroupFlag | ((unsigned long long)(bits16 & 0xffffu) << 32) | ((unsigned long long)(row0 & 0xffffu) << 16) |
         (unsigned long long)(col & 0xffffu);
}

FXI_HD int row0(unsigned long long item) { return (int)((item >> 16) & 0xffffull); }
FXI_HD int col(unsigned long long item) { return (int)(item & 0xffffull); }
FXI_HD bool is_group(unsigned long long item) { return (item & kGroupFlag) != 0ull; }
FXI_HD bool bit(unsigned long long item, int q) { return ((item >> (32 + q)) & 1ull) != 0ull; }

}  // namespace fxi
