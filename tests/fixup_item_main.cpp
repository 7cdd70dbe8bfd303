// Host program of tests/test_fixup_item_host.py: csrc/fixup_item.h compiled by g++.  For `count` random transposed words
// (a fixed-seed 64-bit LCG) and every (rt, h) it packs an item from the word's 16 bits and prints one line per case:
//   rt h row0 col word  row0_back col_back group upper15  bits_ok  gather_ok  zero_item_fields_ok
// bits_ok: bit q of the item = bit 32 rt + 4 h + row_of(q) of the word, for all q; gather_ok: no bit outside the 16 set;
// zero_item_fields_ok: the item packed with bits 0 and with bits 0xffff differ in bits 32 .. 47 only.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "fixup_item.h"

int main(int argc, char** argv) {
  const int count = argc > 1 ? atoi(argv[1]) : 16;
  uint64_t x = 0x9e3779b97f4a7c15ull;
  auto next = [&]() {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    return x ^ (x >> 29);
  };
  for (int k = 0; k < count; ++k) {
    // the first words are the corner cases: nothing, everything, one bit per pair position
    const uint64_t word = k == 0 ? 0ull : k == 1 ? ~0ull : k < 66 ? (1ull << (k - 2)) : next();
    for (int rt = 0; rt < 2; ++rt)
      for (int h = 0; h < 2; ++h) {
        const unsigned int row0 = (unsigned int)(next() & 0xffffu), col = (unsigned int)(next() & 0xffffu);
        const unsigned int bits = fxi::gather_bits(word, rt, h);
        const unsigned long long item = fxi::pack(row0, col, bits);
        int bits_ok = 1;
        for (int q = 0; q < 16; ++q)
          if (fxi::bit(item, q) != (((word >> (32 * rt + 4 * h + fxi::row_of(q))) & 1ull) != 0ull)) bits_ok = 0;
        const int gather_ok = (bits >> 16) == 0u;
        const unsigned long long lo = fxi::pack(row0, col, 0u), hi = fxi::pack(row0, col, 0xffffu);
        const int fields_ok = (lo ^ hi) == (0xffffull << 32) && fxi::row0(lo) == fxi::row0(hi) && fxi::col(lo) == fxi::col(hi);
        printf("%d %d %u %u %llu %d %d %d %llu %d %d %d\n", rt, h, row0, col, (unsigned long long)word, fxi::row0(item),
               fxi::col(item), fxi::is_group(item) ? 1 : 0, (unsigned long long)((item >> 48) & 0x7fffull), bits_ok, gather_ok,
               fields_ok);
      }
  }
  // the 16 row offsets of an item: 0..3, 8..11, 16..19, 24..27
  for (int q = 0; q < 16; ++q) printf("%d%c", fxi::row_of(q), q == 15 ? '\n' : ' ');
  return 0;
}
