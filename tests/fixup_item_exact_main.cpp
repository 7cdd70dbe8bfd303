// Host driver of csrc/fixup_item.h for tests/test_fixup_item_exact_host.py: the fix-up's write-back on the no-store
// route packs the 16 EXACT bits of an item's pairs over the item (row0 and col as the item has them); the replay reads
// bit q back for pair q.  One line per case: row0 col provisional exact row0_back col_back group upper15 bits_ok
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "fixup_item.h"

int main(int argc, char** argv) {
  const int count = argc > 1 ? atoi(argv[1]) : 100;
  uint64_t x = 0x9e3779b97f4a7c15ull;
  auto next = [&]() {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
  };
  for (int k = 0; k < count; ++k) {
    // corner cases first: no bit, every bit, the 16 single bits, their complements; then random fields
    unsigned int exact = k == 0 ? 0u : k == 1 ? 0xffffu : k < 18 ? 1u << (k - 2) : k < 34 ? 0xffffu ^ (1u << (k - 18)) : (unsigned int)(next() & 0xffffu);
    const unsigned int prov = (unsigned int)(next() & 0xffffu);
    const unsigned int row0 = k < 34 ? (k & 1 ? 65532u : 0u) : (unsigned int)(next() % 65533u);
    const unsigned int col = k < 34 ? (k & 2 ? 65535u : 0u) : (unsigned int)(next() & 0xffffu);
    const unsigned long long item = fxi::pack(row0, col, prov);  // as K1's harvest leaves it
    const unsigned long long back = fxi::pack((unsigned int)fxi::row0(item), (unsigned int)fxi::col(item), exact);  // the write-back
    int ok = 1;
    for (int q = 0; q < 16; ++q) ok &= fxi::bit(back, q) == (((exact >> q) & 1u) != 0u) ? 1 : 0;
    printf("%u %u %u %u %d %d %d %llu %d\n", row0, col, prov, exact, fxi::row0(back), fxi::col(back), fxi::is_group(back) ? 1 : 0,
           (back >> 48) & 0x7fffull, ok);
  }
  return 0;
}
