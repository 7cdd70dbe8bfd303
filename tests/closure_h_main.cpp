// csrc/closure_h.h on the HOST: reads cases from the file named on the command line and prints the H of every row.
// Case: int32 m, uint16 deg[m] (clamped degree by rank), uint64 words[m][ceil(m / 64)] (the full compact rows); the
// file ends with m = 0.  Output: one line per case, the m H values.  (tests/test_closure_h_host.py)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "closure_h.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  for (;;) {
    int32_t m = 0;
    if (std::fread(&m, 4, 1, f) != 1 || m <= 0) break;
    const int ng = (m + 63) / 64;
    std::vector<uint16_t> deg((size_t)m);  // (exactly m: a read past the block's columns is an error the sanitizer sees)
    std::vector<uint64_t> words((size_t)m * ng);
    if (std::fread(deg.data(), 2, (size_t)m, f) != (size_t)m) return 3;
    if (std::fread(words.data(), 8, words.size(), f) != words.size()) return 3;
    for (int v = 0; v < m; ++v) std::printf("%d%c", clh::row(words.data() + (size_t)v * ng, m, deg.data()), v + 1 < m ? ' ' : '\n');
  }
  std::fclose(f);
  return 0;
}
