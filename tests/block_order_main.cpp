// Host program over csrc/fixup_regions.h (tests/test_block_order_host.py): K1's block decode.  For every T of the
// command line and CHUNKS in {1, 2, 4} prints one line per (T, CHUNKS):
//   T chunks blocks once twice missing outside
// once / twice / missing count the (row group, column group) pairs of the triangular grid -- column group X has
// min(gyr, 2 chunks (X + 1)) row groups -- by how often fxr::decode_block produces them over blockIdx.x = 0 .. nb - 1;
// outside counts decodes that are no block of the grid.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fixup_regions.h"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    const int T = atoi(argv[a]);
    for (int chunks : {1, 2, 4}) {
      const int gyr = fxr::row_groups(T), nb = fxr::blocks(T, chunks);
      const int ct = fxr::kChunkTiles * chunks, gxc = (T + ct - 1) / ct;
      std::vector<long long> first((size_t)gxc + 1, 0);  // blocks in front of column group X, by the grid's definition
      for (int X = 0; X < gxc; ++X) first[(size_t)X + 1] = first[(size_t)X] + (gyr < 2 * chunks * (X + 1) ? gyr : 2 * chunks * (X + 1));
      std::vector<int> seen((size_t)first[(size_t)gxc], 0);
      long long outside = 0;
      for (int bx = 0; bx < nb; ++bx) {
        int Ig = -1, X = -1;
        fxr::decode_block(bx, nb, gyr, chunks, &Ig, &X);
        if (X < 0 || X >= gxc || Ig < 0 || Ig >= first[(size_t)X + 1] - first[(size_t)X]) {
          ++outside;
          continue;
        }
        ++seen[(size_t)first[(size_t)X] + Ig];
      }
      long long once = 0, twice = 0, missing = 0;
      for (int s : seen) once += s == 1, twice += s > 1, missing += s == 0;
      printf("%d %d %d %lld %lld %lld %lld\n", T, chunks, nb, once, twice, missing, outside);
    }
  }
  return 0;
}
