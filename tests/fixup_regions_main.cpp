// Host program over csrc/fixup_regions.h (tests/test_fixup_regions_host.py): for T = argv[1] .. argv[2] and
// CHUNKS in {1, 2, 4} prints one line per (T, CHUNKS):
//   T chunks cells owned_once double_owned unowned outside max_index arena_regions fixup_ok
// owned_once / double_owned / unowned count the upper-triangle cells by how many (block, wave, chunk) of K1's launch
// grid own them -- through K1's own block decode, XCD remap included; outside counts grid slots that claim a cell
// outside the triangle; fixup_ok = the fix-up's enumeration of every tile visits exactly that tile's cells, as one
// run of consecutive indices.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fixup_regions.h"

int main(int argc, char** argv) {
  const int t0 = argc > 1 ? atoi(argv[1]) : 1, t1 = argc > 2 ? atoi(argv[2]) : 45;
  for (int T = t0; T <= t1; ++T)
    for (int chunks : {1, 2, 4}) {
      const int nch = fxr::n_chunks(T), gyr = fxr::row_groups(T), nb = fxr::blocks(T, chunks);
      const long long cells = fxr::cells(T);
      std::vector<int> owners((size_t)cells, 0);
      long long outside = 0, max_index = -1;
      for (int bx = 0; bx < nb; ++bx) {
        int Ig, X;
        fxr::decode_block(bx, nb, gyr, chunks, &Ig, &X);
        if (Ig < 0 || Ig >= gyr || X < 0 || X * chunks >= nch + chunks) {  // not a block of the grid at all
          ++outside;
          continue;
        }
        for (int w = 0; w < fxr::kRowTiles; ++w)
          for (int c = 0; c < chunks; ++c) {
            const int I = fxr::kRowTiles * Ig + w, Xc = X * chunks + c;
            if (!fxr::is_cell(I, Xc, T)) continue;  // (K1 writes nothing for such a slot)
            const long long idx = fxr::cell(I, Xc, T);
            if (idx < 0 || idx >= cells) {
              ++outside;
              continue;
            }
            ++owners[(size_t)idx];
            if (idx > max_index) max_index = idx;
          }
      }
      // every upper-triangle cell by its definition (chunk Xc holds column tiles 8 Xc .. 8 Xc + 7; one of them >= I)
      long long once = 0, twice = 0, unowned = 0, tri = 0;
      int fixup_ok = 1;
      for (int I = 0; I < T; ++I) {
        long long prev = -1;
        int visited = 0;
        for (int Xc = 0; Xc < nch; ++Xc) {
          const bool upper = fxr::kChunkTiles * Xc + fxr::kChunkTiles - 1 >= I;
          if (upper != fxr::is_cell(I, Xc, T)) fixup_ok = 0;
          if (!upper) continue;
          ++tri;
          const long long idx = fxr::cell(I, Xc, T);
          const int o = idx >= 0 && idx < cells ? owners[(size_t)idx] : -1;
          once += o == 1;
          twice += o > 1;
          unowned += o == 0;
        }
        // the fix-up's walk of tile I
        for (int Xc = fxr::first_chunk(I); Xc < nch; ++Xc) {
          const long long idx = fxr::region_offset(0, T, I, Xc) / fxr::kRegionWords;
          if (fxr::kChunkTiles * Xc + fxr::kChunkTiles - 1 < I) fixup_ok = 0;
          if (prev >= 0 && idx != prev + 1) fixup_ok = 0;
          if (Xc == fxr::first_chunk(I) && idx != fxr::row_base(I, nch)) fixup_ok = 0;
          prev = idx;
          ++visited;
        }
        if (visited != nch - (I / fxr::kChunkTiles)) fixup_ok = 0;
        if (prev + 1 != fxr::row_base(I + 1, nch)) fixup_ok = 0;  // rows tile the arena without gaps
      }
      if (tri != cells) fixup_ok = 0;
      // a second problem starts behind the first one's arena
      if (fxr::region_offset(1, T, 0, 0) != fxr::arena_words(T)) fixup_ok = 0;
      printf("%d %d %lld %lld %lld %lld %lld %lld %lld %d\n", T, chunks, cells, once, twice, unowned, outside, max_index,
             (long long)(fxr::arena_words(T) / fxr::kRegionWords), fixup_ok);
    }
  return 0;
}
