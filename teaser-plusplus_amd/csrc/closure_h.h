// The H value of a row of the degree closure's compact graph, from the row's FULL words (kernels_heuristic.hip: the
// verdict launch of the three-launch route computes it for its rows; tests/closure_h_main.cpp evaluates the SAME code on
// the host).  Plain C++ with compiler builtins only, every function __host__ __device__ under hipcc.
//
// The candidate set R is ranked by (degree descending, vertex ascending); d_i is the degree of rank i clamped to the
// size cap of R (P <= |R| <= cap, so min(P, d) is the same), a sequence that does not increase.  For a row with set
// bits at the ranks i,
//   H = max over the set bits i of min(P_i, d_i),     P_i = the set bits of the row up to and including i,
// and P does not decrease.  The row is walked in blocks of 64 ranks with the running count `base` of the blocks in
// front:
//   below  base + cnt <= d of the block's last rank: every P of the block <= every d of it, min = P, largest at the
//          last set bit: base + cnt;
//   above  base + 1 >= d of the block's first rank: every P >= every d, min = d, largest at the first set bit;
//   else   P crosses d inside the block.  P(k) >= d(k) is monotone in the position k, so the first position k* where
//          it holds is found by bisection: the set bits in front of k* contribute the P of the last of them, those from
//          k* on the d of the first of them.
// Bits at or beyond `cols` (ranks >= |R|) must be zero.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CLH_HD __host__ __device__ __forceinline__
#else
#define CLH_HD inline
#endif

namespace clh {

CLH_HD uint64_t bits_below(int k) { return k >= 64 ? ~0ull : ((1ull << k) - 1ull); }

// One block of a row: `full` the row's word, `base` the set bits of the row in front of the block, dblk[k] the clamped
// degree of the block's rank k (k < cols <= 64), hmax the H of the blocks in front.  Returns the H up to and including
// this block; the caller adds popcount(full) to base.
template <class Deg>
CLH_HD int block(uint64_t full, int base, int cols, const Deg* dblk, int hmax) {
  if (full == 0ull) return hmax;
  const int cnt = __builtin_popcountll(full);
  const int d_hi = (int)dblk[0], d_lo = (int)dblk[cols - 1];
  int cand;
  if (base + cnt <= d_lo) {
    cand = base + cnt;
  } else if (base + 1 >= d_hi) {
    cand = (int)dblk[__builtin_ctzll(full)];
  } else {
    int lo = 0, hi = cols;  // the first position with P >= d lies in [lo, hi]; hi = cols: none
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const int P = base + __builtin_popcountll(full & bits_below(mid + 1));
      if (P >= (int)dblk[mid])
        hi = mid;
      else
        lo = mid + 1;
    }
    const uint64_t front = full & bits_below(lo), back = full & ~bits_below(lo);
    cand = front ? base + __builtin_popcountll(front) : 0;
    if (back) {
      const int db = (int)dblk[__builtin_ctzll(back)];
      cand = cand > db ? cand : db;
    }
  }
  return hmax > cand ? hmax : cand;
}

// A whole row of ng = ceil(m / 64) words.
template <class Deg>
CLH_HD int row(const uint64_t* words, int m, const Deg* deg) {
  int base = 0, hmax = 0;
  for (int B = 0; 64 * B < m; ++B) {
    const int cols = m - 64 * B < 64 ? m - 64 * B : 64;
    hmax = block(words[B], base, cols, deg + 64 * B, hmax);
    base += __builtin_popcountll(words[B]);
  }
  return hmax;
}

}  // namespace clh
