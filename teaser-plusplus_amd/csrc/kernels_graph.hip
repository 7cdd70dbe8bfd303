// kernels_graph.hip -- gfx950 kernels for the O(N^2) stage and the greedy/peel clique stages.
//
//   K1  tim_graph_kernel   fused computeTIMs (reference registration.cc:512-551) +
//                          ScaleInliersSelector / TLS-scale consensus test (registration.cc:427-443,
//                          410-425) + mask->graph loop (registration.cc:614-619): the TIMs are
//                          never materialised; output is the symmetric adjacency bitmap.
//   K2  degrees / starts / greedy clique / peel: stand in for pmc's compute_cores + pmc_heu
//                          (reference graph.cc:58-59, 88-102).
//
// Compiled with -ffp-contract=off: the pruning predicate must round every product and add
// individually, as the reference's default (non-FMA) build does.  FMAs below are explicit.
#include <algorithm>
#include <utility>
#include <vector>

#include <cstdio>
#include <cstdlib>

#include "internal.h"
#include "fixup_item.h"
#include "fixup_regions.h"
#include "k1_consts.h"
#include "wave_utils.h"

namespace thip {

// ------------------------------------------------------------------------------------------
// K1 predicate
// ------------------------------------------------------------------------------------------
// Reference semantics (registration.cc:434-442): with a = src_j - src_i, b = dst_j - dst_i,
//   edge <=> | sqrt((ax^2+ay^2)+az^2) - sqrt((bx^2+by^2)+bz^2) | <= beta      (all IEEE double).
// Exact arithmetic: with A = |a|^2, B = |b|^2, t = A + B, D = A - B,
//   edge <=> t <= beta^2  or  d := D^2 - 2 beta^2 t + beta^4 <= 0         (d = (t-beta^2)^2 - 4AB).
// FAST PATH (per pair: 6 sub, 6 fma/mul for A and B, 2 add, 2 fma for d, 2 for the band, 3 cmp):
// A, B, d are evaluated with FMAs -- NOT the reference's rounding -- and the sign of d is trusted
// only when |d| clears a guard band of 2e-12 (t^2 + beta^4) >= 1e-12 (t + beta^2)^2: three
// orders of magnitude above both the rounding error of the fast d (a few 1e-16 (t+beta^2)^2) and
// the gap between the reference's rounded predicate and the exact one (<= ~4e-15 (t+beta^2)^2).
// EXACT PATH (inside the band -- a vanishing fraction of pairs -- and for any NaN): the reference
// expression itself, products and sums individually rounded (this file is compiled with
// -ffp-contract=off) and correctly rounded sqrt, so the bitmap is bit-identical by construction.
struct EdgeConst {
  double beta;        // 2 noise_bound sqrt(cbar2)
  double beta2;       // beta^2
  double m2beta2;     // -2 beta^2
  double beta4;       // beta^4
  double s_hat;       // scale estimate (MODE 1)
};

__device__ __forceinline__ bool tim_edge_exact(double ax, double ay, double az, double bx,
                                               double by, double bz, double beta) {
  const double A = (ax * ax + ay * ay) + az * az;
  const double B = (bx * bx + by * by) + bz * bz;
  return __builtin_fabs(__builtin_sqrt(A) - __builtin_sqrt(B)) <= beta;
}

// fast path; *uncertain is set when the sign of d cannot be trusted (guard band or NaN)
__device__ __forceinline__ bool tim_edge_fast(double ax, double ay, double az, double bx,
                                              double by, double bz, const EdgeConst& k,
                                              bool* uncertain, bool* short_pair) {
  const double A = __builtin_fma(az, az, __builtin_fma(ay, ay, ax * ax));
  const double B = __builtin_fma(bz, bz, __builtin_fma(by, by, bx * bx));
  const double t = A + B;
  const double D = A - B;
  const double d = __builtin_fma(D, D, __builtin_fma(t, k.m2beta2, k.beta4));
  const double band = __builtin_fma(t, t, k.beta4) * 2e-12;
  *uncertain = !(__builtin_fabs(d) > band);
  *short_pair = t <= k.beta2;
  return d <= 0.0;
}

// TLS-scale consensus (registration.cc:415-424 + :86): raw = |b|/|a|, alpha = beta * (1/|a|),
// edge <=> |raw - s_hat| <= alpha.  Evaluated literally (IEEE sqrt / div).
__device__ __forceinline__ bool tim_edge_scaled(double ax, double ay, double az, double bx,
                                                double by, double bz, const EdgeConst& k) {
  const double v1 = __builtin_sqrt((ax * ax + ay * ay) + az * az);
  const double v2 = __builtin_sqrt((bx * bx + by * by) + bz * bz);
  const double raw = v2 / v1;
  const double alpha = k.beta * (1.0 / v1);
  return __builtin_fabs(raw - k.s_hat) <= alpha;
}

// Tiling: a wave owns 64 rows (lane = row) and walks 64-column tiles of the upper triangle.
// The tile's 64 column points are staged once in a per-wave LDS buffer and read back as
// broadcast ds_read_b128 (same address in every lane), software-pipelined three columns ahead;
// per column the 64 row lanes evaluate the predicate, the lane keeps its own bit (row word) and
// the wave ballot IS the transposed word (row j, word I, kept in lane j by v_writelane) -- so each
// unordered pair is evaluated once and both halves of the symmetric bitmap are written.
// A block = 4 waves x kColTilesPerWave consecutive column tiles of ONE row tile, so a row's words
// from one block are contiguous (128 B).
constexpr int kColTilesPerWave = 4;
constexpr int kWavesPerBlock = 4;
constexpr int kColTilesPerBlock = kColTilesPerWave * kWavesPerBlock;

// One 64-row x 64-column tile, fully unrolled over the columns (B is a compile-time constant so
// the own-bit constant and the v_writelane lane select are immediates).
typedef double d2 __attribute__((ext_vector_type(2)));

template <int MODE>
struct ColTile {
  static constexpr int kPf = 3;         // software prefetch distance (columns)
  const double* cb;                     // LDS: this wave's 64 column points, 6 doubles each
  d2 pf[kPf][3];                        // prefetched column points (registers)
  int cb_addr;                          // LDS byte address of cb

  // 3 x ds_read_b128 of column C (48 B), broadcast: every lane reads the same address
  template <int C>
  __device__ __forceinline__ void load_col(d2 (&slot)[3]) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(slot[0]) : "v"(cb_addr), "n"(48 * C));
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(slot[1]) : "v"(cb_addr), "n"(48 * C + 16));
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(slot[2]) : "v"(cb_addr), "n"(48 * C + 32));
  }
  double six, siy, siz, dix, diy, diz;  // row point (per lane)
  unsigned int own_lo, own_hi;          // this lane's row word
  int tr_lo, tr_hi;                     // lane b: ballot of column b (the transposed word)
  uint64_t unc_cols;                    // wave-uniform: columns to redo with the exact predicate

  template <int B>
  __device__ __forceinline__ void step(const EdgeConst& kc) {
    // Column point B was prefetched kPf steps ago into slot S; wait for it (LDS returns in order,
    // so the younger prefetches stay in flight), then refill the slot with column B + kPf.
    // The loads and waits are inline asm because the compiler otherwise sinks every LDS read to
    // just before its use (no latency hiding); the "+v" operands order the uses after the wait.
    constexpr int S = B % kPf;
    constexpr int younger = 3 * ((63 - B) < (kPf - 1) ? (63 - B) : (kPf - 1));
    asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(pf[S][0]), "+v"(pf[S][1]), "+v"(pf[S][2]) : "n"(younger));
    const double sjx = pf[S][0].x, sjy = pf[S][0].y, sjz = pf[S][1].x;
    const double djx = pf[S][1].y, djy = pf[S][2].x, djz = pf[S][2].y;
    if (B + kPf < 64) load_col<B + kPf>(pf[S]);
    bool e;
    uint64_t m;
    if (MODE == 0) {
      bool unc, shortp;
      const bool neg = tim_edge_fast(sjx - six, sjy - siy, sjz - siz, djx - dix, djy - diy,
                                     djz - diz, kc, &unc, &shortp);
      // columns holding an uncertain lane are redone exactly after the tile (scalar bookkeeping)
      unc_cols |= (__builtin_amdgcn_ballot_w64(unc) != 0ull) ? (1ull << B) : 0ull;
      // each compare writes its lane mask straight to an SGPR pair; OR them as scalars
      m = __builtin_amdgcn_ballot_w64(neg) | __builtin_amdgcn_ballot_w64(shortp);
      e = neg | shortp;
    } else {
      // reference TIM is v_j - v_i with i < j; in the transposed direction the norms are equal
      e = tim_edge_scaled(sjx - six, sjy - siy, sjz - siz, djx - dix, djy - diy, djz - diz, kc);
      m = __builtin_amdgcn_ballot_w64(e);
    }
    // consume the mask NOW (the empty asm pins the accumulators in VGPRs; without it the
    // compiler keeps all 64 masks live in SGPRs and spills them)
    if (B < 32) {
      own_lo |= e ? (1u << (B & 31)) : 0u;
      asm volatile("" : "+v"(own_lo));
    } else {
      own_hi |= e ? (1u << (B & 31)) : 0u;
      asm volatile("" : "+v"(own_hi));
    }
    // lane B keeps the ballot: v_writelane_b32 (no clang builtin on this toolchain)
    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(tr_lo) : "s"((int)(unsigned int)m), "n"(B));
    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(tr_hi) : "s"((int)(unsigned int)(m >> 32)), "n"(B));
  }
  template <int... Bs>
  __device__ __forceinline__ void run(const EdgeConst& kc, std::integer_sequence<int, Bs...>) {
    (step<Bs>(kc), ...);
  }
};

// Logical block -> (row tile I, column group X).  Row tile fastest, so the blocks in flight share a
// column group.  XCD-aware remap (hardware deals consecutive workgroup ids round-robin over the 8
// XCDs): inside every run of 128 ids, the 16 logical neighbours (16 consecutive row tiles of one
// column group = the writers of one 128-B line of transposed words) are given the same XCD, so
// their 8-byte partial writes merge in that XCD's L2; every XCD still gets 16 of each 128 blocks.
__device__ __forceinline__ void tim_block_coords(int gx, int gy, int* I, int* X) {
  const int nblk = gx * gy;
  const int pid = blockIdx.x;
  int lid = pid;
  if (pid < (nblk & ~127)) lid = (pid & ~127) | ((pid & 7) << 4) | ((pid >> 3) & 15);
  *I = lid % gy;
  *X = lid / gy;
}

// FP64 path of one wave: 64 rows (row tile I) x kColTilesPerWave column tiles from Jbase.
template <int MODE>
__device__ __forceinline__ void tim_wave_fp64(const double* __restrict__ ps,
                                              const double* __restrict__ pd,
                                              uint64_t* __restrict__ bm, int n, int W, int I,
                                              int Jbase, const EdgeConst& kc, double* cbw) {
  const int T = W, S = bm_stride(W);  // tiles = words of a row; words between two rows
  const int lane = threadIdx.x & 63;
  const int i = I * 64 + lane;
  const bool vi = i < n;
  const int ic = vi ? i : n - 1;
  const double six = ps[3 * ic], siy = ps[3 * ic + 1], siz = ps[3 * ic + 2];
  const double dix = pd[3 * ic], diy = pd[3 * ic + 1], diz = pd[3 * ic + 2];
  const uint64_t rowmask = (n - I * 64 >= 64) ? ~0ull : ((1ull << (n - I * 64)) - 1ull);

  for (int s = 0; s < kColTilesPerWave; ++s) {
    const int J = Jbase + s;
    if (J < I || J >= T) continue;
    const int j0 = J * 64;
    // stage the tile's 64 column points in LDS (lane b -> column j0+b, clamped to n-1)
    {
      const int jc = min(j0 + lane, n - 1);
      double* w = cbw + 6 * lane;
      w[0] = ps[3 * jc]; w[1] = ps[3 * jc + 1]; w[2] = ps[3 * jc + 2];
      w[3] = pd[3 * jc]; w[4] = pd[3 * jc + 1]; w[5] = pd[3 * jc + 2];
    }
    ColTile<MODE> ct;
    ct.cb = cbw;
    ct.six = six; ct.siy = siy; ct.siz = siz; ct.dix = dix; ct.diy = diy; ct.diz = diz;
    ct.own_lo = 0; ct.own_hi = 0; ct.tr_lo = 0; ct.tr_hi = 0; ct.unc_cols = 0;
    ct.cb_addr = (int)(uintptr_t)cbw;  // LDS aperture: the low 32 bits are the LDS byte address
    // every staging ds_write above must have been ISSUED before the asm reads (in-order LDS)
    asm volatile("" ::: "memory");
    ct.template load_col<0>(ct.pf[0]);
    ct.template load_col<1>(ct.pf[1]);
    ct.template load_col<2>(ct.pf[2]);
    ct.run(kc, std::make_integer_sequence<int, 64>());
    uint64_t own = ((uint64_t)ct.own_hi << 32) | ct.own_lo;
    uint64_t trw = ((uint64_t)(unsigned int)ct.tr_hi << 32) | (unsigned int)ct.tr_lo;
    if (MODE == 0) {
      // exact redo of the (very rare) columns with a lane inside the guard band
      uint64_t todo = ct.unc_cols;
      while (todo) {
        const int b = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int jc = min(j0 + b, n - 1);
        const bool e = tim_edge_exact(ps[3 * jc] - six, ps[3 * jc + 1] - siy, ps[3 * jc + 2] - siz,
                                      pd[3 * jc] - dix, pd[3 * jc + 1] - diy, pd[3 * jc + 2] - diz,
                                      kc.beta);
        const uint64_t m = __ballot(e);
        own = (own & ~(1ull << b)) | ((uint64_t)(e ? 1 : 0) << b);
        trw = (lane == b) ? m : trw;
      }
    }
    // masks applied once per tile: columns / rows beyond n, and the diagonal
    const uint64_t colmask = (n - j0 >= 64) ? ~0ull : ((1ull << (n - j0)) - 1ull);
    own &= colmask;
    if (J == I) own &= ~(1ull << lane);
    if (vi) bm[(int64_t)i * S + J] = own;
    if (J != I && j0 + lane < n) {
      bm[(int64_t)(j0 + lane) * S + I] = trw & rowmask;
    }
    // the rows' padding words: zeroed by the wave of the row tile's last column tile (every row tile has one)
    if (J == T - 1 && vi)
      for (int w = T; w < S; ++w) bm[(int64_t)i * S + w] = 0ull;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void tim_graph_kernel(const ProbDesc* __restrict__ descs,
                                                        const double* __restrict__ src,
                                                        const double* __restrict__ dst,
                                                        uint64_t* __restrict__ bitmap,
                                                        double beta, int gx, int gy,
                                                        const ProbState* __restrict__ states) {
  const ProbDesc d = descs[blockIdx.y];
  const int n = d.n, W = d.W;
  const int T = W;  // row/column tiles of 64
  int I, X;
  tim_block_coords(gx, gy, &I, &X);
  if (I >= T) return;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int Jbase = (X * kWavesPerBlock + wave) * kColTilesPerWave;
  if (Jbase + kColTilesPerWave - 1 < I || Jbase >= T) return;  // below the diagonal / outside

  __shared__ __attribute__((aligned(16))) double cbuf[kWavesPerBlock][64 * 6];
  EdgeConst kc;
  kc.beta = beta;
  kc.beta2 = beta * beta;
  kc.m2beta2 = -2.0 * kc.beta2;
  kc.beta4 = kc.beta2 * kc.beta2;
  kc.s_hat = 1.0;
  if (MODE == 1) kc.s_hat = states[blockIdx.y].scale;
  tim_wave_fp64<MODE>(src + 3 * d.pt_off, dst + 3 * d.pt_off, bitmap + d.bm_off, n, W, I, Jbase, kc,
                      cbuf[wave]);  // cbuf[wave] is private to this wave: no block barrier needed
}

// ==========================================================================================
// K1 on the matrix cores (fixed-scale predicate).  The squared TIM norms are small dense contractions
// (|s_j - s_i|^2 = n_i + n_j - 2 s_i.s_j), so the terms of the predicate that are LINEAR in them come out of the
// matrix pipe for a 32 x 32 tile of pairs at a time; the f32 result is a FILTER whose sign is trusted only outside
// a rigorous error band, everything inside the band is re-evaluated with the reference expression in FP64
// (tim_fixup_group_kernel), so the bitmap stays bit-identical to the oracle.  Points are centred (and scaled) per
// problem and rounded to f32 by the pre-pass; every f32 coordinate is split into two fp16 pieces (x = x_h + x_m
// to 2^-22 relative, 11 + 11 significant bits) and the products that matter are laid out along K; every
// fp16 x fp16 product is exact in f32, only the accumulation rounds (hardware model: every internal addition errs
// by at most one f32 ulp of the sum of |terms|; scripts/probe/mfma_f16_error.hip measures the instruction's own
// figure).  Geometry the filter cannot resolve (beta tiny or huge against the cloud, non-finite input)
// => that problem runs the FP64 body (tim_wave_fp64) instead, chosen per problem on the device; n > 65536 (16-bit
// worklist indices) => the host launches tim_graph_kernel<0>.
// Two earlier formulations (A, B from the matrix pipe; u / w with a per-value band) are archived, not compiled:
// scripts/probe/experiments/k1_formulations_1_2.hip.txt.
// ==========================================================================================
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

struct TimPrep {         // per problem, zeroed then filled by the pre-pass
  // bounding boxes as order-preserving uint images of the f32 coordinates (atomicMax only):
  // hi[k] = max key(v), lo[k] = max ~key(v)  (k = 0..2 src xyz, 3..5 dst xyz)
  unsigned int hi[6];
  unsigned int lo[6];
  unsigned int r2_bits;  // max |centred f32 point|^2 over both clouds (float bits, atomicMax)
  // the problem's counted segment of the fix-up worklist (items; written by the host: tim_prep_fill_segments)
  unsigned int seg_off_lo, seg_off_hi, seg_cap;
  // band constant C and route of the matrix-core filter (tim_prep_consts_kernel, once per problem: worked out per
  // WAVE inside K1 -- a square root, four divisions, ~240 dependent VALU instructions -- it was a tenth of the
  // kernel's vector work and the head of every wave's set-up chain)
  float band_c;
  int use_mfma;
  unsigned int pad[2];
};

__device__ __forceinline__ unsigned int f32_key(float f) {  // monotone float -> uint
  const unsigned int b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float f32_unkey(unsigned int k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// centre of a problem's cloud c (0 src, 1 dst), axis k: any finite value is valid (the error
// analysis uses the rounded CENTRED coordinates), so the f32 bounding box is enough
__device__ __forceinline__ double prep_centre(const TimPrep* pr, int c, int k) {
  const float hi = f32_unkey(pr->hi[3 * c + k]), lo = f32_unkey(~pr->lo[3 * c + k]);
  const double mid = 0.5 * ((double)lo + (double)hi);
  return (mid == mid && fabs(mid) < 1e300) ? mid : 0.0;
}

__global__ __launch_bounds__(256) void tim_prep_bbox_kernel(const ProbDesc* __restrict__ descs,
                                                            const double* __restrict__ src,
                                                            const double* __restrict__ dst,
                                                            TimPrep* __restrict__ prep) {
  const ProbDesc d = descs[blockIdx.y];
  const double* ps = src + 3 * d.pt_off;
  const double* pd = dst + 3 * d.pt_off;
  unsigned int hi[6] = {0, 0, 0, 0, 0, 0}, lo[6] = {0, 0, 0, 0, 0, 0};
  for (int i = blockIdx.x * 1024 + threadIdx.x; i < min(d.n, (int)(blockIdx.x + 1) * 1024); i += 256)
    for (int k = 0; k < 3; ++k) {
      const unsigned int a = f32_key((float)ps[3 * i + k]), b = f32_key((float)pd[3 * i + k]);
      hi[k] = max(hi[k], a);
      lo[k] = max(lo[k], ~a);
      hi[3 + k] = max(hi[3 + k], b);
      lo[3 + k] = max(lo[3 + k], ~b);
    }
  for (int k = 0; k < 6; ++k) {
    for (int o = 32; o > 0; o >>= 1) {
      hi[k] = max(hi[k], (unsigned int)__shfl_xor((int)hi[k], o, 64));
      lo[k] = max(lo[k], (unsigned int)__shfl_xor((int)lo[k], o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      if (hi[k]) atomicMax(&prep[blockIdx.y].hi[k], hi[k]);
      if (lo[k]) atomicMax(&prep[blockIdx.y].lo[k], lo[k]);
    }
  }
}

// (a & m) | (b & ~m) as ONE v_bfi / v_bitop3
__device__ __forceinline__ unsigned int bit_select(unsigned int m, unsigned int a, unsigned int b) {
  return __builtin_amdgcn_bitop3_b32(m, a, b, 0xCA);  // (written with & | ^ the compiler re-associates three selects into nine instructions)
}
// The epilogue's column bits of one lane arrive as four bytes {bit 7: row 3 of group g, bits 6..3: junk (exponent bits
// that came along with the sign), bits 2..0: rows 2, 1, 0}.  lo = the bytes of lane half h = 0 (rows 8 g + 0..3), hi =
// those of h = 1 (rows 8 g + 4..7) -> the column's 32 row bits in order.  Every select masks the junk off.
__device__ __forceinline__ unsigned int merge_gap_bytes(unsigned int lo, unsigned int hi) {
  const unsigned int even = bit_select(0x07070707u, lo, lo >> 4);  // nibble 2 g = rows 8 g + 0..3 (odd nibbles: junk)
  const unsigned int odd = bit_select(0x70707070u, hi << 4, hi);   // nibble 2 g + 1 = rows 8 g + 4..7
  return bit_select(0x0F0F0F0Fu, even, odd);
}

// Offset of a buffer store / atomic that must do nothing: beyond every descriptor's num_records (bitmaps stay
// below 2^31 bytes for n <= 65536) and ALIGNED -- a misaligned no-return atomic (e.g. 0xffffffff) raises a
// memory violation instead of being dropped by the range check.
constexpr unsigned int kOobOffset = 0x80000000u;

// Block = 4 waves = 4 consecutive row tiles (64 rows each) x kMfmaColTiles 64-column tiles.
constexpr int kMfmaRowTiles = 4;
constexpr int kMfmaColTiles = 8;

constexpr int kWorkBuf = 64 * 6;  // per-wave LDS staging (the FP64 path's column buffer): 384 items
// u / w kernels: every wave owns a region of the worklist per column chunk: a count word + 63 items (fixup_regions.h;
// the constant band flags ~5 lane-tiles per region at the bench geometry, none above 18: profiles/r8a)
using fxr::kRegionItems;
using fxr::kRegionWords;
static_assert(fxr::kChunkTiles == kMfmaColTiles && fxr::kRowTiles == kMfmaRowTiles, "fixup_regions.h mirrors the block shape");

// ------------------------------------------------------------------------------------------
// Operands and band constants of the u / w algebra
//
// With A = |s_j - s_i|^2 (src), B = |d_j - d_i|^2 (dst):   | sqrt A - sqrt B | <= beta
//   <=>  sqrt A + sqrt B <= beta   or   d := u^2 + w <= 0,   u = B - A - beta^2,  w = -4 beta^2 A
// (d = (x^2 - beta^2)(S^2 - beta^2) with x = sqrt B - sqrt A, S = sqrt A + sqrt B).  Both u and w are LINEAR in
// the Gram terms, so they come straight out of the matrix pipe.  The operands are fp16: 11 significant bits, so TWO
// round-to-nearest pieces h + m carry an f32 coordinate to 2^-22 relative and only the products h h', h m', m h' are
// needed.  The kernel computes the pair (X, Y) = (w / kappa^2, u / kappa), kappa = 4 beta^2, with TWO chained
// v_mfma_f32_32x32x16_f16 per 32 x 32 tile: the first link sums -A / kappa over 15 K slots (9 coordinate products,
// the squared norms n_i, n_j in three exact pieces each), the second adds (B - beta^2) / kappa over 16 (9 products,
// m_i, m_j, beta^2 / kappa = 1/4), and Y^2 + X = d / kappa^2 has the sign of d.  Two row operands per row half, two
// 1-KB column-operand loads per half tile.  (Archived: the formulation with w as a third MFMA over the chain's first
// column operand, scripts/probe/experiments/k1_three_mfma_uw.patch, and the bf16 one before it -- three pieces, four
// MFMAs, three loads -- k1_bf16_three_piece.patch.)
// The points are centred and scaled per problem by g 2^s: g in (1, sqrt 2] such that kappa = 4 (g beta)^2 is a power
// of two -- every factor 1 / kappa is then an exponent shift of the values behind the operand pieces, exact -- and 2^s
// (k1c::norm_shift, from the bounding boxes) such that the largest half extent lies in [16, 32): fp16 has 5 exponent
// bits, and in this window every piece stays below 65504 (squared norms <= 8192) while the low pieces keep the
// precision the budget assumes (a piece below 2^-14 is subnormal and rounds to a multiple of 2^-24: an ABSOLUTE error
// with its own term).  What the window cannot hold -- kappa outside [2^-17, 2^15], R^2 > 8192 -- fails the admission
// test and runs the FP64 body.  The error budget (eps_y = (640 u R^2) / kappa + sub_y, eps_x = (200 u R^2) / kappa +
// sub_y / 2), the band constants and the admission test are in k1_consts.h (consts_xy), term by term, derived in the
// kappa-multiplied units u = kappa Y, w = kappa^2 X of the lines below; host programs evaluate the same code.
//   per-value band (admission only): with lam = 2 beta R, eta = eps_u / lam:
//     |d~ - d*| <= [ (eta + u) |d~| + eta |w~| + K0' ] / (1 - eta), K0' = eps_u lam + eps_u^2 + eps_w (1 + eta);
//   short pairs: S <= beta implies A, B <= beta^2, hence u* in [-2 beta^2, 0], w* in [-4 beta^4, 0] and |d*| <= 4 beta^4;
//     the band is at least that bound plus the error terms: they go to the fix-up, where the reference expression decides.
// ==========================================================================================

// Packed operands of one 64-point tile (tile t of a problem = points 64 t .. 64 t + 63, padded with copies of the
// problem's last point; tiles are indexed like the bitmap's row words, ProbDesc.w_off + t): 128 B per
// correspondence, 8 KB per tile.  Laid out so that the 64 lanes of a wave -- lane = (h, c), c = point within a
// 32-point group, lane half h holding K slots 8h..8h+7 -- load 1 KB of CONSECUTIVE memory per MFMA operand:
// [32-point group][MFMA][h][c].  (A first layout with 128 B per point made every such load touch 32 separate
// 128-B lines: the vector L1 was the kernel's hidden bottleneck.)
struct TimOperandTile2 {
  uint4 a[2][2][2][32];  // row side: the chain's two operands (K slots 0..15: X, 16..31: Y - X)
  uint4 b[2][2][2][32];  // column side: the same slots
};
constexpr int kTimColOperands = 2;
constexpr int kTimRowOperands = 2;

// fp16 bits of v, round to nearest even, subnormals kept (v_cvt_f16_f32 under the kernel's default denormal mode)
__device__ __forceinline__ unsigned short f16_bits(float v) { return __builtin_bit_cast(unsigned short, (_Float16)v); }
__device__ __forceinline__ float f16_value(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
// two / three fp16 pieces of an f32: v = h + m (+ l) + r.  Two pieces: |r| <= max(2^-22 |v|, 2^-25); three: r = 0
// for |v| >= 1/2 and |r| <= 2^-25 below (the differences are exact in f32)
__device__ __forceinline__ void f16_split3(float v, float* h, float* m, float* l) {
  *h = f16_value(f16_bits(v));
  const float r1 = v - *h;
  *m = f16_value(f16_bits(r1));
  *l = f16_value(f16_bits(r1 - *m));
}
// largest half extent of the two clouds' f32 bounding boxes
__device__ __forceinline__ double prep_half_extent(const TimPrep* pr) {
  double H = 0.0;
  for (int k = 0; k < 6; ++k) {
    const float hi = f32_unkey(pr->hi[k]), lo = f32_unkey(~pr->lo[k]);
    const double e = 0.5 * ((double)hi - (double)lo);
    H = e > H ? e : H;  // (NaN never enters)
  }
  return H;
}

__global__ __launch_bounds__(256) void tim_prep_pack2_kernel(const ProbDesc* __restrict__ descs,
                                                             const double* __restrict__ src,
                                                             const double* __restrict__ dst,
                                                             TimPrep* __restrict__ prep,
                                                             TimOperandTile2* __restrict__ ops,
                                                             int32_t* __restrict__ deg, double beta) {
  const ProbDesc d = descs[blockIdx.y];
  const int ip = blockIdx.x * 256 + threadIdx.x;  // padded point index
  float mx = 0.f;
  if (ip < d.W * 64 && d.n > 0) {
    double g;
    int kexp;
    k1c::scale(beta, &g, &kexp);
    const int i = min(ip, d.n - 1);
    const TimPrep* pr = prep + blockIdx.y;
    const int sh = k1c::norm_shift(prep_half_extent(pr));
    kexp += 2 * sh;  // kappa of the normalised system
    g *= k1c::pow2_d(sh);
    const double* a = src + 3 * (d.pt_off + i);
    const double* b = dst + 3 * (d.pt_off + i);
    const float sx = (float)((a[0] - prep_centre(pr, 0, 0)) * g), sy = (float)((a[1] - prep_centre(pr, 0, 1)) * g),
                sz = (float)((a[2] - prep_centre(pr, 0, 2)) * g);
    const float dx = (float)((b[0] - prep_centre(pr, 1, 0)) * g), dy = (float)((b[1] - prep_centre(pr, 1, 1)) * g),
                dz = (float)((b[2] - prep_centre(pr, 1, 2)) * g);
    // squared norms of the f32 points, exact in double up to its own rounding
    const double na_d = ((double)sx * sx + (double)sy * sy) + (double)sz * sz;
    const double nb_d = ((double)dx * dx + (double)dy * dy) + (double)dz * dz;
    const float na = (float)na_d, nb = (float)nb_d;
    // K slots (k1_consts.h, "The X / Y formulation").  Every slot product carries 2^-kexp = 1 / kappa: the values are
    // shifted by exact powers of two BEFORE they are split (coordinates 2^-ra on the row side and 2^-rb on the column
    // side, the squared norms 2^-pa against P = 2^-pb), so the pieces are those of the unshifted value wherever they
    // stay normal fp16 numbers, and a subnormal piece is rounded once (the budget's absolute terms).
    //   slot    A (row i)                          B (column j)
    //   3c+0    h(s_c 2^-ra)                       2 h(s_c 2^-rb)
    //   3c+1    h(s_c 2^-ra)                       2 m(s_c 2^-rb)
    //   3c+2    m(s_c 2^-ra)                       2 h(s_c 2^-rb)          c = 0, 1, 2
    //   9-11    -h, -m, -l (n_i 2^-pa)             P
    //   12-14   P                                  -h, -m, -l (n_j 2^-pa)
    //   15      0                                  0                       first link:  X = -A / kappa
    //   16+3c   h, h, m (d_c 2^-ra)                -2 h, -2 m, -2 h (d_c 2^-rb)
    //   25-27   h, m, l (m_i 2^-pa)                P
    //   28-30   P                                  h, m, l (m_j 2^-pa)
    //   31      -1/4                               1                       second link: Y = X + (B - beta^2) / kappa
    // (n = |s|^2, m = |d|^2 of the normalised f32 points)
    int ra, rb, pa, pb;
    k1c::xy_shifts(kexp, &ra, &rb, &pa, &pb);
    const float fra = (float)k1c::pow2_d(-ra), frb = (float)k1c::pow2_d(-rb), fpa = (float)k1c::pow2_d(-pa);
    const unsigned short P = f16_bits((float)k1c::pow2_d(-pb));
    unsigned short A[32], B[32];
    for (int k = 0; k < 32; ++k) A[k] = B[k] = 0;
    const float cs[3] = {sx, sy, sz}, cd[3] = {dx, dy, dz};
    float h, m, l;
    for (int c = 0; c < 3; ++c) {
      f16_split3(cs[c] * fra, &h, &m, &l);  // -A contributes +2 s.s'
      A[3 * c] = f16_bits(h); A[3 * c + 1] = A[3 * c]; A[3 * c + 2] = f16_bits(m);
      f16_split3(cs[c] * frb, &h, &m, &l);
      B[3 * c] = f16_bits(2.0f * h); B[3 * c + 1] = f16_bits(2.0f * m); B[3 * c + 2] = B[3 * c];
      f16_split3(cd[c] * fra, &h, &m, &l);  // +B contributes -2 d.d'
      A[16 + 3 * c] = f16_bits(h); A[16 + 3 * c + 1] = A[16 + 3 * c]; A[16 + 3 * c + 2] = f16_bits(m);
      f16_split3(cd[c] * frb, &h, &m, &l);
      B[16 + 3 * c] = f16_bits(-2.0f * h); B[16 + 3 * c + 1] = f16_bits(-2.0f * m); B[16 + 3 * c + 2] = B[16 + 3 * c];
    }
    f16_split3(na * fpa, &h, &m, &l);
    A[9] = f16_bits(-h); A[10] = f16_bits(-m); A[11] = f16_bits(-l); B[9] = P; B[10] = P; B[11] = P;
    B[12] = A[9]; B[13] = A[10]; B[14] = A[11]; A[12] = P; A[13] = P; A[14] = P;
    f16_split3(nb * fpa, &h, &m, &l);
    A[25] = f16_bits(h); A[26] = f16_bits(m); A[27] = f16_bits(l); B[25] = P; B[26] = P; B[27] = P;
    B[28] = A[25]; B[29] = A[26]; B[30] = A[27]; A[28] = P; A[29] = P; A[30] = P;
    A[31] = 0xb400;  // -1/4 = -beta^2 / kappa
    B[31] = 0x3c00;  // 1
    TimOperandTile2* tile = ops + d.w_off + (ip >> 6);
    const int gq = (ip >> 5) & 1, cc = ip & 31;
    for (int mf = 0; mf < kTimRowOperands; ++mf)
      for (int hh = 0; hh < 2; ++hh) {
        const unsigned short* pa = A + 16 * mf + 8 * hh;
        tile->a[gq][mf][hh][cc] = make_uint4(pa[0] | ((unsigned int)pa[1] << 16), pa[2] | ((unsigned int)pa[3] << 16),
                                             pa[4] | ((unsigned int)pa[5] << 16), pa[6] | ((unsigned int)pa[7] << 16));
        if (mf >= kTimColOperands) continue;
        const unsigned short* pb = B + 16 * mf + 8 * hh;
        tile->b[gq][mf][hh][cc] = make_uint4(pb[0] | ((unsigned int)pb[1] << 16), pb[2] | ((unsigned int)pb[3] << 16),
                                             pb[4] | ((unsigned int)pb[5] << 16), pb[6] | ((unsigned int)pb[7] << 16));
      }
    mx = na > nb ? na : nb;
    if (!(mx == mx)) mx = INFINITY;  // NaN coordinates: force the FP64 path
    if (ip < d.n) deg[d.pt_off + ip] = 0;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float t = __shfl_xor(mx, o, 64);
    mx = t > mx ? t : mx;
  }
  if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(&prep[blockIdx.y].r2_bits, __float_as_uint(mx));
}

#ifdef TEASER_K1_LAB
// Lab build only: the u / w formulation of rounds 7 - 9 -- w = -kappa A as a THIRD MFMA over the chain's first column
// operand, kappa-shifted row pieces, constants k1c::consts -- kept as a variant (TEASER_K1_VARIANT + 10000) for A/B runs
// inside one binary: 160 B per correspondence, three row operands.  The product packs the X / Y operands above.
struct TimOperandTile3 {
  uint4 a[2][3][2][32];  // row side: the u chain's two operands, then the w MFMA's
  uint4 b[2][2][2][32];  // column side: two operands -- the w MFMA multiplies the u chain's FIRST one again
};
__global__ __launch_bounds__(256) void tim_prep_pack3_kernel(const ProbDesc* __restrict__ descs,
                                                             const double* __restrict__ src,
                                                             const double* __restrict__ dst,
                                                             TimPrep* __restrict__ prep,
                                                             TimOperandTile3* __restrict__ ops,
                                                             int32_t* __restrict__ deg, double beta) {
  const ProbDesc d = descs[blockIdx.y];
  const int ip = blockIdx.x * 256 + threadIdx.x;  // padded point index
  float mx = 0.f;
  if (ip < d.W * 64 && d.n > 0) {
    double g;
    int kexp;
    k1c::scale(beta, &g, &kexp);
    const int i = min(ip, d.n - 1);
    const TimPrep* pr = prep + blockIdx.y;
    const int sh = k1c::norm_shift(prep_half_extent(pr));
    kexp += 2 * sh;  // kappa of the normalised system
    g *= k1c::pow2_d(sh);
    const double* a = src + 3 * (d.pt_off + i);
    const double* b = dst + 3 * (d.pt_off + i);
    const float sx = (float)((a[0] - prep_centre(pr, 0, 0)) * g), sy = (float)((a[1] - prep_centre(pr, 0, 1)) * g),
                sz = (float)((a[2] - prep_centre(pr, 0, 2)) * g);
    const float dx = (float)((b[0] - prep_centre(pr, 1, 0)) * g), dy = (float)((b[1] - prep_centre(pr, 1, 1)) * g),
                dz = (float)((b[2] - prep_centre(pr, 1, 2)) * g);
    // squared norms of the f32 points, exact in double up to its own rounding
    const double na_d = ((double)sx * sx + (double)sy * sy) + (double)sz * sz;
    const double nb_d = ((double)dx * dx + (double)dy * dy) + (double)dz * dz;
    const float na = (float)na_d, nb = (float)nb_d;
    const double beta2s = k1c::pow2_d(kexp - 2);  // (normalised beta)^2 = kappa / 4, exact
    const float kappa = (float)k1c::pow2_d(kexp);
    const float delta_row = (float)(nb_d - na_d - beta2s);  // m_i - n_i - beta^2 (this point as a ROW)
    const float delta_col = (float)(nb_d - na_d);           // m_j - n_j          (this point as a COLUMN)
    // K slots.  Column side B[0..31] = the two operands of the u chain; row side A[0..31] the u chain's, A[32..47]
    // the w MFMA's, which runs over the FIRST column operand B[0..15] again: that operand holds exactly what w needs
    // from a column point -- the (h, m, h) pieces of the src coordinates, its squared-norm pieces and kappa -- and
    // every other factor that is w's alone sits on the row side, which stays in registers.
    //   slot   B (column j)                        A, u chain (row i)         A, w (row i)
    //   3c+0   2 h(s_c)                            h(s_c)                     kappa h(s_c)
    //   3c+1   2 m(s_c)                            h(s_c)                     kappa h(s_c)
    //   3c+2   2 h(s_c)                            m(s_c)                     kappa m(s_c)          c = 0, 1, 2
    //   9,10   -h(n_j), -m(n_j)                    0                          kappa
    //   11-13  1                                   h, m, l (m_i - n_i - b^2)  0
    //   14,15  kappa                               0                          -h(n_i), -m(n_i)
    //   16+3c  -2 h(d_c), -2 m(d_c), -2 h(d_c)     h, h, m (d_c)                                     (second operand)
    //   25-27  h, m, l (m_j - n_j)                 1
    // (kappa h etc. are rounded to fp16 once more only where they are subnormal: below 2^-14; kappa as a column
    // slot is exact for 2^-24 <= kappa <= 2^15, which the admission test requires)
    unsigned short A[48], B[32];
    for (int k = 0; k < 48; ++k) A[k] = 0;
    for (int k = 0; k < 32; ++k) B[k] = 0;
    const float cs[3] = {sx, sy, sz}, cd[3] = {dx, dy, dz};
    const unsigned short one = 0x3c00;
    float h, m, l;
    for (int c = 0; c < 3; ++c) {
      f16_split3(cs[c], &h, &m, &l);  // -A contributes +2 s.s'
      B[3 * c] = f16_bits(2.0f * h); B[3 * c + 1] = f16_bits(2.0f * m); B[3 * c + 2] = B[3 * c];
      A[3 * c] = f16_bits(h); A[3 * c + 1] = A[3 * c]; A[3 * c + 2] = f16_bits(m);
      // w = -kappa n_i - kappa n_j + 2 kappa s.s': products (h,h') (h,m') (m,h'), kappa on the row side
      A[32 + 3 * c] = f16_bits(kappa * h); A[32 + 3 * c + 1] = A[32 + 3 * c]; A[32 + 3 * c + 2] = f16_bits(kappa * m);
      f16_split3(cd[c], &h, &m, &l);  // +B contributes -2 d.d'
      B[16 + 3 * c] = f16_bits(-2.0f * h); B[16 + 3 * c + 1] = f16_bits(-2.0f * m); B[16 + 3 * c + 2] = B[16 + 3 * c];
      A[16 + 3 * c] = f16_bits(h); A[16 + 3 * c + 1] = A[16 + 3 * c]; A[16 + 3 * c + 2] = f16_bits(m);
    }
    f16_split3(na, &h, &m, &l);
    B[9] = f16_bits(-h); B[10] = f16_bits(-m);      // -n_j
    A[32 + 9] = f16_bits(kappa); A[32 + 10] = A[32 + 9];
    B[11] = one; B[12] = one; B[13] = one;
    B[14] = f16_bits(kappa); B[15] = B[14];
    A[32 + 14] = f16_bits(-h); A[32 + 15] = f16_bits(-m);  // -n_i (times the column's kappa)
    f16_split3(delta_row, &h, &m, &l);
    A[11] = f16_bits(h); A[12] = f16_bits(m); A[13] = f16_bits(l);
    f16_split3(delta_col, &h, &m, &l);
    A[25] = one; A[26] = one; A[27] = one; B[25] = f16_bits(h); B[26] = f16_bits(m); B[27] = f16_bits(l);
    TimOperandTile3* tile = ops + d.w_off + (ip >> 6);
    const int gq = (ip >> 5) & 1, cc = ip & 31;
    for (int mf = 0; mf < 3; ++mf)
      for (int hh = 0; hh < 2; ++hh) {
        const unsigned short* pa = A + 16 * mf + 8 * hh;
        tile->a[gq][mf][hh][cc] = make_uint4(pa[0] | ((unsigned int)pa[1] << 16), pa[2] | ((unsigned int)pa[3] << 16),
                                             pa[4] | ((unsigned int)pa[5] << 16), pa[6] | ((unsigned int)pa[7] << 16));
        if (mf >= kTimColOperands) continue;
        const unsigned short* pb = B + 16 * mf + 8 * hh;
        tile->b[gq][mf][hh][cc] = make_uint4(pb[0] | ((unsigned int)pb[1] << 16), pb[2] | ((unsigned int)pb[3] << 16),
                                             pb[4] | ((unsigned int)pb[5] << 16), pb[6] | ((unsigned int)pb[7] << 16));
      }
    mx = na > nb ? na : nb;
    if (!(mx == mx)) mx = INFINITY;  // NaN coordinates: force the FP64 path
    if (ip < d.n) deg[d.pt_off + ip] = 0;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float t = __shfl_xor(mx, o, 64);
    mx = t > mx ? t : mx;
  }
  if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(&prep[blockIdx.y].r2_bits, __float_as_uint(mx));
}
#endif  // TEASER_K1_LAB

// ==========================================================================================
// K1, the matrix-core filter ("min |d|"): the u / w algebra and operands above, with the error band taken off the
// per-pair path.  Per accumulator value the VALU issues 2.5 instructions:
//   d = fma(u, u, w)                         (the provisional edge bit is sign(d), collected by one v_alignbit)
//   m = min3(m, |d_0|, |d_1|)                (one v_min3_f32 per two values: the smallest |d| of the lane's 16 pairs
//                                             of a 32 x 32 tile)
// and ONE compare per lane and tile decides whether any of those 16 pairs could lie inside the error band
// (m <= C).  Such a lane-tile is a GROUP item for the FP64 fix-up: (problem, column, 16 rows 4h + (q & 3) + 8 (q >> 2)
// of a 32-row half tile); tim_fixup_group_kernel evaluates the reference expression for all 16 pairs and flips the
// bits (and degrees) that differ from the provisional ones.  Nothing is parked in LDS: the lane's group flags of
// the whole block row (8 column tiles x 4 half tiles = 32 bits) live in one register.
//
// The band is a CONSTANT per problem (a per-value band K2 |w| + K0 flags four times fewer lane-tiles but costs one more
// fma per value: measured slower).  In the scaled system of the operands (eps_u, eps_w = kappa eps_A as above;
// u~ = u* + e_u, w~ = w* + e_w, d~ = fl(u~^2 + w~)):  |w*| <= kappa (2R)^2 = (4 beta R)^2 =: Wm.
//   (A) |u*| <= U0 := 4 beta R (1 + 1e-3) + 2 eps_u:  |u~^2 + w~ - d*| <= 2 U0 eps_u + eps_u^2 + eps_w =: E, so
//       |d~| > C >= (E + G) / (1 - 4u) implies sign(d~) = sign(d*) and |d*| > G (the gap between the reference's
//       rounded double predicate and the exact one);
//   (B) |u*| >  U0:  d* >= U0^2 - Wm > 0 (not an edge), and u~^2 + w~ >= (U0 - eps_u)^2 - Wm - eps_w > 0 as well
//       (eps_w = 5200 u beta^2 R^2 << 2e-3 Wm): the provisional bit is right whatever |d~| is.
//   Short pairs (S <= beta, the one region where the sign of d misleads) have |d~| <= short_d <= C: always a group.
// Self pairs (u = -beta^2, w = 0, d = beta^4 <= C) would flag every lane of a diagonal tile: the diagonal column tile
// of a wave runs a second copy of the loop body that leaves them out of the minimum.
// The kernel's registers hold Y = u / kappa and X = w / kappa^2 (operands above), its d is Y^2 + X = d / kappa^2 and
// the band constant it compares with is C / kappa^2 (k1c::consts_xy): the lines above read the same in either unit
// (short pairs |d| / kappa^2 <= 1/4, self pairs 1/16).
// ==========================================================================================
__global__ void tim_prep_consts_kernel(TimPrep* __restrict__ prep, int batch, double beta) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= batch) return;
  const k1c::ConstsXY c = k1c::consts_xy(beta, k1c::norm_shift(prep_half_extent(prep + p)), prep[p].r2_bits);
  prep[p].band_c = c.C;
  prep[p].use_mfma = c.use_mfma;
}
#ifdef TEASER_K1_LAB
__global__ void tim_prep_consts3_kernel(TimPrep* __restrict__ prep, int batch, double beta) {  // (the UW3 variant's)
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= batch) return;
  const k1c::Consts c = k1c::consts(beta, k1c::norm_shift(prep_half_extent(prep + p)), prep[p].r2_bits);
  prep[p].band_c = c.C;
  prep[p].use_mfma = c.use_mfma;
}
#endif

// worklist item: 16 rows of one column and their provisional bits (fixup_item.h; tim_fixup_group_kernel)

// The open-only rebuild's search for its problem (tim_graph_mfma3_kernel with NS = kK1Rebuild): the ord-th problem of
// the batch that the closure left open and that ran the matrix-core body, or -1.  Every wave of the workgroup scans
// the states itself, one ballot per 64 problems: no list, no buffer, no launch in front.
__device__ __forceinline__ int k1_rebuild_find_open(const ProbState* __restrict__ states, const TimPrep* __restrict__ prep,
                                                    const int batch, int ord) {
  const int ln = (int)(threadIdx.x & 63);
  for (int base = 0; base < batch; base += 64) {
    const int b = base + ln;
    const bool open = b < batch && !states[b].deg_closed && prep[b].use_mfma;
    uint64_t m = __builtin_amdgcn_ballot_w64(open);
    const int cnt = __builtin_popcountll(m);
    if (ord < cnt) {
      for (int k = 0; k < ord; ++k) m &= m - 1ull;  // (wave-uniform)
      return base + (int)__builtin_ctzll(m);
    }
    ord -= cnt;
  }
  return -1;
}
// the rebuild's next pass: the workgroup's next logical block of its problem, then (open-only) its next problem
__device__ __forceinline__ bool k1_rebuild_next(int& lb, const int nlb, int& ord, unsigned int& pb, const int rb_open,
                                                const ProbState* __restrict__ states, const TimPrep* __restrict__ prep,
                                                const ProbDesc* __restrict__ descs, ProbDesc& d, int& n, int& W, int& T, int& S) {
  if ((lb += (int)gridDim.x) < nlb) return true;
  if (!rb_open) return false;
  ord += (int)gridDim.y;
  const int found = k1_rebuild_find_open(states, prep, rb_open, ord);
  if (found < 0) return false;
  pb = (unsigned int)found;
  lb = (int)blockIdx.x;
  d = descs[pb];
  n = d.n, W = d.W, T = W, S = bm_stride(W);
  return true;
}

// The product's instantiation (launch_tim_graph_mfma); the lab build (scripts/probe/k1_lab) times the others.
constexpr bool kK1Pipe = false, kK1Plain = true;
constexpr int kK1Chunks = 1, kK1Occ = 3;
constexpr int kRebuildOpenSlots = 2;  // the open-only rebuild's grid: open problems served side by side

// PIPE: software-pipelined schedule.  The wave works on QUARTER tiles (32 x 32) with two accumulator sets: while the
// matrix pipe runs the two MFMAs of quarter k + 1, the vector ALU runs the epilogue of quarter k -- interleaved
// inside the one wave (sched_group_barrier: one MFMA, then a share of the epilogue), across the column tiles of the
// loop as well.  The flat schedule (PIPE = false: 4 MFMAs, then both epilogues) relies on the other two waves of the
// SIMD to fill the matrix pipe's shadow.
// PLAIN: d = fma(u, u, w) as one v_fma_f32 per value instead of one v_pk_fma_f32 per two (MI355X_MICROARCH.md prices
// a packed f32 instruction beside MFMAs above two plain ones).  Measured (profiles/r5a/k1_lab.jsonl, 64 x 10 k, kernel
// alone): flat + packed 0.693 ms, flat + PLAIN 0.658, PIPE + packed 0.719, PIPE + plain 0.697; CHUNKS 2 / 4 with the
// flat schedule 0.74 / 0.81 (packed), 0.72 / 0.73 (plain); under the two-lane pipeline 0.876 (packed) / 0.846 (plain).
// OCC = 4 (the 128-VGPR build, four workgroups per CU: lab variants 1000 / 1010) spills 264 bytes, 14 scratch
// accesses per column tile: 1.01 ms packed, 1.26 ms plain (profiles/r5p) -- the fourth wave needs a kernel with a
// smaller live set (one accumulator set, row operands in LDS), not a register cap.
// CHUNKS: column chunks (of kMfmaColTiles tiles) a block walks with the same four waves.
// LOWER: the transposed words (the bitmap's lower triangle) are stored.  Without it the flush behind the loop still
// counts them for the degrees and issues neither of their stores: a bitmap row r is then valid from word r / 64 on, and
// what lies in front of it is whatever an earlier batch left there.  The route whose only reader of the bitmap is the
// degree closure runs so (solver.hip); tim_mirror_lower_kernel rebuilds the lower triangle for whoever else reads it.
// UW3 (lab build only, flat schedule): the three-MFMA u / w formulation on TimOperandTile3 operands, for A/B runs
// against the X / Y chain inside one binary; d is then in the units of u^2 + w and the band constant k1c::consts's.
// NS (the third store mode; with LOWER = false): kK1NoStore -- no row is stored at all.  The loop, the transposes and
// the degree counting are the storing kernel's; the flush stores the one own word of the wave's DIAGONAL tile (both
// directions of its 64 x 64 pairs: the fix-up reads the provisional bits of that tile's items there, K1 parks zero
// for them), no other own word, no padding, no transposed word.  The route behind it (solver.hip) is the one on which
// the closure evaluates the pairs of its candidate set itself (tim_closure_pairs_kernel) and nobody reads a row.
// kK1Rebuild (with LOWER = true) -- the rows of such a batch rebuilt on demand from the handle's own operand arena:
// the full store, nothing written to the regions, the segment counters or the states, the degrees added into a
// scratch array nobody reads; problems on the FP64 body (their rows are in place) and, with rb_open, problems the
// closure has decided are skipped, and a block walks the logical blocks lb, lb + gridDim.x, .. of the nlb_arg a
// problem has.  The open-only launch has the grid of ONE problem x kRebuildOpenSlots slots, whatever the batch's size:
// a workgroup finds the open problems itself (k1_rebuild_find_open) and serves every kRebuildOpenSlots-th of them.
// Measured (profiles/r12a, r13a): on K1's own grid x batch the workgroups of an all-closed batch leave at once and
// cost 14 us alone, but each still needs a K1-sized slot (144 VGPRs x 4 waves, 34 KB of LDS), and in the two-lane
// pipeline those slots are held by the OTHER lane's K1 -- the launch then ends with that K1 and the lane's tail behind
// it: the bench fell 1.4 % BELOW the parent.  64 workgroups x batch (the form up to r12a) walked one open problem's 420
// blocks in 7 passes, up to 245 us; 128 and 210 x batch lost 1.7 % and 6 % against it; one problem x 2 slots gained
// 3.0 %.  tim_fixup_replay_kernel puts the fix-up's recorded answers on top.
constexpr int kK1NoStore = 1, kK1Rebuild = 2;
template <bool PIPE, bool PLAIN, int OCC, int CHUNKS, bool LOWER, bool UW3 = false, int NS = 0>
__global__ __launch_bounds__(256, OCC) void tim_graph_mfma3_kernel(
    const ProbDesc* __restrict__ descs, const double* __restrict__ src,
    const double* __restrict__ dst, const void* __restrict__ ops, const TimPrep* __restrict__ prep,
    uint64_t* __restrict__ bitmap, double beta, int gyr,
    unsigned long long* __restrict__ work, unsigned int* __restrict__ work_count,
    ProbState* __restrict__ states, int32_t* __restrict__ deg, unsigned long long* __restrict__ regions, int Tmax,
    int rb_open, int nlb_arg) {
  static_assert(NS == 0 || (NS == kK1NoStore && !LOWER) || (NS == kK1Rebuild && LOWER), "store modes");
  // The problem: blockIdx.y, except in the open-only rebuild (rb_open = the batch's size), whose grid is the size of
  // ONE problem times gridDim.y slots: workgroup (x, y) serves the y-th, (y + gridDim.y)-th, .. open problem of the
  // batch and finds it by scanning the batch's states itself (k1_rebuild_find_open); without one it leaves at once.
  unsigned int pb = blockIdx.y;
  int ord = (int)blockIdx.y;
  if constexpr (NS == kK1Rebuild) {  // (uniform over the block)
    if (rb_open) {
      const int found = k1_rebuild_find_open(states, prep, rb_open, ord);
      if (found < 0) return;
      pb = (unsigned int)found;
    } else if (!prep[pb].use_mfma) {
      return;
    }
  }
  ProbDesc d = descs[pb];
  int n = d.n, W = d.W;
  int T = W, S = bm_stride(W);  // tiles = words of a bitmap row; words between two rows
  // One pass per logical block.  Every instantiation but the rebuild's makes exactly one (lb = blockIdx.x; the loop's
  // condition is constant false and `continue` is its early exit), so the body below is not indented for it.
  int lb = (int)blockIdx.x;
  const int nlb = NS == kK1Rebuild ? nlb_arg : (int)gridDim.x;
  do {
  // block decode: only the blocks that touch the upper triangle are launched (column group X has
  // min(gyr, 2 CHUNKS (X + 1)) row groups; blockIdx.x enumerates them), in an XCD-aware order: workgroups go to the
  // 8 XCDs round robin in dispatch order, so the blocks of one XCD take CONSECUTIVE logical indices -- the four
  // neighbouring row groups whose transposed words fill one 128-byte line of a bitmap row run on the same XCD at
  // about the same time and merge in that L2, and a column group's operands are fetched into one L2 instead of eight
  // (fxr::decode_block, fixup_regions.h: the host test of the region arena runs the same decode)
  int Ig, X;
  fxr::decode_block(lb, nlb, gyr, CHUNKS, &Ig, &X);
  // a block = 4 row tiles x CHUNKS chunks of kMfmaColTiles column tiles, walked chunk after chunk by the same four
  // waves: a wave's set-up (descriptors, band constants, row operands: three dependent memory round trips) and its
  // wind-down (the last stores' acknowledgement) took 40 % of its lifetime when it lived for 8 column tiles only
  // (s_memtime trace, profiles/r4f); column group X has min(gyr, 2 CHUNKS (X + 1)) row groups
  constexpr int kBlockColTiles = kMfmaColTiles * CHUNKS;
  const int I0 = Ig * kMfmaRowTiles, Jbase = X * kBlockColTiles;
  // The wave's region of chunk c is the CELL (row tile I0 + wave, column chunk X CHUNKS + c) of the problem's arena
  // (fixup_regions.h), addressed by what it covers and not by where the launch grid put the wave: the fix-up finds all
  // regions of a row tile as one run.  Cells exist in the upper triangle of the batch's largest problem (Tmax tiles)
  // only; every cell a wave owns gets a count word on every path, also on the early exits (the arena is not cleared).
  auto region_of = [&](int wv, int chunk) -> unsigned long long* {
    if constexpr (NS == kK1Rebuild) return nullptr;  // (the arena keeps the items the fix-up has recorded its answers in)
    const int Iw = I0 + wv, Xc = X * CHUNKS + chunk;
    return fxr::is_cell(Iw, Xc, Tmax) ? regions + fxr::region_offset((int)pb, Tmax, Iw, Xc) : nullptr;
  };
  auto zero_regions = [&]() {
    if ((threadIdx.x & 63) < CHUNKS) {
      unsigned long long* r = region_of((int)(threadIdx.x >> 6), (int)(threadIdx.x & 63));
      if (r) r[0] = 0ull;
    }
  };
  if (I0 >= T || Jbase >= T || Jbase + kBlockColTiles - 1 < I0) {  // outside / below the diagonal
    zero_regions();
    continue;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int I = I0 + wave;

  const double* __restrict__ ps = src + 3 * d.pt_off;
  const double* __restrict__ pd = dst + 3 * d.pt_off;
  uint64_t* __restrict__ bm = bitmap + d.bm_off;
  // ONE LDS array (18 KB per workgroup): the wave's own words of all its column tiles, staged so that every global
  // store covers whole 64-byte runs.  The FP64 body's column buffer and the group-item staging of the harvest reuse
  // the wave's slice (neither is live together with the own words).
  __shared__ __attribute__((aligned(16))) uint64_t lds_own[kMfmaRowTiles][64][kMfmaColTiles + 1];  // +1: conflict-free
  static_assert(sizeof(lds_own[0]) >= sizeof(double) * 64 * 6 && sizeof(lds_own[0]) >= 8 * kWorkBuf, "aliased buffers");
  // the transposed words of the whole block row are parked here ([column tile][row][wave]: the four waves' words of
  // a bitmap row are 32 contiguous bytes) and written behind the loop, so that the loop's only vector-memory
  // operations are the operand loads (stored per column tile -- a 64-line scattered store + a degree atomic per wave
  // and tile -- every other operand wait of the loop also waited for their acknowledgement: gfx9 counts loads and
  // stores on ONE in-order vmcnt)
  __shared__ __attribute__((aligned(16))) uint64_t lds_tr[kMfmaColTiles][64][kMfmaRowTiles];
  // (the operand loads are issued before the band constants are worked out: they are harmless on the FP64 route)
  // one operand tile: kRowOps row operands, then kTimColOperands column operands, per 32-point group (TimOperandTile2;
  // the lab's UW3 variant: TimOperandTile3)
  constexpr int kRowOps = UW3 ? 3 : kTimRowOperands;
  constexpr int kTileBytes = 2 * (kRowOps + kTimColOperands) * 1024, kColBase = 2 * kRowOps * 1024;
  static_assert(UW3 || (kTileBytes == (int)sizeof(TimOperandTile2) && kColBase == (int)offsetof(TimOperandTile2, b)), "tile layout");
  const char* __restrict__ qt = reinterpret_cast<const char*>(ops) + (size_t)d.w_off * kTileBytes;
  const int h = lane >> 5, c = lane & 31;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t q_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)qt, 0, (int)((unsigned int)T * (unsigned int)kTileBytes), 0x00020000);
  auto load_op = [&](int tile, int side, int g, int m) -> uint4 {  // side 0 = a (rows), 1 = b (columns): m = 0..1
    const int soff = tile * kTileBytes + (side ? kColBase + (g * kTimColOperands + m) * 1024 : (g * kRowOps + m) * 1024);
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(q_rsrc, lane * 16, soff, 0);
    return make_uint4(v.x, v.y, v.z, v.w);
  };
  f16x8 ar[2][kRowOps];
  {
    const int It = min(I, T - 1);
    for (int rt = 0; rt < 2; ++rt)
      for (int m = 0; m < kRowOps; ++m) ar[rt][m] = __builtin_bit_cast(f16x8, load_op(It, 0, rt, m));
  }
  const bool rowvalid = I < T;
  const uint64_t rowmask = !rowvalid ? 0ull : (n - I * 64 >= 64) ? ~0ull : ((1ull << (n - I * 64)) - 1ull);
  const int Jfirst = max(Jbase, I), Jend = min(Jbase + kBlockColTiles, T);  // the wave's column tiles, all chunks
  uint4 bX[kTimColOperands], bY[kTimColOperands];  // column operands: X = the tile's first 32 columns (ct 0), Y = the other 32 (PIPE only)
  {
    const int Jf = min(Jfirst, T - 1);
    for (int m = 0; m < kTimColOperands; ++m) bX[m] = load_op(Jf, 1, 0, m);
    if (PIPE)
      for (int m = 0; m < kTimColOperands; ++m) bY[m] = load_op(Jf, 1, 1, m);
  }
  const TimPrep pr = prep[pb];  // (uniform address: scalar loads)
  if (!pr.use_mfma) {  // per problem: uniform over the block
    EdgeConst kc;
    kc.beta = beta;
    kc.beta2 = beta * beta;
    kc.m2beta2 = -2.0 * kc.beta2;
    kc.beta4 = kc.beta2 * kc.beta2;
    kc.s_hat = 1.0;
    if (I < T)
      for (int jb = Jbase; jb < Jbase + kBlockColTiles; jb += kColTilesPerWave)
        if (!(jb + kColTilesPerWave - 1 < I || jb >= T))
          tim_wave_fp64<0>(ps, pd, bm, n, W, I, jb, kc, reinterpret_cast<double*>(&lds_own[wave][0][0]));
    zero_regions();
    continue;
  }
  const __amdgpu_buffer_rsrc_t deg_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(deg + d.pt_off), 0, (int)((unsigned int)n * 4u), 0x00020000);
  const __amdgpu_buffer_rsrc_t bm_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)bm, 0, (int)((unsigned int)n * (unsigned int)S * 8u), 0x00020000);
  int degacc = 0;
  // the value of a diagonal 32 x 32 tile (ct == rt) that is this lane's self pair: row 4h + (q & 3) + 8 (q >> 2) == c
  const int cq = c - 4 * h;
  const int selfq = (cq >= 0 && (cq & 4) == 0) ? ((cq & 3) | ((cq >> 3) << 2)) : -1;
  unsigned int flags = 0;  // one bit per (active column tile, ct, rt) in issue order, youngest in bit 0
  const float thr = pr.band_c;

  struct Acc {
    f32x16 U, W;  // U = Y = u / kappa (the chain's end), W = X = w / kappa^2 (its first link, which stays live)
  };
  // the two chained MFMAs of one 32 x 32 quarter tile: X = -A / kappa over K slots 0..15, Y = X + (B - beta^2) / kappa
  // over 16..31, written to registers of its own
  static_assert(!(UW3 && PIPE), "the three-MFMA lab variant has the flat schedule only");
  auto mf = [&](Acc& a, const f16x8(&arow)[kRowOps], const uint4(&b)[kTimColOperands]) {
    f32x16 z;
    for (int k = 0; k < 16; ++k) z[k] = 0.f;
    a.W = __builtin_amdgcn_mfma_f32_32x32x16_f16(arow[0], __builtin_bit_cast(f16x8, b[0]), z, 0, 0, 0);
    a.U = __builtin_amdgcn_mfma_f32_32x32x16_f16(arow[1], __builtin_bit_cast(f16x8, b[1]), a.W, 0, 0, 0);
  };
  // epilogue of one quarter tile: the lane's 16 provisional column bits (sign of d = u^2 + w) and the group flag
  auto epi = [&](const Acc& a, bool self_tile) -> unsigned int {
    unsigned int colbits = 0;
    float m = INFINITY;
#pragma unroll
    for (int qp = 7; qp >= 0; --qp) {  // descending q: bit q of the word = register q
      float d0, d1;
      if (PLAIN) {
        d0 = __builtin_fmaf(a.U[2 * qp], a.U[2 * qp], a.W[2 * qp]);
        d1 = __builtin_fmaf(a.U[2 * qp + 1], a.U[2 * qp + 1], a.W[2 * qp + 1]);
      } else {
        const f32x2 u2 = {a.U[2 * qp], a.U[2 * qp + 1]}, w2 = {a.W[2 * qp], a.W[2 * qp + 1]};
        const f32x2 d2 = __builtin_elementwise_fma(u2, u2, w2);
        d0 = d2.x;
        d1 = d2.y;
      }
      float v0 = __builtin_fabsf(d0), v1 = __builtin_fabsf(d1);
      if (self_tile) {
        v0 = (selfq == 2 * qp) ? INFINITY : v0;
        v1 = (selfq == 2 * qp + 1) ? INFINITY : v1;
      }
      m = __builtin_fminf(__builtin_fminf(m, v0), v1);
      // value 2 qp + 1 opens a group of four rows when qp is odd: it enters with FIVE bits (its sign on top of four
      // exponent bits), which leaves a gap that the merge of the two lane halves masks off (finish_tile)
      colbits = __builtin_amdgcn_alignbit(colbits, __float_as_uint(d1), (qp & 1) ? 27 : 31);
      colbits = __builtin_amdgcn_alignbit(colbits, __float_as_uint(d0), 31);
    }
    // flags = 2 flags + !(m > thr): the compare's lane mask is the carry-in of flags + flags (the compiler's own
    // sequence was compare, select, shift, or)
    asm("v_cmp_nlt_f32_e32 vcc, %2, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(flags) : "v"(m), "s"(thr) : "vcc");
    return colbits;
  };
  // stage j = 16 of the bit transposes: after v_permlane16_swap(x, x) the first result holds {own, partner} and the
  // second {partner, own} in the {even, odd} rows of 16 lanes; one byte permute builds the stage's output
  const unsigned int sel16 = (lane & 16) ? 0x03020706u : 0x01000504u;
  // a column tile's four quarter words -> transposed words (lower triangle) and own words (LDS), degrees
  auto finish_tile = [&](const int J, const bool diag, const unsigned int (&tr)[2][2]) {
    const int j0 = J * 64;
    // lane (c, h) holds rows 4h + (q&3) + 8(q>>2) of column (ct, c); after the half swap lanes 0-31 hold column
    // (0, c) and lanes 32-63 column (1, c) = column `lane`
    unsigned int tw[2], ow[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      // r[0]: the 16 bits of half h = 0 (rows 8 g + 0..3 of the column), r[1]: those of h = 1 (rows 8 g + 4..7)
      const auto r = __builtin_amdgcn_permlane32_swap(tr[0][rt], tr[1][rt], false, false);
      tw[rt] = merge_gap_bytes(r[0], r[1]);
      // row-major words = the 32 x 32 bit transpose of the column words inside each half: 5 butterfly stages over
      // lane distance j = 16 .. 1 (the lower lane of a pair keeps x & m and takes (partner << j) & ~m, the upper one
      // keeps x & ~m and takes (partner >> j) & m).  The partner's word comes through the VALU's own cross-lane
      // paths -- v_permlane16_swap + one byte permute for j = 16, DPP moves for 8 (row_ror:8), 4 (row_half_mirror,
      // then the quads reversed), 2 and 1 (quad_perm) -- not through ds_swizzle: ten LDS round trips per column tile
      // in a dependent chain were the part of the epilogue no schedule could hide.
      unsigned int x;
      {
        const auto sw = __builtin_amdgcn_permlane16_swap(tw[rt], tw[rt], false, false);
        x = __builtin_amdgcn_perm(sw[0], sw[1], sel16);
      }
#pragma unroll
      for (int st = 1; st < 5; ++st) {
        const int j = 16 >> st;
        unsigned int p;
        switch (st) {
          case 1: p = __builtin_amdgcn_update_dpp(0u, x, 0x128, 0xf, 0xf, true); break;  // row_ror:8
          case 2:
            p = __builtin_amdgcn_update_dpp(0u, x, 0x141, 0xf, 0xf, true);   // row_half_mirror: lane ^ 7
            p = __builtin_amdgcn_update_dpp(0u, p, 0x1b, 0xf, 0xf, true);    // quad_perm [3,2,1,0]: lane ^ 3
            break;
          case 3: p = __builtin_amdgcn_update_dpp(0u, x, 0x4e, 0xf, 0xf, true); break;   // quad_perm [2,3,0,1]
          default: p = __builtin_amdgcn_update_dpp(0u, x, 0xb1, 0xf, 0xf, true); break;  // quad_perm [1,0,3,2]
        }
        const bool up = (lane & j) != 0;
        const unsigned int shifted = __builtin_amdgcn_alignbit(p, p, up ? j : 32 - j);
        const unsigned int km[5] = {0x0000FFFFu, 0x00FF00FFu, 0x0F0F0F0Fu, 0x33333333u, 0x55555555u};
        const unsigned int keep = up ? ~km[st] : km[st];
        x = bit_select(keep, x, shifted);
      }
      ow[rt] = x;  // lane (r, half ct): the 32 column bits (ct) of row 32 rt + r
    }
    const auto ro = __builtin_amdgcn_permlane32_swap(ow[0], ow[1], false, false);
    uint64_t ownw = ((uint64_t)ro[1] << 32) | ro[0];
    const uint64_t trw = ((uint64_t)tw[1] << 32) | tw[0];
    const uint64_t colmask = (n - j0 >= 64) ? ~0ull : ((1ull << (n - j0)) - 1ull);
    ownw &= colmask;
    if (diag) ownw &= ~(1ull << lane);
    if (NS != kK1NoStore || diag) lds_own[wave][lane][(J - Jbase) & (kMfmaColTiles - 1)] = ownw;  // (nobody reads the others back)
    degacc += __builtin_popcountll(ownw);
    // rows beyond n hold no bits (clamped: the padding repeats the last point); the diagonal tile has no transposed copy
    const uint64_t trw_out = diag ? 0ull : (trw & rowmask);  // (columns beyond n: the flush stores no such row)
    lds_tr[(J - Jbase) & (kMfmaColTiles - 1)][lane][wave] = trw_out;
  };

  // flat schedule: per 32-column half the 4 MFMAs of both row halves (the two chains interleaved by hand), then the epilogues
  auto body_flat = [&](const int J, auto diag_tag) {
    constexpr bool DIAG = decltype(diag_tag)::value;
    unsigned int tr[2][2];  // [ct][rt]: this lane's 16 column bits
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const f16x8 b0 = __builtin_bit_cast(f16x8, bX[0]), b1 = __builtin_bit_cast(f16x8, bX[1]);
      const int Jn = (ct == 0 || J + 1 >= Jend) ? J : J + 1, gn = ct ^ 1;
      f32x16 z;
      for (int k = 0; k < 16; ++k) z[k] = 0.f;
      Acc acc[2];
      // the MFMA burst and the operand loads behind it are issued at raised priority, the epilogue at the default: a
      // wave's loads win the arbitration against the other waves' vector work (-2 % on the bench step, profiles/r5t;
      // lowering the priority BEFORE the loads, or one level for the whole loop, gains nothing)
      __builtin_amdgcn_s_setprio(2);
      if constexpr (UW3) {  // u's first link into U, then w = the third row operand over the same column operand
        acc[0].U = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[0][0], b0, z, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        acc[1].U = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[1][0], b0, z, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        acc[0].W = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[0][kRowOps - 1], b0, z, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        acc[1].W = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[1][kRowOps - 1], b0, z, 0, 0, 0);
      } else {
        acc[0].W = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[0][0], b0, z, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        acc[1].W = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[1][0], b0, z, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      // each operand of the next half tile is requested right behind the last MFMA that reads its registers: the
      // load's way into the address unit runs beside the matrix pipe (0.592 -> 0.576 ms alone, -0.6 % on the bench
      // step: profiles/r5t/r5t21)
      bX[0] = load_op(Jn, 1, gn, 0);
      __builtin_amdgcn_sched_barrier(0);
      acc[0].U = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[0][1], b1, UW3 ? acc[0].U : acc[0].W, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      acc[1].U = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[1][1], b1, UW3 ? acc[1].U : acc[1].W, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      bX[1] = load_op(Jn, 1, gn, 1);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) tr[ct][rt] = epi(acc[rt], DIAG && ct == rt);
    }
    finish_tile(J, DIAG, tr);
  };

  // pipelined schedule.  Invariant at the top of an iteration: accA holds the MFMA results of quarter (ct 0, rt 0)
  // of column tile J, bX / bY the column operands of J.  Phase k runs the MFMAs of quarter k + 1 beside the epilogue
  // of quarter k; the last phase starts the next column tile (its operands were fetched two phases earlier).
  Acc accA, accB;
  // schedule of one phase: 4 x (1 MFMA, a share of the VALU work)
#define TIM_K1_INTERLEAVE(N)                                                              \
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                      \
  __builtin_amdgcn_sched_group_barrier(0x002, N, 0);                                      \
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                      \
  __builtin_amdgcn_sched_group_barrier(0x002, N, 0);                                      \
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                      \
  __builtin_amdgcn_sched_group_barrier(0x002, N, 0);                                      \
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                      \
  __builtin_amdgcn_sched_group_barrier(0x002, N, 0)
  constexpr int kEpiShare = PLAIN ? 13 : 9;  // VALU instructions of a quarter's epilogue / 4
  auto body_pipe = [&](const int J, auto diag_tag) {
    constexpr bool DIAG = decltype(diag_tag)::value;
    const int Jn = min(J + 1, Jend - 1);  // (the last iteration starts a quarter nobody reads)
    unsigned int tr[2][2];
    mf(accB, ar[1], bX);                  // (ct 0, rt 1)
    tr[0][0] = epi(accA, DIAG);
    TIM_K1_INTERLEAVE(kEpiShare);
    __builtin_amdgcn_sched_barrier(0);
    for (int m = 0; m < kTimColOperands; ++m) bX[m] = load_op(Jn, 1, 0, m);  // X is free: next tile's first half, used in phase 3
    mf(accA, ar[0], bY);                  // (ct 1, rt 0)
    tr[0][1] = epi(accB, false);
    __builtin_amdgcn_sched_group_barrier(0x020, kTimColOperands, 0);
    TIM_K1_INTERLEAVE(kEpiShare);
    __builtin_amdgcn_sched_barrier(0);
    mf(accB, ar[1], bY);                  // (ct 1, rt 1)
    tr[1][0] = epi(accA, false);
    TIM_K1_INTERLEAVE(kEpiShare);
    __builtin_amdgcn_sched_barrier(0);
    for (int m = 0; m < kTimColOperands; ++m) bY[m] = load_op(Jn, 1, 1, m);  // Y is free: next tile's second half, used in phase 1
    mf(accA, ar[0], bX);                  // next tile's (ct 0, rt 0)
    tr[1][1] = epi(accB, DIAG);
    finish_tile(J, DIAG, tr);
    __builtin_amdgcn_sched_group_barrier(0x020, kTimColOperands, 0);
    TIM_K1_INTERLEAVE(kEpiShare + 16);
    __builtin_amdgcn_sched_barrier(0);
  };

#undef TIM_K1_INTERLEAVE
  unsigned long long* wbuf = reinterpret_cast<unsigned long long*>(&lds_own[wave][0][0]);  // private to the wave
  bool primed = false;  // PIPE: accA holds the first quarter of the next column tile
#pragma nounroll
  for (int chunk = 0; chunk < CHUNKS; ++chunk) {
    const int Jc0 = Jbase + chunk * kMfmaColTiles, Jc1 = min(Jc0 + kMfmaColTiles, Jend);
    unsigned long long* const region = region_of(wave, chunk);  // (wave-uniform; null: no such cell)
    if (Jc0 >= Jend) {  // (block-uniform) beyond the problem: no region to resolve
      if (lane == 0 && region) region[0] = 0ull;
      continue;
    }
    const int Ja = rowvalid ? max(Jc0, Jfirst) : Jc1;  // this wave's first column tile of the chunk
    if (Ja < Jc1) {
      int J = Ja;
      if (PIPE) {
        if (!primed) {
          mf(accA, ar[0], bX);
          __builtin_amdgcn_sched_barrier(0);
          primed = true;
        }
        if (J == I) {
          body_pipe(J, std::true_type());
          ++J;
        }
#pragma nounroll
        for (; J < Jc1; ++J) body_pipe(J, std::false_type());
      } else {
        if (J == I) {
          body_flat(J, std::true_type());
          ++J;
        }
#pragma nounroll
        for (; J < Jc1; ++J) body_flat(J, std::false_type());
      }
    }
    const int nact = max(Jc1 - Ja, 0);
    {
      // transposed words of the chunk: thread -> (column tile, row): the four waves' words I0 .. I0 + 3 of bitmap
      // row j (32 contiguous bytes; a word exists where its row tile lies strictly below the column tile), and ONE
      // degree atomic per row for their bits.  (Block-uniform control flow up to here: every wave meets the barriers.)
      __syncthreads();
#pragma unroll
      for (int it = 0; it < (kMfmaColTiles * 64) / 256; ++it) {
        const int idx = it * 256 + (int)threadIdx.x, Jr = idx >> 6, r = idx & 63, J = Jc0 + Jr, j = J * 64 + r;
        const uint4 lo = *reinterpret_cast<const uint4*>(&lds_tr[Jr][r][0]);
        const uint4 hi = *reinterpret_cast<const uint4*>(&lds_tr[Jr][r][2]);
        const bool rowok = J < Jc1 && j < n;
        const unsigned int base = ((unsigned int)j * (unsigned int)S + (unsigned int)I0) * 8u;
        if (Jc0 > I0 + 3 && I0 + 3 < T) {  // (block-uniform) the chunk lies strictly right of all four row tiles
          const int cnt = (__builtin_popcount(lo.x) + __builtin_popcount(lo.y)) + (__builtin_popcount(lo.z) + __builtin_popcount(lo.w)) +
                          (__builtin_popcount(hi.x) + __builtin_popcount(hi.y)) + (__builtin_popcount(hi.z) + __builtin_popcount(hi.w));
          if (LOWER) {
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{lo.x, lo.y, lo.z, lo.w}, bm_rsrc, rowok ? base : kOobOffset, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{hi.x, hi.y, hi.z, hi.w}, bm_rsrc, rowok ? base + 16u : kOobOffset, 0, 0);
          }
          __builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(cnt, deg_rsrc, (rowok && cnt) ? (unsigned int)j * 4u : kOobOffset, 0, 0);
          continue;
        }
        bool ok[4];
        for (int k = 0; k < 4; ++k) ok[k] = rowok && I0 + k < T && I0 + k < J;
        const unsigned int w32[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        int cnt = 0;
        for (int k = 0; k < 4; ++k) cnt += ok[k] ? __builtin_popcount(w32[2 * k]) + __builtin_popcount(w32[2 * k + 1]) : 0;
        if (!LOWER) {  // (counted for the degrees, not stored)
        } else if (ok[3]) {  // (ok[3] implies the other three)
          __builtin_amdgcn_raw_buffer_store_b128(u32x4{lo.x, lo.y, lo.z, lo.w}, bm_rsrc, base, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b128(u32x4{hi.x, hi.y, hi.z, hi.w}, bm_rsrc, base + 16u, 0, 0);
        } else {
          for (int k = 0; k < 3; ++k)
            __builtin_amdgcn_raw_buffer_store_b64(u32x2{w32[2 * k], w32[2 * k + 1]}, bm_rsrc,
                                                  ok[k] ? base + 8u * k : kOobOffset, 0, 0);
        }
        __builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(cnt, deg_rsrc, cnt ? (unsigned int)j * 4u : kOobOffset, 0, 0);
      }
      if (CHUNKS > 1) __syncthreads();  // (the next chunk rewrites lds_tr)
    }
    // own words of the chunk: lanes 8r..8r+7 store the (up to) 8 consecutive words of one row
    if (NS == kK1NoStore) {
      // ... of which this mode stores one: word I of the wave's 64 rows, where the chunk holds its diagonal tile
      if (Ja == I && Ja < Jc1) {
        const uint64_t w = lds_own[wave][lane][(I - Jbase) & (kMfmaColTiles - 1)];
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{(unsigned int)w, (unsigned int)(w >> 32)}, bm_rsrc,
                                              I * 64 + lane < n ? ((unsigned int)(I * 64 + lane) * (unsigned int)S + (unsigned int)I) * 8u : kOobOffset,
                                              0, 0);
      }
    } else if (nact > 0) {
      const int kk = lane & 7, J = Jc0 + kk;
      // (the problem's last chunk ends at the row stride: its words T .. S - 1 are the rows' padding, stored as zeros, so
      // that this run too covers its whole 64 bytes)
      const bool pad = J >= T, colok = (J >= Ja && J < Jc1) || pad;
      const unsigned int off0 = ((unsigned int)(I * 64 + (lane >> 3)) * (unsigned int)S + (unsigned int)J) * 8u;
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int r = it * 8 + (lane >> 3);
        const uint64_t w = pad ? 0ull : lds_own[wave][r][kk];
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{(unsigned int)w, (unsigned int)(w >> 32)}, bm_rsrc,
                                              (colok && I * 64 + r < n) ? off0 + (unsigned int)it * 64u * (unsigned int)S : kOobOffset,
                                              0, 0);
      }
    }
    // ---- group items of the chunk's flagged lane-tiles: one pass over the wave's active column tiles, staged in the
    // wave's LDS slice (the own words are on their way), then the wave's OWN region of the worklist (plain stores, no
    // atomic); only a wave with more items sends the rest through the problem's counted segment.
    int wcount = 0;  // wave-uniform
    if constexpr (NS != kK1Rebuild) {
      // flags: 4 bits per active column tile, the OLDEST tile in the highest nibble; bit 3: (ct 0, rt 0), 2: (0, 1),
      // 1: (1, 0), 0: (1, 1).  Lane-tiles beyond n (padding: copies of the last point) are dropped: rows only in the
      // problem's last row tile, columns only in its last column tile.
      unsigned int vf = flags;
      if (I * 64 + 4 * h >= n) vf &= ~0xAAAAAAAAu;       // rt 0
      if (I * 64 + 32 + 4 * h >= n) vf &= ~0x55555555u;  // rt 1
      if (T - 1 >= Ja && T - 1 < Jc1 && (n & 63)) {
        const int sh = 4 * (Jc1 - T);  // (= nact - 1 - (T - 1 - Ja))
        if ((T - 1) * 64 + c >= n) vf &= ~(0xCu << sh);
        if ((T - 1) * 64 + 32 + c >= n) vf &= ~(0x3u << sh);
      }
      if (__builtin_amdgcn_ballot_w64(vf != 0u) != 0ull) {
        // exclusive prefix of the lanes' item counts, bit by bit through v_mbcnt (no cross-lane dependency chain)
        const int mine = __builtin_popcount(vf);
        int base = 0, total = 0;
#pragma unroll
        for (int bit = 0; bit < 6; ++bit) {
          const uint64_t m = __builtin_amdgcn_ballot_w64(((mine >> bit) & 1) != 0);
          base += (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u)) << bit;
          total += __builtin_popcountll(m) << bit;
        }
        if (total > kWorkBuf) {  // adversarial geometry: the host reruns the batch on the FP64 kernel
          if (lane == 0) states[pb].k1_overflow = 1;
        } else {
          int kk = base;
#pragma nounroll
          while (vf) {
            const int pos = 31 - __builtin_clz(vf);
            vf &= ~(1u << pos);
            const int J = Ja + (nact - 1 - (pos >> 2));
            const int ct = ((pos >> 1) & 1) ^ 1, rt = (pos & 1) ^ 1;
            const unsigned int rowp = (unsigned int)(I * 64 + 32 * rt + 4 * h);
            const unsigned int colp = (unsigned int)(J * 64 + 32 * ct + c);
            // the item's 16 provisional bits: the column's transposed word is still parked in lds_tr (its flush only
            // read it; a diagonal tile parks zero: the fix-up reads those bits from the own words, which hold both
            // directions)
            const uint64_t tword = lds_tr[(J - Jbase) & (kMfmaColTiles - 1)][32 * ct + c][wave];
            wbuf[kk++] = fxi::pack(rowp, colp, fxi::gather_bits(tword, rt, h));
          }
          wcount = total;
        }
      }
    }
    flags = 0;
    if constexpr (NS != kK1Rebuild) {
      // (a wave has items only where its row tile reaches the chunk's columns, i.e. in a cell: region != null then)
      const int nreg = !region ? 0 : (wcount < kRegionItems ? wcount : kRegionItems);
      if (lane == 0 && region) region[0] = (unsigned long long)nreg;
      if (lane < nreg) region[1 + lane] = wbuf[lane];
      if (wcount > nreg) {
        const int extra = wcount - nreg;
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(work_count + pb, (unsigned int)extra);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base + (unsigned int)extra > pr.seg_cap) {
          if (lane == 0) states[pb].k1_overflow = 1;
        } else {
          unsigned long long* seg = work + (((size_t)pr.seg_off_hi << 32) | (size_t)pr.seg_off_lo);
#pragma nounroll
          for (int k2i = lane; k2i < extra; k2i += 64) seg[base + k2i] = wbuf[nreg + k2i];
        }
      }
    }
  }
  if (rowvalid)
    __builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(degacc, deg_rsrc, (unsigned int)(I * 64 + lane) * 4u, 0, 0);
  } while (NS == kK1Rebuild &&  // (`continue` lands here too; the next pass rewrites the LDS arrays)
           (__syncthreads(), k1_rebuild_next(lb, nlb, ord, pb, rb_open, states, prep, descs, d, n, W, T, S)));
}

// FP64 resolution of the filter's GROUP items: 16 lanes per item, lane q owns the pair
// (row0 + (q & 3) + 8 (q >> 2), col).  The bitmap holds the filter's provisional bit sign(d~), and so does the item
// (fixup_item.h); a pair whose reference predicate disagrees flips its bit(s) with one atomicXor each (row-major copy;
// transposed copy outside diagonal blocks, unless K1 left the lower triangle out: `upper`) and the two degrees follow.
// Every bit is owned by exactly one lane of one item, so the plain read of the provisional bit races with nothing.  A WAVE takes a whole ROW TILE: it stages the tile's 64 points once, walks the
// tile's regions (fixup_regions.h: one run of cells, one 64-lane load each -- lane 0: the count word, lane k: item k),
// queues their items in LDS and resolves the queue in dense rounds of 64 items, four items per step, every load of
// a round issued before the first use.  (A wave per REGION -- the layout up to round 7 -- paid the staging, the
// column-side loads, two fences and two half-empty resolve steps for the ~5 items of a region, and staged a row
// tile's points once per column chunk it meets: profiles/r8a.)
// 15 of a group's 16 pairs are far from the boundary: the FP64 fast path (FMA, no sqrt, its own 2e-12 guard band:
// tim_edge_fast) decides them, the reference expression itself only inside that band.
// Overflow (the problem's counted segment was too small): its bitmap is cleared instead (the stages enqueued behind
// K1 see an empty graph, not unresolved, possibly asymmetric bits), the problem is flagged and the host reruns the
// batch on the FP64 kernel.
// mode: kFixUpper -- K1 left the lower triangle out.  NOSTORE -- K1 stored nothing but the diagonal tiles' words
// (kK1NoStore): outside a diagonal tile the provisional bits come with the item on both paths, the staged one and the
// counted segment's, no bitmap bit is flipped and only the two degrees follow; and every item gets the 16 EXACT bits
// of its pairs written back into its own word (one ballot per step, one lane per item).  The worklist arena lives
// until the handle's next solve, so it then holds the reference predicate's answer for every pair the filter could
// not decide: what tim_fixup_replay_kernel puts on top of a rebuilt bitmap without looking at a point.
// NOSTORE is a template parameter, mode carries kFixUpper only: the storing routes' fix-up is then the code it was
// (66 VGPRs, 28 KB of LDS; with a runtime flag every route paid the write-back's 84 VGPRs and the queue's home indices).
constexpr int kFixUpper = 1;
template <bool NOSTORE>
__global__ __launch_bounds__(256) void tim_fixup_group_kernel(const ProbDesc* __restrict__ descs, int batch,
                                                              const double* __restrict__ src,
                                                              const double* __restrict__ dst,
                                                              uint64_t* __restrict__ bitmap, double beta,
                                                              unsigned long long* __restrict__ work,
                                                              const unsigned int* __restrict__ work_count,
                                                              ProbState* __restrict__ states,
                                                              int32_t* __restrict__ deg,
                                                              unsigned long long* __restrict__ regions,
                                                              int Tmax,
                                                              const TimPrep* __restrict__ prep, int mode) {
  TAIL_WAVE_PRIO();
  constexpr bool nostore = NOSTORE;
  const bool upper = nostore || (mode & kFixUpper) != 0;
  const int prob = blockIdx.y;
  const unsigned int total = work_count[prob];
  const TimPrep tpr = prep[prob];
  const unsigned int cap = tpr.seg_cap;
  const ProbDesc d = descs[prob];
  const int n = d.n, W = d.W, S = bm_stride(W);
  if (total > cap) {
    const int64_t words = (int64_t)n * S;  // (padding included: zero like everywhere)
    uint64_t* bm = bitmap + d.bm_off;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (int64_t)gridDim.x * 256) bm[w] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) states[prob].k1_overflow = 1;
    return;
  }
  int32_t* dg = deg + d.pt_off;
  if (!tpr.use_mfma) {
    // this problem ran the FP64 body inside K1 (no filter, no worklist, no degree atomics): its degrees are the row
    // popcounts (what a separate degree launch did for these problems)
    const uint64_t* bm = bitmap + d.bm_off;
    const int lane = threadIdx.x & 63;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += gridDim.x * 4) {
      const uint64_t* r = bm + (int64_t)row * S;
      int c = 0;
      for (int w = lane; w < W; w += 64) c += __popcll(r[w]);
      c = wave_sum_i(c);
      if (lane == 0) dg[row] = c;
    }
    return;
  }
  const double* ps = src + 3 * d.pt_off;
  const double* pd = dst + 3 * d.pt_off;
  unsigned int* bm32 = reinterpret_cast<unsigned int*>(bitmap + d.bm_off);
  EdgeConst kc;
  kc.beta = beta;
  kc.beta2 = beta * beta;
  kc.m2beta2 = -2.0 * kc.beta2;
  kc.beta4 = kc.beta2 * kc.beta2;
  kc.s_hat = 1.0;
  const int lane = threadIdx.x & 63, q = lane & 15, sub = lane >> 4, wave = threadIdx.x >> 6;
  const int rq = (q & 3) + 8 * (q >> 2);
  // STAGED = true (items of the regions): all items of a wave's queue come from ONE 64-row tile.  Its 64 points
  // are staged once per tile in the wave's LDS slice, and outside the diagonal tile the 16 provisional bits of an item
  // come with the item itself.  Per item: one broadcast fetch of the column point, instead of 17 points and 16 words on
  // 16 different bitmap rows (1.8 KB of sectors per item: that traffic, not the arithmetic, was the kernel's 0.175 ms
  // per 64 x 10 k launch).
  __shared__ double row_pts[4][64][6];
  // ... and so are the COLUMN sides of a round's items (round 6): lane k fetches the column point of item k -- six
  // load instructions per round of up to 64 items -- and the 16 lanes of an item read it back from the wave's LDS slice.  (Fetched inside the item loop they were
  // seven instructions per FOUR items, each for four distinct addresses: ~5 M vector-memory instructions per
  // 64 x 10 k batch, two thirds of what K1 itself issues, and on a step bound by the board's power limit the fix-up's
  // energy -- 0.1 J of 1.1 -- is paid for in K1's clock: profiles/r6v, r6w.)
  __shared__ __attribute__((aligned(16))) double col_pts[4][64][6];
  auto resolve = [&](unsigned long long it, bool valid, auto staged, int tile, int slot, unsigned long long* home) {
    constexpr bool STAGED = decltype(staged)::value;
    const bool live = valid;  // (the item exists: `valid` goes on to mean this lane's pair)
    int r = fxi::row0(it) + rq, col = fxi::col(it);
    valid = valid && r < n && col < n && r != col;
    r = valid ? r : (STAGED ? tile * 64 : 0);
    col = valid ? col : 0;
    // every load up front: the two points (and, below, the word that holds the provisional bit where the item does not)
    double sx, sy, sz, dx, dy, dz, cx, cy, cz, ex, ey, ez;
    if (STAGED) {
      const double* rp = row_pts[wave][r & 63];
      sx = rp[0]; sy = rp[1]; sz = rp[2]; dx = rp[3]; dy = rp[4]; dz = rp[5];
      const double* cp = col_pts[wave][slot];
      cx = cp[0]; cy = cp[1]; cz = cp[2]; ex = cp[3]; ey = cp[4]; ez = cp[5];
    } else {
      sx = ps[3 * r]; sy = ps[3 * r + 1]; sz = ps[3 * r + 2];
      dx = pd[3 * r]; dy = pd[3 * r + 1]; dz = pd[3 * r + 2];
      cx = ps[3 * col]; cy = ps[3 * col + 1]; cz = ps[3 * col + 2];
      ex = pd[3 * col]; ey = pd[3 * col + 1]; ez = pd[3 * col + 2];
    }
    unsigned int* wp = bm32 + 2 * ((int64_t)r * S + (col >> 6)) + ((col >> 5) & 1);
    const unsigned int bit = 1u << (col & 31);
    const bool offdiag = (r >> 6) != (col >> 6);
    bool prov;
    if ((STAGED || nostore) && offdiag) {  // (uniform over the valid lanes of an item)
      prov = fxi::bit(it, q);
    } else {
      prov = (*wp & bit) != 0u;
    }
    const double ax = cx - sx, ay = cy - sy, az = cz - sz, bx = ex - dx, by = ey - dy, bz = ez - dz;
    bool unc, shortp;
    bool e = tim_edge_fast(ax, ay, az, bx, by, bz, kc, &unc, &shortp);
    e |= shortp;
    if (unc) e = tim_edge_exact(ax, ay, az, bx, by, bz, beta);
    if constexpr (nostore) {  // the item's word takes its pairs' exact bits: lanes 16 sub .. 16 sub + 15 of the ballot
      const uint64_t em = __builtin_amdgcn_ballot_w64(valid && e);
      if (q == 0 && live) *home = fxi::pack((unsigned int)fxi::row0(it), (unsigned int)fxi::col(it), (unsigned int)(em >> (16 * sub)) & 0xffffu);
    }
    if (!valid || prov == e) return;
    if (!nostore || !offdiag) atomicXor(wp, bit);
    atomicAdd(dg + r, e ? 1 : -1);
    if (offdiag) {  // the transposed copy, where there is one, and the column's degree
      if (!upper) atomicXor(bm32 + 2 * ((int64_t)col * S + (r >> 6)) + ((r >> 5) & 1), 1u << (r & 31));
      atomicAdd(dg + col, e ? 1 : -1);
    }
  };
  // The per-wave item queue: a region adds at most 63 items to fewer than 64 pending ones.
  __shared__ unsigned long long queue[4][2 * kRegionWords];
  static_assert(kRegionWords == 64, "one region = one 64-lane load");
  // (NOSTORE) where a queued item came from: its word's index in the row tile's run of regions (< 2^16: at most
  // 128 chunks of 64 words)
  __shared__ unsigned short qsrc[nostore ? 4 : 1][nostore ? 2 * kRegionWords : 1];
  const int T = W, nch = fxr::n_chunks(T);
  // one round: the first `cnt` (<= 64) items of the queue, all of row tile `tile`, whose regions begin at `run`
  auto round = [&](int cnt, int tile, unsigned long long* run) {
    if (lane < cnt) {  // item `lane`: its column point
      const int col = min(fxi::col(queue[wave][lane]), n - 1);
      double* cp = col_pts[wave][lane];
      const double c0 = ps[3 * col], c1 = ps[3 * col + 1], c2 = ps[3 * col + 2];
      const double e0 = pd[3 * col], e1 = pd[3 * col + 1], e2 = pd[3 * col + 2];
      cp[0] = c0; cp[1] = c1; cp[2] = c2; cp[3] = e0; cp[4] = e1; cp[5] = e2;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // wave-private LDS slices: same-wave ordering suffices
#pragma nounroll
    for (int base = 0; base < cnt; base += 4) {
      const int k = base + sub;
      resolve(queue[wave][k], k < cnt, std::true_type(), tile, k, nostore ? run + qsrc[nostore ? wave : 0][nostore ? k : 0] : nullptr);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the next round overwrites the slices)
  };
  // Row tiles are taken in pairs (p, T - 1 - p): tile I has n_chunks - first_chunk(I) regions, so every pair walks
  // about n_chunks + 1 of them and the four waves of a workgroup finish together.  Waves stride over the pairs: the
  // grid (launch_tim_graph_mfma: a wave per pair of the largest problem, or S_FIXUP_WGS workgroups) may be any size.
  const int wv = blockIdx.x * 4 + wave, nwv = gridDim.x * 4, npairs = (T + 1) >> 1;
  for (int pi = wv; pi < npairs; pi += nwv) {
    for (int side = 0; side < 2; ++side) {
      const int tile = side ? T - 1 - pi : pi;
      if (side && tile == pi) break;  // (the middle tile of an odd T)
      {  // the tile's 64 row points, staged once: lane l holds point 64 tile + l
        const int pr = min(tile * 64 + lane, n - 1);
        double* rp = row_pts[wave][lane];
        rp[0] = ps[3 * pr]; rp[1] = ps[3 * pr + 1]; rp[2] = ps[3 * pr + 2];
        rp[3] = pd[3 * pr]; rp[4] = pd[3 * pr + 1]; rp[5] = pd[3 * pr + 2];
      }
      const int Xc0 = fxr::first_chunk(tile);
      unsigned long long* reg = regions + fxr::region_offset(prob, Tmax, tile, Xc0);
      int qn = 0;  // queued items (wave-uniform), < 64 between regions
      unsigned long long mine = reg[lane];
      for (int Xc = Xc0; Xc < nch; ++Xc) {
        const unsigned long long cur = mine;
        if (Xc + 1 < nch) mine = reg[(size_t)(Xc + 1 - Xc0) * kRegionWords + lane];  // (in flight beside this region's work)
        const int cnt = min((int)__builtin_amdgcn_readfirstlane((unsigned int)cur), kRegionItems);
        if (cnt <= 0) continue;
        // append: the valid lanes are 1 .. cnt, so the exclusive prefix of the valid flags is lane - 1
        if (lane >= 1 && lane <= cnt) {
          queue[wave][qn + lane - 1] = cur;
          if constexpr (nostore) qsrc[wave][qn + lane - 1] = (unsigned short)((Xc - Xc0) * kRegionWords + lane);
        }
        qn += cnt;
        if (qn >= kRegionWords) {
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          round(kRegionWords, tile, reg);
          qn -= kRegionWords;
          const unsigned long long moved = queue[wave][kRegionWords + lane];  // (every lane reads before any writes)
          unsigned short moved_src = 0;
          if constexpr (nostore) moved_src = qsrc[wave][kRegionWords + lane];
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          if (lane < qn) {
            queue[wave][lane] = moved;
            if constexpr (nostore) qsrc[wave][lane] = moved_src;
          }
        }
      }
      if (qn > 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        round(qn, tile, reg);
      }
    }
  }
  unsigned long long* seg = work + (((size_t)tpr.seg_off_hi << 32) | (size_t)tpr.seg_off_lo);
  const unsigned int ngrp = gridDim.x * 16;
  for (unsigned int w = (blockIdx.x * 256 + threadIdx.x) >> 4; w < total; w += ngrp) resolve(seg[w], true, std::false_type(), 0, 0, seg + w);
}

// The recorded answers of a no-store batch's fix-up put on top of the rows K1 has just rebuilt (kK1Rebuild): 16 lanes
// per item; for every pair of an item the recorded bit is the reference predicate's answer and the bit in the bitmap
// the filter's, stored a launch ago; where they differ both copies are flipped (a diagonal tile's pair has one: its
// mirror image is a pair of its own).  No point is loaded, nothing is evaluated, no degree is touched.  A wave takes a
// row tile's run of regions, region after region; the counted segment follows.  open_only: as in K1.
__global__ __launch_bounds__(256) void tim_fixup_replay_kernel(const ProbDesc* __restrict__ descs,
                                                               uint64_t* __restrict__ bitmap,
                                                               const unsigned long long* __restrict__ work,
                                                               const unsigned int* __restrict__ work_count,
                                                               const ProbState* __restrict__ states,
                                                               const unsigned long long* __restrict__ regions,
                                                               int Tmax, const TimPrep* __restrict__ prep, int open_only) {
  const int prob = blockIdx.y;
  const TimPrep tpr = prep[prob];
  const unsigned int total = work_count[prob];
  if (!tpr.use_mfma || total > tpr.seg_cap || (open_only && states[prob].deg_closed)) return;
  const ProbDesc d = descs[prob];
  const int n = d.n, W = d.W, S = bm_stride(W), T = W, nch = fxr::n_chunks(T);
  unsigned int* bm32 = reinterpret_cast<unsigned int*>(bitmap + d.bm_off);
  const int lane = threadIdx.x & 63, q = lane & 15, sub = lane >> 4;
  const int rq = fxi::row_of(q);
  auto replay = [&](unsigned long long it, bool live) {
    const int r = fxi::row0(it) + rq, col = fxi::col(it);
    if (!live || r >= n || col >= n || r == col) return;
    unsigned int* wp = bm32 + 2 * ((int64_t)r * S + (col >> 6)) + ((col >> 5) & 1);
    const unsigned int bit = 1u << (col & 31);
    if (((*wp & bit) != 0u) == fxi::bit(it, q)) return;
    atomicXor(wp, bit);
    if ((r >> 6) != (col >> 6)) atomicXor(bm32 + 2 * ((int64_t)col * S + (r >> 6)) + ((r >> 5) & 1), 1u << (r & 31));
  };
  const int wv = blockIdx.x * 4 + (int)(threadIdx.x >> 6), nwv = gridDim.x * 4;
  for (int tile = wv; tile < T; tile += nwv) {
    const int Xc0 = fxr::first_chunk(tile);
    const unsigned long long* reg = regions + fxr::region_offset(prob, Tmax, tile, Xc0);
    for (int Xc = Xc0; Xc < nch; ++Xc) {
      const unsigned long long cur = reg[(size_t)(Xc - Xc0) * kRegionWords + lane];  // lane 0: the count, lane k: item k
      const int cnt = min((int)__builtin_amdgcn_readfirstlane((unsigned int)cur), kRegionItems);
      for (int base = 0; base < cnt; base += 4) {
        const int k = base + sub;  // item k sits in lane k + 1
        const unsigned long long it = __shfl(cur, min(k + 1, 63));
        replay(it, k < cnt);
      }
    }
  }
  const unsigned long long* seg = work + (((size_t)tpr.seg_off_hi << 32) | (size_t)tpr.seg_off_lo);
  const unsigned int ngrp = gridDim.x * 16;
  for (unsigned int w = (blockIdx.x * 256 + threadIdx.x) >> 4; w < total; w += ngrp) replay(seg[w], true);
}

// Launch 2 of the degree closure where K1 has stored no row (kTimNoStore): the FULL compact rows of the candidate set
// R straight from the points.  For every rank pair a < b the predicate is evaluated ONCE, with the two-step expression
// of the fix-up's resolve() (the FP64 fast path with its guard band, the reference expression inside it: the bit a
// stored row would hold).  A wave takes a 64 x 64 block (A, B >= A) of rank pairs -- the blocks below the diagonal are
// without work -- with the 64 row points staged in its LDS slice (a broadcast read per row) and lane l's column point
// (rank 64 B + l) in registers, and leaves BOTH words of the block: one ballot per row is the row-side word
// (64 A + r, B), and the 64 predicate values lane l sees over the row loop are, bit for bit, the mirrored word
// (64 B + l, A) -- one OR per row.  Off the diagonal lane l stores its row word to comp[64 A + l][B] and its column word
// to comp[64 B + l][A]; the diagonal block stores the OR of the two to comp[64 A + l][A] (zero diagonal).  So every word
// (row < m, block < ng) of the pool is written exactly once per launch, whatever the grid: the verdict launch reads
// full rows and there is neither a zero fill nor a symmetrise launch behind this one.  The points come from the pool
// the order launch staged in rank order (six doubles per rank): contiguous loads, no key is read.  |R| ~ 900 at
// N = 10 k is ~120 blocks, ~0.5 M pairs per problem.
__global__ __launch_bounds__(256) void tim_closure_pairs_kernel(uint64_t* __restrict__ comp_pool /* [batch][kCoreCap][kCoreWords] */,
                                                                const double* __restrict__ pts_pool /* [batch][kCoreCap][6] */,
                                                                const int32_t* __restrict__ counters, double beta) {
  TAIL_WAVE_PRIO();
  const int m = counters[blockIdx.y];
  if (m < 2) return;
  const double* pts = pts_pool + (size_t)blockIdx.y * kCoreCap * 6;
  uint64_t* comp = comp_pool + (size_t)blockIdx.y * kCoreCap * kCoreWords;
  EdgeConst kc;
  kc.beta = beta;
  kc.beta2 = beta * beta;
  kc.m2beta2 = -2.0 * kc.beta2;
  kc.beta4 = kc.beta2 * kc.beta2;
  kc.s_hat = 1.0;
  __shared__ double row_pts[4][64][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ng = (m + 63) >> 6, units = ng * (ng + 1) / 2;
  for (int u = blockIdx.x * 4 + wave; u < units; u += gridDim.x * 4) {
    int A = 0, rem = u;  // row block A has the ng - A blocks A .. ng - 1
    while (rem >= ng - A) {
      rem -= ng - A;
      ++A;
    }
    const int B = A + rem, ra = 64 * A + lane, rb = 64 * B + lane;
    {  // (ranks beyond m: the last rank's point, masked below -- the pool holds nothing there)
      const double* pa = pts + 6 * min(ra, m - 1);
      double* rp = row_pts[wave][lane];
      rp[0] = pa[0]; rp[1] = pa[1]; rp[2] = pa[2];
      rp[3] = pa[3]; rp[4] = pa[4]; rp[5] = pa[5];
    }
    const double* pb = pts + 6 * min(rb, m - 1);
    const double cx = pb[0], cy = pb[1], cz = pb[2];
    const double ex = pb[3], ey = pb[4], ez = pb[5];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // wave-private slice: same-wave ordering suffices
    uint64_t word = 0ull, colw = 0ull;
    const int rows = min(64, m - 64 * A);
    for (int r = 0; r < rows; ++r) {
      const double* rp = row_pts[wave][r];
      const double ax = cx - rp[0], ay = cy - rp[1], az = cz - rp[2], bx = ex - rp[3], by = ey - rp[4], bz = ez - rp[5];
      bool unc, shortp;
      bool e = tim_edge_fast(ax, ay, az, bx, by, bz, kc, &unc, &shortp);
      e |= shortp;
      if (unc) e = tim_edge_exact(ax, ay, az, bx, by, bz, beta);
      const bool valid = rb < m && 64 * A + r < rb;
      const uint64_t mk = __builtin_amdgcn_ballot_w64(e && valid);
      word = lane == r ? mk : word;
      colw |= (uint64_t)(e && valid) << r;
    }
    // (ranks >= m: no row is stored for them, and the mask leaves their bits zero in every word that is)
    if (A == B) {
      if (ra < m) comp[(size_t)ra * kCoreWords + A] = word | colw;
    } else {
      if (ra < m) comp[(size_t)ra * kCoreWords + B] = word;
      if (rb < m) comp[(size_t)rb * kCoreWords + A] = colw;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the next block overwrites the slice)
  }
}

// The lower triangle of a bitmap whose K1 stored the upper one only (LOWER = false), rebuilt on demand: per problem and
// pair of tiles I < J the 64 own words U[64 I + l][J] are read, their 64 x 64 bits transposed and written as
// L[64 J + l][I].  A wave takes a run of kMirrorRun consecutive I of one J -- lane l keeps the words of row 64 J + l
// and stores them as one contiguous run.  The upper triangle is only read: the kernel is idempotent, and harmless on a
// bitmap that holds both halves.  skip_closed: problems the degree closure has decided are left as they are (nobody
// behind the closure reads their rows).
constexpr int kMirrorRun = 8;
__global__ __launch_bounds__(256) void tim_mirror_lower_kernel(const ProbDesc* __restrict__ descs,
                                                               uint64_t* __restrict__ bitmap,
                                                               const ProbState* __restrict__ states, int skip_closed) {
  const ProbDesc d = descs[blockIdx.y];
  const int n = d.n, W = d.W, T = W, S = bm_stride(W);
  if (T < 2 || (skip_closed && states[blockIdx.y].deg_closed)) return;
  const int lane = threadIdx.x & 63;
  const int runs = (T + kMirrorRun - 1) / kMirrorRun;  // runs of row tiles per column tile (those at or beyond J: idle)
  uint64_t* bm = bitmap + d.bm_off;
  for (int wv = blockIdx.x * 4 + (int)(threadIdx.x >> 6); wv < T * runs; wv += gridDim.x * 4) {
    const int J = wv / runs, Ia = (wv % runs) * kMirrorRun, Ib = min(Ia + kMirrorRun, J);
    if (Ia >= Ib) continue;
    uint64_t out[kMirrorRun];
#pragma unroll
    for (int k = 0; k < kMirrorRun; ++k) {
      out[k] = 0ull;
      if (Ia + k >= Ib) continue;  // (wave-uniform)
      // row 64 (Ia + k) + lane < 64 J <= n: every lane has a row
      const uint64_t x = bm[(int64_t)(64 * (Ia + k) + lane) * S + J];
#pragma unroll
      for (int c = 0; c < 64; ++c) {  // bit r of the ballot = bit c of row r's word = bit r of column c's word
        const uint64_t m = __builtin_amdgcn_ballot_w64(((x >> c) & 1ull) != 0ull);
        out[k] = lane == c ? m : out[k];
      }
    }
    const int row = 64 * J + lane;
    if (row < n) {
#pragma unroll
      for (int k = 0; k < kMirrorRun; ++k)
        if (Ia + k < Ib) bm[(int64_t)row * S + Ia + k] = out[k];
    }
  }
}

void launch_tim_graph(hipStream_t s, const ProbDesc* d_desc, int batch, int max_n,
                      const double* d_src, const double* d_dst, uint64_t* d_bitmap,
                      double noise_bound, double cbar2, int mode, const ProbState* d_state) {
  if (batch <= 0 || max_n <= 0) return;
  const int T = (max_n + 63) / 64;
  const double beta = 2 * noise_bound * sqrt(cbar2);  // registration.cc:438 / :421
  const int gx = (T + kColTilesPerBlock - 1) / kColTilesPerBlock, gy = T;
  dim3 grid(gx * gy, batch);
  if (mode == 0)
    hipLaunchKernelGGL(tim_graph_kernel<0>, grid, dim3(256), 0, s, d_desc, d_src, d_dst, d_bitmap,
                       beta, gx, gy, d_state);
  else
    hipLaunchKernelGGL(tim_graph_kernel<1>, grid, dim3(256), 0, s, d_desc, d_src, d_dst, d_bitmap,
                       beta, gx, gy, d_state);
}

// ------------------------------------------------------------------------------------------
// Host side of the matrix-core K1: buffer sizes, the fix-up worklist's layout, the three launches.
// ------------------------------------------------------------------------------------------
int64_t tim_prep_bytes(int batch) { return (int64_t)batch * ((int64_t)sizeof(TimPrep) + 4) + 64; }  // + one worklist counter per problem
#ifdef TEASER_K1_LAB
int64_t tim_operand_bytes(int64_t total_tiles) { return total_tiles * (int64_t)sizeof(TimOperandTile3); }  // (the larger)
#else
int64_t tim_operand_bytes(int64_t total_tiles) { return total_tiles * (int64_t)sizeof(TimOperandTile2); }
#endif

// blocks of the matrix-core kernel for a problem of T 64-point tiles: those touching the upper triangle; a block
// covers 4 row tiles x `chunks` chunks of kMfmaColTiles column tiles
static int tim_mfma_blocks(int T, int chunks) { return fxr::blocks(T, chunks); }
// the region arena's stride per problem: one region per cell (row tile, column chunk) of the largest problem's upper
// triangle (fixup_regions.h) -- the same for every launch geometry, so also the largest of them
static int64_t tim_region_words(int max_n) { return fxr::arena_words((max_n + 63) / 64); }

// Worklist layout in 8-byte words: one counted segment per problem (the overflow of the waves' own regions) sized
// from THAT problem's pair count -- pairs / 256 items, at least 2^16 (typical use: ~1e-3 of the pairs as group items,
// most of them in the regions) -- at prefix offsets, so that one large problem in a batch of small ones gets the
// room it needs (a uniform stride from the batch average sent it to the all-FP64 rerun); then the regions
// (kRegionWords per (row tile, column chunk) cell of the upper triangle, shaped by the largest problem).  A segment that
// overflows flags its problem and the host reruns the batch on the FP64 kernel.
static int64_t tim_segment_items(int n) {
  const int64_t seg = std::max<int64_t>((int64_t)n * (n - 1) / 2 / 256, 1 << 16);
  return std::min<int64_t>(seg, 0x7fffffffll);
}
int64_t tim_work_items(const int32_t* n, int batch) {
  int64_t segs = 0;
  int max_n = 0;
  for (int b = 0; b < batch; ++b) {
    segs += tim_segment_items(n[b]);
    max_n = std::max(max_n, n[b]);
  }
  return segs + tim_region_words(max_n) * std::max(batch, 1);
}
// writes every problem's segment offset / capacity into the (host-staged, otherwise zero) TimPrep records of the
// solve's header block; returns the items all segments take (the regions follow them)
int64_t tim_prep_fill_segments(void* host_prep, const int32_t* n, int batch) {
  TimPrep* pr = reinterpret_cast<TimPrep*>(host_prep);
  int64_t off = 0;
  for (int b = 0; b < batch; ++b) {
    const int64_t seg = tim_segment_items(n[b]);
    pr[b].seg_off_lo = (unsigned int)((uint64_t)off & 0xffffffffu);
    pr[b].seg_off_hi = (unsigned int)((uint64_t)off >> 32);
    pr[b].seg_cap = (unsigned int)seg;
    off += seg;
  }
  return off;
}

// Diagnostic (scripts/probe/k1_probe, mode "work"): the region arena and the segment counters K1 left behind.  With
// regions_out == nullptr only the sizes are returned: the arena's stride per problem in 8-byte words and the regions
// per problem in use (the cells of the largest problem's upper triangle).
int tim_probe_worklist(const void* d_prep, const void* d_work, int64_t work_cap, int batch, int max_n,
                       unsigned long long* regions_out, int64_t* stride_words, int64_t* used_regions,
                       unsigned int* seg_counts) {
  const int64_t reg_words = tim_region_words(max_n);
  *stride_words = reg_words;
  *used_regions = fxr::cells((max_n + 63) / 64);
  if (!regions_out) return 0;
  const unsigned long long* regions = reinterpret_cast<const unsigned long long*>(d_work) + (work_cap - reg_words * (int64_t)batch);
  hipError_t e = hipMemcpy(regions_out, regions, (size_t)reg_words * (size_t)batch * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && seg_counts)
    e = hipMemcpy(seg_counts, reinterpret_cast<const char*>(d_prep) + sizeof(TimPrep) * (size_t)batch, 4 * (size_t)batch,
                  hipMemcpyDeviceToHost);
  return (int)e;
}

#ifdef TEASER_K1_LAB
// Lab build only (scripts/probe/k1_lab): the schedule / geometry of the kernel is picked per launch from
// TEASER_K1_VARIANT so that a probe can time them side by side.  Every variant produces the same bitmap
// (scripts/probe/k1_lab/k1_lab.py asserts it).  The product library has ONE instantiation and reads no environment.
struct K1Variant { int pipe, plain, chunks, occ4, uw3; };
static K1Variant k1_lab_variant() {
  const char* ev = getenv("TEASER_K1_VARIANT");
  const int v = ev ? atoi(ev) : 0;
  // v = 10000 * uw3 + 1000 * occ4 + 100 * chunks_log2 + 10 * plain + pipe   (occ4: the 128-VGPR build, four workgroups
  // per CU; uw3: the three-MFMA u / w formulation with its own operands and constants -- flat schedule, one chunk)
  K1Variant k;
  k.uw3 = (v / 10000) % 10 != 0;
  k.occ4 = (v / 1000) % 10 != 0;
  k.pipe = v % 10 != 0;
  k.plain = (v / 10) % 10 != 0;
  k.chunks = 1 << ((v / 100) % 10);
  return k;
}
#endif

// phase 0 pre-pass (bbox, centred fp16 operands, R^2, degrees zeroed), 1 the matrix-core kernel (bitmap
// + degrees), 2 FP64 fix-up of the worklist (+ overflow clear).  Three calls so that the profiling span
// of phase 1 is that kernel alone.  Phases 1 and 2 with kTimUpperOnly added: K1 stores the upper triangle only and the
// fix-up flips no transposed bit.  kTimMirror / kTimMirrorOpen: the lower triangle rebuilt from the upper one, for
// every problem / for the problems the degree closure left open (only d_desc, batch, max_n, d_bitmap, d_state are read).
// kTimNoStore on phases 1 and 2, kTimClosurePairs, kTimRebuild / kTimRebuildOpen: the route without stores (internal.h).  d_pk: total_tiles TimOperandTile2, total_tiles = sum of the problems' W;
// d_prep: tim_prep_bytes(batch), zero except the segment fields (tim_prep_fill_segments), part of the header upload;
// work_cap = tim_work_items(n, batch).
void launch_tim_graph_mfma(hipStream_t s, int phase, const ProbDesc* d_desc, int batch, int max_n,
                           int64_t total_tiles, const double* d_src, const double* d_dst,
                           void* d_pk, void* d_prep, void* d_work, int64_t work_cap,
                           uint64_t* d_bitmap, ProbState* d_state, int32_t* d_deg, double noise_bound,
                           double cbar2) {
  if (batch <= 0 || max_n <= 0) return;
  (void)total_tiles;
  const int T = (max_n + 63) / 64;
  if (phase == kTimMirror || phase == kTimMirrorOpen) {
    if (T < 2) return;
    const int waves = T * ((T + kMirrorRun - 1) / kMirrorRun);
    // (the waves stride over the runs: a grid sized for the work of ONE open problem would be ~800 workgroups per
    // problem that leave at once behind a batch the closure decided -- 30 us of dispatch at 64 x 10 k)
    hipLaunchKernelGGL(tim_mirror_lower_kernel, dim3((unsigned)std::min(64, (waves + 3) / 4), batch), dim3(256), 0, s, d_desc,
                       d_bitmap, d_state, phase == kTimMirrorOpen ? 1 : 0);
    return;
  }
  const double beta = 2 * noise_bound * sqrt(cbar2);  // registration.cc:438
  if (phase == kTimClosurePairs) {  // d_pk: the closure's scratch, d_prep: its counters (2 * batch ints, zero on entry)
    int32_t* counters = reinterpret_cast<int32_t*>(d_prep);
    launch_degree_closure_order(s, d_desc, batch, d_deg, d_state, d_pk, counters, d_src, d_dst);
    const ClosurePools cp = degree_closure_pools(d_pk, batch);
    hipLaunchKernelGGL(tim_closure_pairs_kernel, dim3(degree_closure_wgs(batch), batch), dim3(256), 0, s, cp.comp, cp.pts,
                       counters, beta);
    return;
  }
#ifdef TEASER_K1_LAB
  // the lab instantiations keep the full store, and the fix-up its flips of both copies with them: a rebuild then finds
  // every row in place
  const bool upper = false, nostore = false;
  if (phase == kTimRebuild || phase == kTimRebuildOpen) return;
#else
  const bool upper = (phase & kTimUpperOnly) != 0;
  const bool nostore = (phase & kTimNoStore) != 0;
#endif
  phase &= ~(kTimUpperOnly | kTimNoStore);
  TimPrep* prep = reinterpret_cast<TimPrep*>(d_prep);
  unsigned long long* work = reinterpret_cast<unsigned long long*>(d_work);
  unsigned int* work_count = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(d_prep) +
                                                            sizeof(TimPrep) * (size_t)batch);  // [batch]
  const int64_t reg_words = tim_region_words(max_n);  // per problem
  unsigned long long* regions = work + (work_cap - reg_words * (int64_t)batch);  // behind the counted segments
#ifdef TEASER_K1_LAB
  const K1Variant lab = k1_lab_variant();
#endif
  if (phase == 0) {
    // prep (and the worklist counter behind it) arrive zeroed: part of the solve's header upload
    hipLaunchKernelGGL(tim_prep_bbox_kernel, dim3((max_n + 1023) / 1024, batch), dim3(256), 0, s, d_desc,
                       d_src, d_dst, prep);
#ifdef TEASER_K1_LAB
    if (lab.uw3) {
      hipLaunchKernelGGL(tim_prep_pack3_kernel, dim3((T * 64 + 255) / 256, batch), dim3(256), 0, s, d_desc, d_src,
                         d_dst, prep, reinterpret_cast<TimOperandTile3*>(d_pk), d_deg, beta);
      hipLaunchKernelGGL(tim_prep_consts3_kernel, dim3((batch + 63) / 64), dim3(64), 0, s, prep, batch, beta);
      return;
    }
#endif
    hipLaunchKernelGGL(tim_prep_pack2_kernel, dim3((T * 64 + 255) / 256, batch), dim3(256), 0, s, d_desc, d_src,
                       d_dst, prep, reinterpret_cast<TimOperandTile2*>(d_pk), d_deg, beta);
    hipLaunchKernelGGL(tim_prep_consts_kernel, dim3((batch + 63) / 64), dim3(64), 0, s, prep, batch, beta);
  } else if (phase == 1) {
    const int gyr = (T + kMfmaRowTiles - 1) / kMfmaRowTiles;
#define TIM_K1_LAUNCH(PIPE, PLAIN, CHUNKS) TIM_K1_LAUNCH_OCC(PIPE, PLAIN, kK1Occ, CHUNKS, true)
#define TIM_K1_LAUNCH_OCC(PIPE, PLAIN, OCC, CHUNKS, ...)                                                                       \
  hipLaunchKernelGGL((tim_graph_mfma3_kernel<PIPE, PLAIN, OCC, CHUNKS, __VA_ARGS__>), dim3(tim_mfma_blocks(T, CHUNKS), batch), \
                     dim3(256), 0, s, d_desc, d_src, d_dst, (const void*)d_pk, prep, d_bitmap, beta, gyr, work, work_count,    \
                     d_state, d_deg, regions, T, 0, 0)
#ifdef TEASER_K1_LAB
#define TIM_K1_LAB_CASE(PIPE, PLAIN)                             \
  if (lab.pipe == (PIPE ? 1 : 0) && lab.plain == (PLAIN ? 1 : 0)) { \
    if (lab.chunks == 1) { TIM_K1_LAUNCH(PIPE, PLAIN, 1); }      \
    else if (lab.chunks == 2) { TIM_K1_LAUNCH(PIPE, PLAIN, 2); } \
    else { TIM_K1_LAUNCH(PIPE, PLAIN, 4); }                      \
  }
    if (lab.uw3) {
      if (lab.plain) { TIM_K1_LAUNCH_OCC(false, true, kK1Occ, 1, true, true); } else { TIM_K1_LAUNCH_OCC(false, false, kK1Occ, 1, true, true); }
    } else if (lab.occ4) {
      if (lab.plain) { TIM_K1_LAUNCH_OCC(false, true, 4, 1, true); } else { TIM_K1_LAUNCH_OCC(false, false, 4, 1, true); }
    } else {
      TIM_K1_LAB_CASE(false, false)
      TIM_K1_LAB_CASE(false, true)
      TIM_K1_LAB_CASE(true, false)
      TIM_K1_LAB_CASE(true, true)
    }
#undef TIM_K1_LAB_CASE
#else
    if (nostore) {
      TIM_K1_LAUNCH_OCC(kK1Pipe, kK1Plain, kK1Occ, kK1Chunks, false, false, kK1NoStore);
    } else if (upper) {
      TIM_K1_LAUNCH_OCC(kK1Pipe, kK1Plain, kK1Occ, kK1Chunks, false);
    } else {
      TIM_K1_LAUNCH(kK1Pipe, kK1Plain, kK1Chunks);
    }
#endif
#undef TIM_K1_LAUNCH
#undef TIM_K1_LAUNCH_OCC
#ifndef TEASER_K1_LAB
  } else if (phase == kTimRebuild || phase == kTimRebuildOpen) {
    // K1's full store once more (no worklist, the degrees into d_deg: a scratch array), then the recorded answers on
    // top.  Behind the closure most or all problems are skipped: the open-only launch is sized like the mirror launch
    // (a block walks its share of a problem's logical blocks), the launch for the getters has K1's own grid.
    const int gyr = (T + kMfmaRowTiles - 1) / kMfmaRowTiles, nlb = tim_mfma_blocks(T, kK1Chunks);
    const int open_only = phase == kTimRebuildOpen ? 1 : 0;
    // open-only: one problem's logical blocks x kRebuildOpenSlots slots, whatever the batch's size (the kernel finds
    // the open problems itself); the batch's size travels in rb_open
    const dim3 rb_grid = open_only ? dim3(nlb, kRebuildOpenSlots) : dim3(nlb, batch);
    // (two workgroups per CU: the pass loop keeps ~24 more registers live than one pass, and at three the kernel spills)
    hipLaunchKernelGGL((tim_graph_mfma3_kernel<kK1Pipe, kK1Plain, 2, kK1Chunks, true, false, kK1Rebuild>),
                       rb_grid, dim3(256), 0, s, d_desc, d_src, d_dst,
                       (const void*)d_pk, prep, d_bitmap, beta, gyr, work, work_count, d_state, d_deg, regions, T,
                       open_only ? batch : 0, nlb);
    hipLaunchKernelGGL(tim_fixup_replay_kernel, dim3((unsigned)std::max(4, ((T + 3) / 4 + 1) / 2), batch), dim3(256), 0, s,
                       d_desc, d_bitmap, work, work_count, d_state, regions, T, prep, open_only);
#endif
  } else {
    // a wave per PAIR of row tiles (p, T - 1 - p) of the largest problem, four pairs per workgroup; S_FIXUP_WGS forces
    // the workgroups per problem (the waves stride over the pairs).  The kernel also counts the degrees of the
    // problems that ran the FP64 body inside K1 (no degree atomics there)
    const int64_t forced_wgs = setting(S_FIXUP_WGS);
    const int64_t fix_wgs = forced_wgs > 0 ? forced_wgs : ((T + 1) / 2 + 3) / 4;
    const dim3 fix_grid((unsigned)std::max<int64_t>(4, fix_wgs), batch);
    if (nostore)
      hipLaunchKernelGGL(tim_fixup_group_kernel<true>, fix_grid, dim3(256), 0, s, d_desc, batch, d_src, d_dst, d_bitmap, beta,
                         work, work_count, d_state, d_deg, regions, T, prep, 0);
    else
      hipLaunchKernelGGL(tim_fixup_group_kernel<false>, fix_grid, dim3(256), 0, s, d_desc, batch, d_src, d_dst, d_bitmap, beta,
                         work, work_count, d_state, d_deg, regions, T, prep, upper ? kFixUpper : 0);
  }
}

// ------------------------------------------------------------------------------------------
// degrees: one wave per bitmap row
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void degree_kernel(const ProbDesc* __restrict__ descs,
                                                     const uint64_t* __restrict__ bitmap,
                                                     int32_t* __restrict__ deg) {
  const ProbDesc d = descs[blockIdx.y];
  const int lane = threadIdx.x & 63;
  for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < d.n; row += gridDim.x * 4) {
    const uint64_t* r = bitmap + d.bm_off + (int64_t)row * bm_stride(d.W);
    int c = 0;
    for (int w = lane; w < d.W; w += 64) c += __popcll(r[w]);
    c = wave_sum_i(c);
    if (lane == 0) deg[d.pt_off + row] = c;
  }
}

void launch_degrees(hipStream_t s, const ProbDesc* d_desc, int batch, int max_n,
                    const uint64_t* d_bitmap, int32_t* d_deg, ProbState* d_state) {
  if (batch <= 0 || max_n <= 0) return;
  dim3 grid((max_n + 3) / 4, batch);
  hipLaunchKernelGGL(degree_kernel, grid, dim3(256), 0, s, d_desc, d_bitmap, d_deg);
}

// ------------------------------------------------------------------------------------------
// estimate_scaling = true, first half of TLSScaleSolver::solveForScale (registration.cc:415-422):
// raw_scales[k] = |b_k| / |a_k|, alphas[k] = beta * (1/|a_k|) for every TIM k in the reference's
// pair order k = i*n - i(i+1)/2 + (j-i-1) (registration.cc:531).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trims_kernel(const double* __restrict__ src,
                                                    const double* __restrict__ dst, int n,
                                                    double beta, double* __restrict__ raw,
                                                    double* __restrict__ alpha) {
  const int i = blockIdx.x;
  if (i >= n - 1) return;
  const int64_t seg = (int64_t)i * n - (int64_t)i * (i + 1) / 2;
  const double six = src[3 * i], siy = src[3 * i + 1], siz = src[3 * i + 2];
  const double dix = dst[3 * i], diy = dst[3 * i + 1], diz = dst[3 * i + 2];
  for (int j = i + 1 + threadIdx.x; j < n; j += 256) {
    const double ax = src[3 * j] - six, ay = src[3 * j + 1] - siy, az = src[3 * j + 2] - siz;
    const double bx = dst[3 * j] - dix, by = dst[3 * j + 1] - diy, bz = dst[3 * j + 2] - diz;
    const double v1 = __builtin_sqrt((ax * ax + ay * ay) + az * az);
    const double v2 = __builtin_sqrt((bx * bx + by * by) + bz * bz);
    const int64_t k = seg + (j - i - 1);
    raw[k] = v2 / v1;
    alpha[k] = beta * (1.0 / v1);
  }
}

void launch_trims(hipStream_t s, const double* d_src, const double* d_dst, int n, double beta,
                  double* d_raw, double* d_alpha) {
  if (n < 2) return;
  hipLaunchKernelGGL(trims_kernel, dim3(n - 1), dim3(256), 0, s, d_src, d_dst, n, beta, d_raw,
                     d_alpha);
}

// inlier_selection_mode = NONE (registration.cc:648-654): every measurement is in the "clique"
__global__ void fill_identity_clique_kernel(const ProbDesc* __restrict__ descs,
                                            int32_t* __restrict__ clique,
                                            ProbState* __restrict__ states) {
  const ProbDesc d = descs[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < d.n) clique[d.pt_off + i] = i;
  if (i == 0) {
    ProbState* st = states + blockIdx.y;
    st->lb = d.n;
    st->clique_size = d.n;
    st->proven = 1;
    st->peel_done = 1;
  }
}

void launch_fill_identity_clique(hipStream_t s, const ProbDesc* d_desc, int batch, int max_n,
                                 int32_t* d_clique, ProbState* d_state) {
  if (batch <= 0) return;
  const int bx = max_n > 0 ? (max_n + 255) / 256 : 1;
  hipLaunchKernelGGL(fill_identity_clique_kernel, dim3(bx, batch), dim3(256), 0, s, d_desc,
                     d_clique, d_state);
}

}  // namespace thip
