// Scale, normalisation, band constants and admission test of the K1 matrix-core filter (kernels_graph.hip:
// "Operands and band constants of the u / w algebra").  Plain C++ with no device intrinsic, every function
// __host__ __device__ under hipcc: the device code and a host program (tests/test_k1_f16_consts_host.py) evaluate
// the SAME code.  consts_xy (below) is the kernel's; consts, the u / w formulation with w as a third MFMA, is what the
// lab build's UW3 variant runs and what tests/test_k1_f16_consts_host.py pins.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define K1_HD __host__ __device__ __forceinline__
#else
#define K1_HD inline
#endif

namespace k1c {

// Error budget of the two-piece fp16 operands, in units of u = 2^-24 times R^2 (R = max |normalised centred point|,
// both clouds; beta the normalised bound, kappa = 4 beta^2), term by term:
//   eps_u bounds |u~ - u*|, u = B - A - beta^2 over 32 K slots = two chained v_mfma_f32_32x32x16_f16:
//     16  f32 rounding of the normalised centred coordinates (8 per cloud)
//      3  f32 rounding of the two per-point constants (|.| <= 1.18 R^2 each); their three fp16 pieces are exact
//     32  split residuals: v = h + m + r, |r| <= 2^-22 |v| = 4u |v|; per cloud 2 sum_c (|v r'| + |r v'|) <= 16 u R^2
//     16  dropped m m' products: |m| <= 2^-11 |v|, per cloud 2 sum_c |m m'| <= 8 u R^2
//    420  accumulation: 2 x 16 products + 2 accumulator adds = 34 additions, each erring by at most one f32 ulp (2u)
//         of a magnitude <= sum |terms| <= 6 R^2 + beta^2 <= 6.18 R^2 (beta <= R / 2.4 is required)
//    487  -> kEpsU = 500, plus the ABSOLUTE term of fp16 subnormal rounding (a piece below 2^-14 is rounded to a
//         multiple of 2^-24: error <= 2^-25 = u / 2): the 12 products with an m piece, each against |2 h'| <= 2.002 R,
//         and one u / 2 per constant:  sub_u = u (12.1 R + 1).
//   eps_w bounds |w~ - w*|, w = -kappa A over the chain's first column operand (one MFMA), = kappa eps_A + sub_w:
//      8  coordinates, 2 f32 rounding of the norms, 8 their dropped third pieces (4u R^2 each), 16 split residuals,
//      8  dropped m m', 136 accumulation (17 additions x 2u x 4 R^2): 178 -> kEpsA = 200;
//      sub_w = u (6.1 R + kappa (3.1 R + 1)): the row pieces fp16(kappa h), fp16(kappa h), fp16(kappa m) per
//      coordinate (u / 2 each against |2 h'|, |2 m'|, |2 h'|), the column pieces 2 m' (u against kappa |h|), the low
//      pieces of the two norms (u / 2 against kappa each).
constexpr float kEpsU = 500.0f;
constexpr float kEpsA = 200.0f;
// The accumulation term assumes |D - exact| <= kMfmaUlps u sum|terms| per instruction (17 additions of one f32 ulp);
// scripts/probe/mfma_f16_error.hip measures the instruction's own figure (profiles/r7a/README.md).
constexpr float kMfmaUlps = 34.0f;
constexpr float kShortRatio = 21.76f;

K1_HD double pow2_d(int e) {  // 2^e, e clamped to the normal range of a double
  e = e < -1022 ? -1022 : (e > 1023 ? 1023 : e);
  return __builtin_bit_cast(double, (long long)(e + 1023) << 52);
}
K1_HD float f32_from_bits(unsigned int b) { return __builtin_bit_cast(float, b); }

// scale g in (1, sqrt 2] and kexp such that 4 (g beta)^2 = 2^kexp (the smallest power of two above 4 beta^2)
K1_HD void scale(double beta_d, double* g, int* kexp) {
  const double x = 4.0 * beta_d * beta_d;
  int e = 0;
  const bool ok = x > 1e-300 && x < 1e300;
  if (ok) e = (int)((__builtin_bit_cast(long long, x) >> 52) & 0x7ff) - 1023 + 1;  // floor(log2 x) + 1
  *kexp = e;
  *g = ok ? __builtin_sqrt(pow2_d(e) / x) : 1.0;
}

// Power-of-two normalisation of a problem: shift s with 16 <= H 2^s < 32 for H = the largest half extent of the two
// clouds' f32 bounding boxes (any axis).  Every normalised centred coordinate is then below 32 sqrt 2 = 45.3 and
// R^2 < 6200 (checked on the packed points themselves by the admission test, which does not rely on the box).
// Scaling a problem (coordinates and beta) by 2^k moves s by -k and leaves every packed bit as it was.
K1_HD int norm_shift(double H) {
  if (!(H > 1e-280 && H < 1e280)) return 0;
  const int e = (int)((__builtin_bit_cast(long long, H) >> 52) & 0x7ff) - 1023;  // floor(log2 H)
  return 4 - e;
}

struct Consts {
  float K2, K0, C;  // per-value band K2 |w| + K0 (admission only), constant band C (the kernel's)
  float eps_u, eps_w;
  int kexp;         // kappa = 2^kexp in the normalised system
  int use_mfma;
};

// Band constants in f32, every step rounded towards "wider" by a relative 2^-20 inflation.  s = norm_shift of the
// problem, r2_bits = float bits of the max squared norm of the NORMALISED centred f32 points (both clouds).
// Admission (use_mfma): everything the error analysis needs (eta <= 1/8, beta <= R / 2.4, finite input), and the
// fp16 range: R^2 <= 8192 (every coordinate <= 90.6, every norm and per-point constant <= 1.18 x 8192), kappa R <=
// 60000 (the kappa-shifted row slots of w), 2^-24 <= kappa <= 2^15 (kappa itself is a column slot), and the w
// error small against case (B) of the constant band's derivation.
K1_HD Consts consts(double beta_d, int s, unsigned int r2_bits) {
  Consts c;
  double g;
  int kexp0;
  scale(beta_d, &g, &kexp0);
  const int kexp = kexp0 + 2 * s;
  const double beta_n = beta_d * g * pow2_d(s);  // normalised beta
  const float u = 5.9604644775390625e-8f;        // 2^-24
  const float up = 1.000001f;
  const float r2 = f32_from_bits(r2_bits);
  const float beta = (float)beta_n * up;
  const float kappa = (float)pow2_d(kexp);  // 4 beta^2, exact
  const float R2 = r2 * up;
  const float R = __builtin_sqrtf(R2) * up;
  const float b2 = 0.25f * kappa;  // beta^2, exact
  const float eps_u = (kEpsU * u * R2 + u * (12.1f * R + 1.0f)) * up;
  const float eps_w = (kappa * (kEpsA * u * R2) + u * (6.1f * R + kappa * (3.1f * R + 1.0f))) * up;
  const float lam_lo = 2.0f * (float)beta_n * __builtin_sqrtf(r2) * 0.999999f;  // divisor
  const float lam_hi = 2.0f * beta * R * up;
  const float eta = eps_u / lam_lo * up;
  const bool range = (R2 <= 8192.0f) && (kexp >= -24) && (kexp <= 15) && (kappa * R * 1.001f <= 60000.0f);
  const bool ok = (R2 > 1e-30f) && range && (beta_d > 0) && (eta <= 0.125f) && (eta == eta) && (b2 * 5.76f <= R2) &&
                  (eps_w <= 0.004f * kappa * R2);
  const float den = 1.0f - 2.0f * (ok ? eta : 0.0f) - 2.0f * u;
  const float K2 = eta / den * up;
  // G: the gap between the reference's rounded double predicate and the exact one
  const float G = (1.3e-13f * beta * R2 * R + 8e-15f * b2 * R2) * up;
  const float K0p = (eps_u * lam_hi + eps_u * eps_u + eps_w * (1.0f + eta) + G) * up;
  const float K0 = (K0p / den + 2.0f * K2 * eps_w) * up;
  // short pairs (S <= beta): |d*| <= 4 beta^4, plus what the computed u~, w~ can add
  const float short_d = (4.0f * b2 * b2 * (1.0f + 16.0f * u) + 4.0f * b2 * eps_u + eps_u * eps_u + eps_w) * 1.001f * up;
  const float K0e = K0 * 1.001f * up;
  c.K2 = K2 * 1.001f * up;
  c.K0 = (K0e > short_d ? K0e : short_d) * 1.00001f;
  // constant band (kernels_graph.hip, "K1, the matrix-core filter"): cases (A) / (B)
  const float U0 = (4.0f * beta * R * 1.001f + 2.0f * eps_u) * up;
  const float E = (2.0f * U0 * eps_u + eps_u * eps_u + eps_w + G) * up;
  const float C0 = E / (1.0f - 4.0f * u) * 1.001f * up;
  c.C = (C0 > short_d ? C0 : short_d) * 1.00001f;
  c.eps_u = eps_u;
  c.eps_w = eps_w;
  c.kexp = kexp;
  // a band dominated by the short-pair term (beta close to the size of the cloud) would send most pairs to FP64:
  // beta <~ 0.11 R.  (The bound is on 4 beta^4 against (beta R)^2 R^2, not on the error: kShortRatio = 16 x 680 / 500
  // keeps the limit where it was with the wider eps_u of the bf16 operands.)
  c.use_mfma = (ok && c.K0 == c.K0 && c.K0 < 1e30f && short_d <= kShortRatio * K0e && c.C == c.C && c.C < 1e30f &&
                short_d <= kShortRatio * C0)
                   ? 1
                   : 0;
  return c;
}

// ------------------------------------------------------------------------------------------
// The X / Y formulation (the kernel's since the chain's first link doubles as w): every slot product carries the
// factor 1 / kappa = 2^-kexp, so that the two chained MFMAs leave
//   X = -A / kappa                         (first link,  K slots 0..15)
//   Y = X + (B - beta^2) / kappa = u / kappa   (second link, K slots 16..31)
// and Y^2 + X = (u^2 + w) / kappa^2: the sign of d, its magnitude scaled by an exact power of two.  Where the factor
// sits (exponent shifts of the values BEFORE they are split into fp16 pieces, exact for normal values):
//   coordinates         row side 2^-ra, column side 2^-rb:  ra = floor(kexp / 2), rb = kexp - ra
//   n_i, m_i, n_j, m_j  the three pieces carry 2^-pa, the entry opposite them is 2^-pb instead of 1:
//                       pa = max(kexp, -2), pb = kexp - pa = min(0, kexp + 2)
//   beta^2              -1/4 on the row side against 1
// fp16 range (R^2 <= 8192: |coordinate| <= 90.51, norms <= 8192):  90.51 x 2^-ra <= 46341 needs ra >= -9,
// 2 x 90.51 x 2^-rb <= 46341 needs rb >= -8, 8192 x 2^-pa <= 32768 always, 2^-pb <= 2^15 needs kexp >= -17: all hold
// for kexp >= -17.  Nothing overflows towards large kexp: the pieces only sink into the subnormal range, which the
// absolute terms below pay for.  (The kappa R <= 60000 condition of the w operand is gone with that operand.)
//
// Error budget, in units of u R^2 / kappa for the relative terms (they are those of consts() divided by kappa: an
// exponent shift changes no relative error), term by term:
//   eps_y bounds |Y~ - Y*|:
//     16  f32 rounding of the normalised centred coordinates (8 per cloud)
//      5  f32 rounding of the FOUR per-point constants n_i, n_j, m_i, m_j (|.| <= R^2 each: 4, rounded up); their
//         three fp16 pieces are exact
//     32  split residuals, 16 dropped m m' products: as above
//    557  accumulation: 34 additions x 2u x sum |terms|, sum |terms| <= 2 R^2 (2 s.s') + 2 R^2 (n_i + n_j) + 2 R^2
//         (2 d.d') + 2 R^2 (m_i + m_j) + beta^2 <= 8.18 R^2: the norms enter one by one, not as m - n
//    626  -> kEpsY = 640, plus the ABSOLUTE terms of fp16 subnormal rounding, u / 2 per value (its pieces together):
//         the 6 row coordinates against |2 v'| 2^-rb <= 2.002 R 2^-rb, the 6 column coordinates (2 v' 2^-rb: u / 2
//         as well) against |v| 2^-ra <= 1.001 R 2^-ra, the four constants against 2^-pb:
//         sub_y = u (R (6.1 x 2^-rb + 3.1 x 2^-ra) + 2 x 2^-pb)       (6.1, 3.1: room for the m m' of subnormal pieces)
//   eps_x bounds |X~ - X*|, one MFMA over the src cloud alone: 8 coordinates, 2 f32 rounding of the norms, 16 split
//     residuals, 8 dropped m m', 136 accumulation (17 additions x 2u x 4 R^2): 170 -> kEpsA = 200 as for w;
//     sub_x = sub_y / 2 (three row and three column coordinates, two constants).
// The band is the derivation of consts() (kernels_graph.hip, "K1, the matrix-core filter") with eps_u = kappa eps_y
// and eps_w = kappa^2 eps_x, and every constant it returns divided by the exact power of two that takes it to the
// units of Y and Y^2 + X:  C, K0 by kappa^2, eps_y = eps_u / kappa, eps_x = eps_w / kappa^2.  Short pairs: Y* in
// [-1/2, 0], X* in [-1/4, 0], |d*| / kappa^2 <= 1/4; self pairs: 1/16.
// Admission against consts(): eta <= 1/8 with the wider eps_y refuses R / beta above ~6500 (it was ~8300), and the
// short-pair limit moves with the band (beta <~ 0.11 R as before); kexp >= -17 instead of -24 is never the binding
// condition (eta <= 1/8 and R >= 16 already need kexp >= -15).
constexpr float kEpsY = 640.0f;

struct ConstsXY {
  float K2, K0, C;  // as in Consts, K0 and C in the units of Y^2 + X
  float eps_y, eps_x;
  int kexp;
  int use_mfma;
};

// the exponent shifts of the slot table (tim_prep_pack2_kernel and the tests' model read them here)
K1_HD void xy_shifts(int kexp, int* ra, int* rb, int* pa, int* pb) {
  *ra = kexp >> 1;  // floor
  *rb = kexp - *ra;
  *pa = kexp > -2 ? kexp : -2;
  *pb = kexp - *pa;
}

K1_HD ConstsXY consts_xy(double beta_d, int s, unsigned int r2_bits) {
  ConstsXY c;
  double g;
  int kexp0;
  scale(beta_d, &g, &kexp0);
  const int kexp = kexp0 + 2 * s;
  const double beta_n = beta_d * g * pow2_d(s);  // normalised beta
  const float u = 5.9604644775390625e-8f;        // 2^-24
  const float up = 1.000001f;
  const float r2 = f32_from_bits(r2_bits);
  const float beta = (float)beta_n * up;
  const float kappa = (float)pow2_d(kexp);  // 4 beta^2, exact
  const float R2 = r2 * up;
  const float R = __builtin_sqrtf(R2) * up;
  const float b2 = 0.25f * kappa;  // beta^2, exact
  const bool range = (R2 <= 8192.0f) && (kexp >= -17) && (kexp <= 15);
  int ra, rb, pa, pb;
  xy_shifts(range ? kexp : 0, &ra, &rb, &pa, &pb);
  const float fra = (float)pow2_d(-ra), frb = (float)pow2_d(-rb), fpb = (float)pow2_d(-pb);
  const float sub_y = u * (R * (6.1f * frb + 3.1f * fra) + 2.0f * fpb) * up;
  // in the kappa-multiplied units of consts(): eps_u = kappa eps_y, eps_w = kappa^2 eps_x
  const float eps_u = (kEpsY * u * R2 + kappa * sub_y) * up;
  const float eps_w = (kappa * (kEpsA * u * R2) + kappa * kappa * (0.5f * sub_y)) * up;
  const float lam_lo = 2.0f * (float)beta_n * __builtin_sqrtf(r2) * 0.999999f;  // divisor
  const float lam_hi = 2.0f * beta * R * up;
  const float eta = eps_u / lam_lo * up;
  const bool ok = (R2 > 1e-30f) && range && (beta_d > 0) && (eta <= 0.125f) && (eta == eta) && (b2 * 5.76f <= R2) &&
                  (eps_w <= 0.004f * kappa * R2);
  const float den = 1.0f - 2.0f * (ok ? eta : 0.0f) - 2.0f * u;
  const float K2 = eta / den * up;
  const float G = (1.3e-13f * beta * R2 * R + 8e-15f * b2 * R2) * up;
  const float K0p = (eps_u * lam_hi + eps_u * eps_u + eps_w * (1.0f + eta) + G) * up;
  const float K0 = (K0p / den + 2.0f * K2 * eps_w) * up;
  const float short_d = (4.0f * b2 * b2 * (1.0f + 16.0f * u) + 4.0f * b2 * eps_u + eps_u * eps_u + eps_w) * 1.001f * up;
  const float K0e = K0 * 1.001f * up;
  const float K0f = (K0e > short_d ? K0e : short_d) * 1.00001f;
  const float U0 = (4.0f * beta * R * 1.001f + 2.0f * eps_u) * up;
  const float E = (2.0f * U0 * eps_u + eps_u * eps_u + eps_w + G) * up;
  const float C0 = E / (1.0f - 4.0f * u) * 1.001f * up;
  const float C = (C0 > short_d ? C0 : short_d) * 1.00001f;
  // to the units of Y and Y^2 + X: exact (powers of two, far inside the f32 range for every admitted kexp)
  const float ik = (float)pow2_d(range ? -kexp : 0), ik2 = ik * ik;
  c.K2 = K2 * 1.001f * up;
  c.K0 = K0f * ik2;
  c.C = C * ik2;
  c.eps_y = eps_u * ik;
  c.eps_x = eps_w * ik2;
  c.kexp = kexp;
  c.use_mfma = (ok && K0f == K0f && K0f < 1e30f && short_d <= kShortRatio * K0e && C == C && C < 1e30f &&
                short_d <= kShortRatio * C0 && c.C > 0.0f && c.C < 1e30f)
                   ? 1
                   : 0;
  return c;
}

}  // namespace k1c
