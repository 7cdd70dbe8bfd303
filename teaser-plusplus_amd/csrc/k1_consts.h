// Scale, normalisation, band constants and admission test of the K1 matrix-core filter (kernels_graph.hip:
// "Operands and band constants of the u / w algebra").  Plain C++ with no device intrinsic, every function
// __host__ __device__ under hipcc: the device code and a host program (tests/test_k1_f16_consts_host.py) evaluate
// the SAME code.
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

}  // namespace k1c
