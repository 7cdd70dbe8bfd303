// Characterises the accumulation error of v_mfma_f32_32x32x16_f16 against exact arithmetic, alone and in a chain of two
// (the K1 filter's u chain): max |D - exact| / (u * (sum |a_k b_k| + |C|)), u = 2^-24, over random fp16 operands with
// widely varying magnitudes and signs -- and over operands in the fp16 SUBNORMAL range (exponent field 0): a matrix
// pipe that flushed them would lose those terms entirely, i.e. err ~ sum |terms| = 1.7e7 u.  Calibrates kMfmaUlps
// in csrc/k1_consts.h (the budget assumes 34 u per instruction, 68 u for the chain of two).
// build: hipcc --offload-arch=gfx950 -O2 -o mfma_f16_error mfma_f16_error.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__global__ void k(const uint16_t* A, const uint16_t* B, const float* C, float* D, int chain) {
  // A: [chain][32 rows][16 k] fp16 bits, B: [chain][16 k][32 cols], C/D: [32][32]
  const int lane = threadIdx.x, h = lane >> 5, c = lane & 31;
  f32x16 acc;
  for (int q = 0; q < 16; ++q) acc[q] = C[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + c];
  for (int r = 0; r < chain; ++r) {
    f16x8 a, b;
    for (int kk = 0; kk < 8; ++kk) {
      a[kk] = __builtin_bit_cast(_Float16, A[r * 512 + c * 16 + 8 * h + kk]);
      b[kk] = __builtin_bit_cast(_Float16, B[r * 512 + (8 * h + kk) * 32 + c]);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
  }
  for (int q = 0; q < 16; ++q) D[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + c] = acc[q];
}
static double hf(uint16_t v) {  // exact value of fp16 bits (normal and subnormal)
  const int e = (v >> 10) & 31, m = v & 1023;
  const double mag = e ? ldexp(1.0 + m / 1024.0, e - 15) : ldexp(m / 1024.0, -14);
  return (v & 0x8000) ? -mag : mag;
}
static uint64_t s = 88172645463325252ull;
static uint32_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); }
int main() {
  std::vector<uint16_t> A(1024), B(1024);
  std::vector<float> C(1024), D(1024);
  uint16_t *dA, *dB; float *dC, *dD;
  if (hipMalloc(&dA, 2048) != hipSuccess || hipMalloc(&dB, 2048) != hipSuccess || hipMalloc(&dC, 4096) != hipSuccess ||
      hipMalloc(&dD, 4096) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
  const double u = ldexp(1.0, -24);
  // mode bits: 1 = wide exponent spread, 2 = random C, 4 = A in the subnormal range (B large), 8 = both sides' low
  // halves subnormal (k >= 8)
  for (int chain = 1; chain <= 2; ++chain)
    for (int mode = 0; mode < 16; ++mode) {
      if ((mode & 4) && (mode & 8)) continue;
      double worst = 0, worst_rel_exact = 0;
      for (int trial = 0; trial < 200; ++trial) {
        const int spread = (mode & 1) ? 12 : 2;       // exponent spread of the operands
        const bool withc = (mode & 2) != 0;
        for (size_t i = 0; i < A.size(); ++i) {
          int ea = 15 - (int)(rnd() % spread), eb = 15 - (int)(rnd() % spread);
          if (mode & 4) { ea = 0; eb = 20 + (int)(rnd() % 4); }
          if ((mode & 8) && ((i & 15) >= 8)) ea = 0;                  // A[.][row][k]: k = i & 15
          if ((mode & 8) && (((i & 511) >> 5) >= 8)) eb = 0;          // B[.][k][col]: k = (i & 511) >> 5
          A[i] = (uint16_t)(((rnd() & 1) << 15) | (ea << 10) | (rnd() & 1023));
          B[i] = (uint16_t)(((rnd() & 1) << 15) | (eb << 10) | (rnd() & 1023));
        }
        for (auto& v : C) v = withc ? (float)((int)(rnd() % 2000001) - 1000000) * ((mode & 12) ? 1e-9f : 1e-5f) : 0.f;
        hipMemcpy(dA, A.data(), 2048, hipMemcpyHostToDevice); hipMemcpy(dB, B.data(), 2048, hipMemcpyHostToDevice);
        hipMemcpy(dC, C.data(), 4096, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, dA, dB, dC, dD, chain);
        if (hipMemcpy(D.data(), dD, 4096, hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel failed\n"); return 1; }
        for (int i = 0; i < 32; ++i) for (int j = 0; j < 32; ++j) {
          long double ex = C[i * 32 + j], mag = fabsl((long double)C[i * 32 + j]);
          for (int r = 0; r < chain; ++r)
            for (int kk = 0; kk < 16; ++kk) {
              long double p = (long double)hf(A[r * 512 + i * 16 + kk]) * hf(B[r * 512 + kk * 32 + j]);
              ex += p; mag += fabsl(p);
            }
          const double err = fabs((double)((long double)D[i * 32 + j] - ex));
          if (mag > 0) worst = fmax(worst, err / (u * (double)mag));
          if (fabsl(ex) > 0) worst_rel_exact = fmax(worst_rel_exact, err / (u * fabs((double)ex)));
        }
      }
      printf("chain %d mode %2d (exp spread %2d, C %s, %s): max err = %.3f u*sum|terms|   (%.3f u*|exact|)   assumed %d\n", chain,
             mode, (mode & 1) ? 12 : 2, (mode & 2) ? "random" : "0",
             (mode & 4) ? "A subnormal" : (mode & 8) ? "k >= 8 subnormal on both sides" : "normal operands", worst, worst_rel_exact, 34 * chain);
    }
  return 0;
}
