// posegraph_device.h -- what the pose-graph kernel (kernels_posegraph.hip), its host side (posegraph.hip) and the CPU
// emulation (tests/posegraph_emulation.cpp) share: the descriptor of one graph, the 3 x 4 pose arithmetic, the residual
// and the 6 x 6 system of one edge, and the scalar Levenberg-Marquardt controller.  The contract is written out in
// include/teaser_hip.h, "Pose-graph optimisation".  Everything here is __host__ __device__ and FP64; the translation
// units that include it are compiled with -ffp-contract=off, so the kernel and the emulation run the same roundings
// apart from sin, cos and atan2's library.  The residual calls fma() explicitly (pg_dd_fma): this rests on fma being
// correctly rounded on both sides, which v_fma_f64 and the host's libm are.
#pragma once

#include <math.h>
#include <stdint.h>

#include "teaser_hip.h"

namespace thip {

constexpr int kPgBlock = 256;  // threads of the workgroup that owns a graph
constexpr int kPgTile = 16;    // columns of one panel of the blocked Cholesky factorisation
constexpr int kPgMaxN = 6 * (TEASER_HIP_POSEGRAPH_MAX_NODES - 1);  // free unknowns at most (762)
constexpr double kPgTau = 1e-5;  // lam of a pass's first trial over the largest diagonal entry of H

enum { PG_MODE_OPTIMIZE = 0, PG_MODE_LINEARIZE = 1 };

// One graph of a call.  Offsets count elements of the concatenated arrays: nodes (node_off), edges (edge_off), rows
// of the node CSR (nodeptr_off = node_off + b), its entries (inc_off = 2 edge_off), node pairs (pair_off), rows of
// the pair list (pairptr_off = pair_off + b), doubles of the dense scratch (h_off), free unknowns (g_off).
struct PgDesc {
  int32_t n, m, ref, N;  // N = 6 (n - 1); ref already resolved (reference_node < 0 -> 0)
  int32_t n_pairs, trace_cap, trivial, pad;
  int64_t node_off, edge_off, nodeptr_off, inc_off, pair_off, pairptr_off, h_off, g_off, trace_off;
  teaser_posegraph_option_c opt;
};

// The device arrays of a call (one struct, passed by value to the kernel).
struct PgArgs {
  const PgDesc* desc;
  const double* poses_in;  // 16 per node
  const int32_t* src;
  const int32_t* tgt;
  const double* X;  // 16 per edge
  const double* L;  // 36 per edge
  const uint8_t* unc;
  const int32_t* node_ptr;   // CSR rows: incident edges of a node, ascending
  const int32_t* inc_edge;
  const int32_t* pair_u;     // distinct node pairs u < v, sorted
  const int32_t* pair_v;
  const int32_t* pair_ptr;
  const int32_t* pair_edge;  // their edges, ascending
  double* pose_cur;   // 12 per node
  double* pose_cand;  // 12 per node
  double* e;          // 6 per edge
  double* r;
  double* l;
  double* A;          // 36 per edge, symmetric
  double* bv;         // 6 per edge
  double* conf;
  uint8_t* pruned;
  double* H;  // N x N per graph at h_off
  double* M;  // N x N per graph at h_off: H + lam I, factorised in place
  double* g;  // N per graph at g_off
  double* poses_out;  // 16 per node
  teaser_posegraph_result_c* res;
  teaser_posegraph_trace_c* trace;
  int32_t mode;
};

void launch_posegraph(hipStream_t s, int batch, const PgArgs& args);

#define PG_HD __host__ __device__ inline

// ---- poses: the upper three rows of a 4 x 4, row-major (12 doubles); the last row is 0 0 0 1 ----

// C = A B as 4 x 4 matrices with last rows 0 0 0 1, sums in ascending k
PG_HD void pg_mul(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) C[4 * i + j] = (A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j];
    C[4 * i + 3] = ((A[4 * i] * B[3] + A[4 * i + 1] * B[7]) + A[4 * i + 2] * B[11]) + A[4 * i + 3];
  }
}

// V(xi): R = Rz(c) Ry(b) Rx(a), translation (tx, ty, tz)
PG_HD void pg_V(const double* xi, double* M) {
  const double ca = cos(xi[0]), sa = sin(xi[0]), cb = cos(xi[1]), sb = sin(xi[1]), cg = cos(xi[2]), sg = sin(xi[2]);
  M[0] = cg * cb;
  M[1] = cg * sb * sa - sg * ca;
  M[2] = cg * sb * ca + sg * sa;
  M[4] = sg * cb;
  M[5] = sg * sb * sa + cg * ca;
  M[6] = sg * sb * ca - cg * sa;
  M[8] = -sb;
  M[9] = cb * sa;
  M[10] = cb * ca;
  M[3] = xi[3];
  M[7] = xi[4];
  M[11] = xi[5];
}

// v6(M): the inverse of V
PG_HD void pg_v6(const double* M, double* out) {
  const double sy = sqrt(M[0] * M[0] + M[4] * M[4]);
  if (sy > 1e-6) {
    out[0] = atan2(M[9], M[10]);
    out[1] = atan2(-M[8], sy);
    out[2] = atan2(M[4], M[0]);
  } else {
    out[0] = atan2(-M[6], M[5]);
    out[1] = atan2(-M[8], sy);
    out[2] = 0.0;
  }
  out[3] = M[3];
  out[4] = M[7];
  out[5] = M[11];
}

// The information matrix taken symmetric from its upper triangle
PG_HD double pg_sym(const double* L, int i, int j) { return i <= j ? L[6 * i + j] : L[6 * j + i]; }

// ---- double-double helpers for the residual: E = X^-1 Tt^-1 Ts is a rotation by a few micro-radians near convergence,
// and its off-diagonal entries (the residual) are what is left of sums of products of size one.  Rounded after every
// operation they carry an absolute error of 1e-16, which is 1e-10 of the residual; the products and sums below are
// error-free transformations (fma for the product's error, Knuth's two-sum), so that E is rounded once. ----
struct PgDD {
  double hi, lo;
};

// s += a * b with a given as a double-double
PG_HD void pg_dd_fma(PgDD& s, PgDD a, double b) {
  const double p = a.hi * b;
  const double pe = fma(a.hi, b, -p);
  const double t = s.hi + p;
  const double bb = t - s.hi;
  const double te = (s.hi - (t - bb)) + (p - bb);
  s.hi = t;
  s.lo += (te + pe) + a.lo * b;
}

PG_HD PgDD pg_dd_norm(PgDD s) {
  const double t = s.hi + s.lo;
  return PgDD{t, s.lo - (t - s.hi)};
}

// inverse(T) with the translation -(R^T t) as a double-double (the rotation block is a transpose: exact)
PG_HD void pg_inverse_dd(const double* T, PgDD* O) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) O[4 * r + c] = PgDD{T[4 * c + r], 0.0};
    PgDD s{0.0, 0.0};
    for (int k = 0; k < 3; ++k) pg_dd_fma(s, PgDD{-T[4 * k + r], 0.0}, T[4 * k + 3]);
    O[4 * r + 3] = pg_dd_norm(s);
  }
}

// The residual of one edge at poses Ts, Tt: B = X^-1 Tt^-1 (kept for the Jacobian), e = v6(B Ts), r = e^T L e,
// l = 1 or (mu / (mu + r))^2, and the edge's term of F: l r, plus mu (sqrt(l) - 1)^2 on an uncertain edge.
// Only E is compensated.  The B handed on is the double-double product rounded to double, and pg_edge_system takes the
// Jacobian from it in plain FP64: J multiplies a residual that is already small, so its rounding is not amplified.
PG_HD void pg_edge_residual(const double* Ts, const double* Tt, const double* X, const double* L, int uncertain,
                            double mu, double* B, double* e, double* r, double* l, double* f) {
  PgDD Xi[12], Ti[12], Bd[12];
  double E[12];
  pg_inverse_dd(X, Xi);
  pg_inverse_dd(Tt, Ti);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      PgDD s = j == 3 ? Xi[4 * i + 3] : PgDD{0.0, 0.0};
      for (int k = 0; k < 3; ++k) {  // Xi's rotation entries are plain doubles; Ti's translation is a double-double
        pg_dd_fma(s, Ti[4 * k + j], Xi[4 * i + k].hi);
      }
      Bd[4 * i + j] = pg_dd_norm(s);
      B[4 * i + j] = Bd[4 * i + j].hi;
    }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      PgDD s = j == 3 ? Bd[4 * i + 3] : PgDD{0.0, 0.0};
      for (int k = 0; k < 3; ++k) pg_dd_fma(s, Bd[4 * i + k], Ts[4 * k + j]);
      E[4 * i + j] = s.hi + s.lo;
    }
  pg_v6(E, e);
  double rr = 0.0;
  for (int j = 0; j < 6; ++j) {
    double v = 0.0;
    for (int i = 0; i < 6; ++i) v += e[i] * pg_sym(L, i, j);
    rr += v * e[j];
  }
  *r = rr;
  if (uncertain) {
    const double q = mu / (mu + rr);
    const double ll = q * q;
    const double s = sqrt(ll) - 1.0;
    *l = ll;
    *f = ll * rr + mu * (s * s);
  } else {
    *l = 1.0;
    *f = rr;
  }
}

// The system of one edge: J_s from the six generators (J[i][c] = lin6(B D_c Ts)[i]), A = l (J^T L) J with the lower
// triangle mirrored from the upper so that A is symmetric bit for bit, b = l J^T (L e).
PG_HD void pg_edge_system(const double* B, const double* Ts, const double* L, const double* e, double l, double* A,
                          double* b) {
  double J[36];
  for (int c = 0; c < 6; ++c) {
    // B D_c: the generator D_c has at most two entries
    double G[12];
    for (int k = 0; k < 12; ++k) G[k] = 0.0;
    for (int i = 0; i < 3; ++i) {
      if (c == 0) {
        G[4 * i + 1] = B[4 * i + 2];
        G[4 * i + 2] = -B[4 * i + 1];
      } else if (c == 1) {
        G[4 * i + 2] = B[4 * i];
        G[4 * i] = -B[4 * i + 2];
      } else if (c == 2) {
        G[4 * i] = B[4 * i + 1];
        G[4 * i + 1] = -B[4 * i];
      } else {
        G[4 * i + 3] = B[4 * i + (c - 3)];
      }
    }
    // (B D_c) Ts: the last row of B D_c is zero, so the product's last column has no "+ 1" term
    double P[12];
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) P[4 * i + j] = (G[4 * i] * Ts[j] + G[4 * i + 1] * Ts[4 + j]) + G[4 * i + 2] * Ts[8 + j];
      P[4 * i + 3] = ((G[4 * i] * Ts[3] + G[4 * i + 1] * Ts[7]) + G[4 * i + 2] * Ts[11]) + G[4 * i + 3];
    }
    J[c] = (P[9] - P[6]) / 2;
    J[6 + c] = (P[2] - P[8]) / 2;
    J[12 + c] = (P[4] - P[1]) / 2;
    J[18 + c] = P[3];
    J[24 + c] = P[7];
    J[30 + c] = P[11];
  }
  double Q[36];  // J^T L
  for (int a = 0; a < 6; ++a)
    for (int j = 0; j < 6; ++j) {
      double v = 0.0;
      for (int i = 0; i < 6; ++i) v += J[6 * i + a] * pg_sym(L, i, j);
      Q[6 * a + j] = v;
    }
  for (int a = 0; a < 6; ++a)
    for (int c = a; c < 6; ++c) {
      double v = 0.0;
      for (int j = 0; j < 6; ++j) v += Q[6 * a + j] * J[6 * j + c];
      v = l * v;
      A[6 * a + c] = v;
      A[6 * c + a] = v;
    }
  double w[6];  // L e
  for (int i = 0; i < 6; ++i) {
    double v = 0.0;
    for (int j = 0; j < 6; ++j) v += pg_sym(L, i, j) * e[j];
    w[i] = v;
  }
  for (int a = 0; a < 6; ++a) {
    double v = 0.0;
    for (int i = 0; i < 6; ++i) v += J[6 * i + a] * w[i];
    b[a] = l * v;
  }
}

// ---- the controller: the stop tests and the lam / nu / it / lm updates of one pass, in the restatement's sequence.
// One function, called with the event that has just happened; it answers PG_GO or the status the pass stops with. ----
struct PgCtl {
  double lam, nu;
  int32_t it, lm;
};
enum { PG_GO = -1 };
enum PgEvent {
  PG_EV_START,      // a = max diag H, b = |g|inf of the pass's first linearisation
  PG_EV_SOLVED,     // the factorisation succeeded: a = |d|2, b = |x|2
  PG_EV_GAIN,       // rho > 0: a = F - F', b = F (the relative-residual test; the step is not taken when it fires)
  PG_EV_ACCEPTED,   // the step was taken and relinearised: a = |g|inf, b = F; c = rho
  PG_EV_REJECTED    // rho is not > 0 (a NaN included) or the factorisation failed
};

PG_HD int pg_control(PgCtl& s, PgEvent ev, double a, double b, double c, const teaser_posegraph_option_c& o) {
  switch (ev) {
    case PG_EV_START:
      s.lam = kPgTau * a;
      s.nu = 2.0;
      s.it = 0;
      s.lm = 0;
      return b <= o.min_right_term ? TEASER_HIP_PG_RIGHT_TERM : PG_GO;
    case PG_EV_SOLVED:
      return a <= o.min_relative_increment * (b + o.min_relative_increment) ? TEASER_HIP_PG_INCREMENT : PG_GO;
    case PG_EV_GAIN:
      return a < o.min_relative_residual_increment * b ? TEASER_HIP_PG_REL_RESIDUAL : PG_GO;
    case PG_EV_ACCEPTED: {
      const double t = 2 * c - 1;
      const double alpha = 1 - t * t * t;
      const double lo = o.lower_scale_factor;
      const double hi = o.upper_scale_factor < alpha ? o.upper_scale_factor : alpha;  // min(upper, alpha)
      s.lam = s.lam * (lo > hi ? lo : hi);                                            // max(lower, .)
      s.nu = 2.0;
      if (a <= o.min_right_term) return TEASER_HIP_PG_RIGHT_TERM;
      s.it += 1;
      s.lm = 0;
      if (b < o.min_residual) return TEASER_HIP_PG_RESIDUAL;
      if (s.it >= o.max_iteration) return TEASER_HIP_PG_MAX_ITERATION;
      return PG_GO;
    }
    case PG_EV_REJECTED:
      s.lam = s.lam * s.nu;
      s.nu = s.nu * 2;
      s.lm += 1;
      return s.lm >= o.max_iteration_lm ? TEASER_HIP_PG_MAX_ITERATION_LM : PG_GO;
  }
  return PG_GO;
}

// The trials one pass can run at most: every trial either accepts (it grows, at most max_iteration times) or rejects
// (lm grows, at most max_iteration_lm times between two acceptances).  The loop counts down from this as well.
PG_HD int64_t pg_trial_bound(const teaser_posegraph_option_c& o) {
  return ((int64_t)o.max_iteration + 1) * ((int64_t)o.max_iteration_lm + 1) + 1;
}

// The free unknown block of node i (the reference node's six unknowns are left out); i != ref
PG_HD int pg_free(int i, int ref) { return i < ref ? i : i - 1; }

}  // namespace thip
