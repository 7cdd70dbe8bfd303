// kernels_posegraph.hip -- pose-graph optimisation (Open3D's global_optimization with
// GlobalOptimizationLevenbergMarquardt; the contract is written out in include/teaser_hip.h, "Pose-graph
// optimisation") for gfx950.
//
// ONE workgroup of kPgBlock threads owns a graph and runs both passes of the Levenberg-Marquardt loop to the end: the
// grid is `batch` workgroups, there is no communication between workgroups (no grid sync, no flag), and every loop is
// bounded by a counter, so a launch cannot hang on scheduling.  The scalar decisions are taken by pg_control
// (posegraph_device.h) from values every thread of the workgroup reads from LDS, so they are workgroup-uniform and
// every __syncthreads is reached by all threads.
//
// Phases of a trial, each ended by a workgroup barrier (__syncthreads orders the workgroup's global-memory writes too):
//   linearise   a thread per edge: residual, weight, J_s, A = l J^T L J, b = l J^T L e          -> global work arrays
//   assemble    a thread per ENTRY of a diagonal block (CSR of incident edges), of an off-diagonal block (sorted list
//               of distinct node pairs) and of g; each adds its edges in ascending edge index.  No atomics.
//   factorise   M = H + lam I in the graph's slice of the dense scratch; blocked right-looking Cholesky, kPgTile
//               columns per panel: diagonal tile in LDS (one thread, tile^3 / 6 operations), panel rows one per
//               thread, trailing update one lower-triangle entry per thread with the panel's kPgTile products
//               subtracted in ascending column.  A pivot that is not finite or not positive ends the trial as rejected.
//   solve       forward and backward substitution on g / y / d in LDS, one column (row) per step
//   candidate   a thread per node: T' = V(d_i) T_i; then the residuals of all edges at T' and F'
// Sums over edges or unknowns (F, |d|2, d^T(lam d - g)) are taken per thread over its strided elements in ascending
// order and then over the threads in the fixed order of pg_block_sum; |x|2 and mu are summed by one thread in
// ascending index.  Nothing depends on the batch or on the graph's position in it.
#include <hip/hip_runtime.h>

#include "posegraph_device.h"

namespace thip {

namespace {

struct PgShared {
  double g[kPgMaxN + 6];
  double d[kPgMaxN + 6];
  double y[kPgMaxN + 6];
  double red[kPgBlock];
  double tile[kPgTile * kPgTile];
  double scalar;
  PgCtl ctl;  // the controller's state: every thread runs pg_control on these values, thread 0 stores the result
  int32_t flag;
};

// v over the workgroup in a fixed order, the same value in every thread
__device__ __forceinline__ double pg_block_sum(double v, PgShared& S) {
  __syncthreads();
  S.red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kPgBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) S.red[threadIdx.x] += S.red[threadIdx.x + o];
    __syncthreads();
  }
  return S.red[0];
}

// max over the workgroup, a NaN winning (as numpy's max): the result does not depend on the order
__device__ __forceinline__ double pg_nanmax(double x, double y) { return (x != x || y != y) ? NAN : fmax(x, y); }

__device__ __forceinline__ double pg_block_max(double v, PgShared& S) {
  __syncthreads();
  S.red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kPgBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) S.red[threadIdx.x] = pg_nanmax(S.red[threadIdx.x], S.red[threadIdx.x + o]);
    __syncthreads();
  }
  return S.red[0];
}

// mu of a pass: over the uncertain edges that are not pruned, summed by one thread in ascending edge index
__device__ double pg_mu(const PgArgs& a, const PgDesc& D, PgShared& S) {
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.0;
    int cnt = 0;
    for (int k = 0; k < D.m; ++k)
      if (a.unc[D.edge_off + k] && !a.pruned[D.edge_off + k]) {
        sum += a.L[36 * (D.edge_off + k) + 35];
        ++cnt;
      }
    const double mcd = D.opt.max_correspondence_distance;
    S.scalar = cnt ? D.opt.preference_loop_closure * mcd * mcd * (sum / (double)cnt) : 0.0;
  }
  __syncthreads();
  return S.scalar;
}

// The residuals of every live edge at `poses` and F; store: also e, r, l, A and b (the linearisation).
__device__ double pg_eval(const PgArgs& a, const PgDesc& D, const double* poses, double mu, bool store, PgShared& S) {
  double part = 0.0;
  for (int k = threadIdx.x; k < D.m; k += kPgBlock) {
    const int64_t K = D.edge_off + k;
    if (a.pruned[K]) continue;
    const double* Ts = poses + 12 * (D.node_off + a.src[K]);
    const double* Tt = poses + 12 * (D.node_off + a.tgt[K]);
    double X[12], L[36], B[12], e[6], r, l, f;
    for (int i = 0; i < 12; ++i) X[i] = a.X[16 * K + i];
    for (int i = 0; i < 36; ++i) L[i] = a.L[36 * K + i];
    double ts[12], tt[12];
    for (int i = 0; i < 12; ++i) {
      ts[i] = Ts[i];
      tt[i] = Tt[i];
    }
    pg_edge_residual(ts, tt, X, L, a.unc[K], mu, B, e, &r, &l, &f);
    part += f;
    if (store) {
      double A[36], b[6];
      pg_edge_system(B, ts, L, e, l, A, b);
      for (int i = 0; i < 6; ++i) a.e[6 * K + i] = e[i];
      a.r[K] = r;
      a.l[K] = l;
      for (int i = 0; i < 36; ++i) a.A[36 * K + i] = A[i];
      for (int i = 0; i < 6; ++i) a.bv[6 * K + i] = b[i];
    }
  }
  return pg_block_sum(part, S);
}

// H (free unknowns, N x N) and g from the edges' A and b.  Entries of blocks no edge touches stay zero from the
// start of the kernel.  Returns max diag H in *maxdiag and |g|inf in *gmax.
__device__ void pg_assemble(const PgArgs& a, const PgDesc& D, PgShared& S, double* maxdiag, double* gmax) {
  const int N = D.N;
  double* H = a.H + D.h_off;
  const int32_t* nptr = a.node_ptr + D.nodeptr_off;
  const int32_t* inc = a.inc_edge + D.inc_off;
  __syncthreads();
  for (int idx = threadIdx.x; idx < D.n * 36; idx += kPgBlock) {
    const int node = idx / 36, ent = idx % 36;
    if (node == D.ref) continue;
    double sum = 0.0;
    for (int q = nptr[node]; q < nptr[node + 1]; ++q) {
      const int64_t K = D.edge_off + inc[q];
      if (!a.pruned[K]) sum += a.A[36 * K + ent];
    }
    const int f = 6 * pg_free(node, D.ref);
    H[(int64_t)(f + ent / 6) * N + f + ent % 6] = sum;
  }
  const int32_t* pptr = a.pair_ptr + D.pairptr_off;
  for (int idx = threadIdx.x; idx < D.n_pairs * 36; idx += kPgBlock) {
    const int p = idx / 36, ent = idx % 36;
    const int u = a.pair_u[D.pair_off + p], v = a.pair_v[D.pair_off + p];
    if (u == D.ref || v == D.ref) continue;
    double sum = 0.0;
    for (int q = pptr[p]; q < pptr[p + 1]; ++q) {
      const int64_t K = D.edge_off + a.pair_edge[D.edge_off + q];
      if (!a.pruned[K]) sum -= a.A[36 * K + ent];  // A is symmetric: the edge's direction does not matter
    }
    const int fu = 6 * pg_free(u, D.ref), fv = 6 * pg_free(v, D.ref);
    H[(int64_t)(fu + ent / 6) * N + fv + ent % 6] = sum;
    H[(int64_t)(fv + ent % 6) * N + fu + ent / 6] = sum;
  }
  for (int idx = threadIdx.x; idx < D.n * 6; idx += kPgBlock) {
    const int node = idx / 6, c = idx % 6;
    if (node == D.ref) continue;
    double sum = 0.0;
    for (int q = nptr[node]; q < nptr[node + 1]; ++q) {
      const int64_t K = D.edge_off + inc[q];
      if (a.pruned[K]) continue;
      if (a.src[K] == node)
        sum += a.bv[6 * K + c];
      else
        sum -= a.bv[6 * K + c];
    }
    S.g[6 * pg_free(node, D.ref) + c] = sum;
  }
  __syncthreads();
  double md = -INFINITY, gm = 0.0;
  for (int i = threadIdx.x; i < N; i += kPgBlock) {
    md = pg_nanmax(md, H[(int64_t)i * N + i]);
    gm = pg_nanmax(gm, fabs(S.g[i]));
  }
  *maxdiag = pg_block_max(md, S);
  *gmax = pg_block_max(gm, S);
}

// M = H + lam I (lower triangle), factorised in place: M = L L^T.  false when a pivot is not finite or not positive.
__device__ bool pg_cholesky(const PgArgs& a, const PgDesc& D, double lam, PgShared& S) {
  const int N = D.N;
  const double* H = a.H + D.h_off;
  double* M = a.M + D.h_off;
  __syncthreads();
  for (int64_t idx = threadIdx.x; idx < (int64_t)N * N; idx += kPgBlock) {
    const int i = (int)(idx / N), j = (int)(idx % N);
    if (j <= i) M[idx] = i == j ? H[idx] + lam : H[idx];
  }
  if (threadIdx.x == 0) S.flag = 1;
  __syncthreads();
  for (int kb = 0; kb < N; kb += kPgTile) {
    const int tb = N - kb < kPgTile ? N - kb : kPgTile;
    // the diagonal tile
    for (int idx = threadIdx.x; idx < tb * tb; idx += kPgBlock) {
      const int i = idx / tb, j = idx % tb;
      if (j <= i) S.tile[i * kPgTile + j] = M[(int64_t)(kb + i) * N + kb + j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int j = 0; j < tb; ++j) {
        double dv = S.tile[j * kPgTile + j];
        for (int p = 0; p < j; ++p) dv -= S.tile[j * kPgTile + p] * S.tile[j * kPgTile + p];
        if (!isfinite(dv) || !(dv > 0)) {
          S.flag = 0;
          break;
        }
        const double piv = sqrt(dv);
        S.tile[j * kPgTile + j] = piv;
        for (int i = j + 1; i < tb; ++i) {
          double v = S.tile[i * kPgTile + j];
          for (int p = 0; p < j; ++p) v -= S.tile[i * kPgTile + p] * S.tile[j * kPgTile + p];
          S.tile[i * kPgTile + j] = v / piv;
        }
      }
    }
    __syncthreads();
    if (!S.flag) return false;  // uniform: every thread reads the same LDS word after the barrier
    for (int idx = threadIdx.x; idx < tb * tb; idx += kPgBlock) {
      const int i = idx / tb, j = idx % tb;
      if (j <= i) M[(int64_t)(kb + i) * N + kb + j] = S.tile[i * kPgTile + j];
    }
    // the panel below it: a row per thread, L_row = A_row L_tile^-T.  A tile narrower than kPgTile is the last one
    // and has no rows below it (rem == 0), so a row that exists has all kPgTile columns.
    const int rem = N - kb - tb;
    for (int i = threadIdx.x; i < rem; i += kPgBlock) {
      double* row = M + (int64_t)(kb + tb + i) * N + kb;
      double v[kPgTile];
#pragma unroll
      for (int c = 0; c < kPgTile; ++c) {
        double s = row[c];
#pragma unroll
        for (int p = 0; p < c; ++p) s -= v[p] * S.tile[c * kPgTile + p];
        v[c] = s / S.tile[c * kPgTile + c];
      }
#pragma unroll
      for (int c = 0; c < kPgTile; ++c) row[c] = v[c];
    }
    __syncthreads();
    // the trailing lower triangle: entry (i, j), j <= i, loses the panel's products in ascending column
    const int64_t tri = (int64_t)rem * (rem + 1) / 2;
    for (int64_t idx = threadIdx.x; idx < tri; idx += kPgBlock) {
      int i = (int)((sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
      while ((int64_t)i * (i + 1) / 2 > idx) --i;
      while ((int64_t)(i + 1) * (i + 2) / 2 <= idx) ++i;
      const int j = (int)(idx - (int64_t)i * (i + 1) / 2);
      const double* ri = M + (int64_t)(kb + tb + i) * N + kb;
      const double* rj = M + (int64_t)(kb + tb + j) * N + kb;
      double* t = M + (int64_t)(kb + tb + i) * N + kb + tb + j;
      double s = *t;
      for (int c = 0; c < tb; ++c) s -= ri[c] * rj[c];
      *t = s;
    }
    __syncthreads();
  }
  return true;
}

// d with (L L^T) d = -g; g, y, d in LDS
__device__ void pg_solve(const PgArgs& a, const PgDesc& D, PgShared& S) {
  const int N = D.N;
  const double* M = a.M + D.h_off;
  __syncthreads();
  for (int i = threadIdx.x; i < N; i += kPgBlock) S.y[i] = -S.g[i];
  __syncthreads();
  for (int j = 0; j < N; ++j) {  // forward: y_j is final once columns < j were subtracted
    const double yj = S.y[j] / M[(int64_t)j * N + j];
    __syncthreads();
    if (threadIdx.x == 0) S.y[j] = yj;
    for (int i = j + 1 + threadIdx.x; i < N; i += kPgBlock) S.y[i] -= M[(int64_t)i * N + j] * yj;
    __syncthreads();
  }
  for (int i = N - 1; i >= 0; --i) {  // backward, on L^T: row i of L is column i of L^T
    const double xi = S.y[i] / M[(int64_t)i * N + i];
    __syncthreads();
    if (threadIdx.x == 0) S.y[i] = xi;
    for (int k = threadIdx.x; k < i; k += kPgBlock) S.y[k] -= M[(int64_t)i * N + k] * xi;
    __syncthreads();
  }
  for (int i = threadIdx.x; i < N; i += kPgBlock) S.d[i] = S.y[i];
  __syncthreads();
}

// |x|2 over the free poses: a thread per node, then one thread adds in ascending node index
__device__ double pg_xnorm(const PgDesc& D, const double* poses, PgShared& S) {
  __syncthreads();
  for (int i = threadIdx.x; i < D.n; i += kPgBlock) {
    double v[6], s = 0.0;
    pg_v6(poses + 12 * (D.node_off + i), v);
    for (int c = 0; c < 6; ++c) s += v[c] * v[c];
    S.y[i] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < D.n; ++i)
      if (i != D.ref) s += S.y[i];
    S.scalar = sqrt(s);
  }
  __syncthreads();
  return S.scalar;
}

__device__ void pg_trace(const PgArgs& a, const PgDesc& D, int* n_trace, int pass, double lam, double rho, double Fn,
                         int accepted, int factorised) {
  if (threadIdx.x == 0 && a.trace && *n_trace < D.trace_cap) {
    teaser_posegraph_trace_c& t = a.trace[D.trace_off + *n_trace];
    t.lam = lam;
    t.rho = rho;
    t.F_new = Fn;
    t.pass = pass;
    t.accepted = accepted;
    t.factorised = factorised;
    t.reserved = 0;
  }
  *n_trace += 1;  // rows beyond the capacity are dropped, the count is still reported
}

// One event of the controller.  Its state is kept in LDS, not in registers that live across the whole pass: every
// thread reads it after a barrier, runs pg_control on the same values, and thread 0 stores the result.
__device__ int pg_step(PgShared& S, PgEvent ev, double x, double y, double z, const teaser_posegraph_option_c& o) {
  __syncthreads();
  PgCtl c = S.ctl;
  const int status = pg_control(c, ev, x, y, z, o);
  __syncthreads();
  if (threadIdx.x == 0) S.ctl = c;
  __syncthreads();
  return status;
}

// One pass from pose_cur.  Leaves the final poses in pose_cur and the edges' l at those poses in a.l.
__device__ int pg_pass(const PgArgs& a, const PgDesc& D, PgShared& S, int pass, double* F0, double* Fout, double* mu_out,
                       int* iterations, int* trials, int* n_trace) {
  const teaser_posegraph_option_c& o = D.opt;
  const double mu = pg_mu(a, D, S);
  *mu_out = mu;
  double F = pg_eval(a, D, a.pose_cur, mu, true, S);
  *F0 = F;
  double maxdiag, gmax;
  pg_assemble(a, D, S, &maxdiag, &gmax);
  int status = pg_step(S, PG_EV_START, maxdiag, gmax, 0.0, o);
  int ntr = 0;
  for (int64_t left = pg_trial_bound(o); status == PG_GO && left > 0; --left) {
    bool accepted = false;
    if (pg_cholesky(a, D, S.ctl.lam, S)) {
      pg_solve(a, D, S);
      double dd = 0.0, den = 0.0;
      const double lam = S.ctl.lam;
      for (int i = threadIdx.x; i < D.N; i += kPgBlock) {
        const double x = S.d[i];
        dd += x * x;
        den += x * (lam * x - S.g[i]);
      }
      const double dnorm = sqrt(pg_block_sum(dd, S));
      den = pg_block_sum(den, S);
      const double xnorm = pg_xnorm(D, a.pose_cur, S);
      status = pg_step(S, PG_EV_SOLVED, dnorm, xnorm, 0.0, o);
      if (status != PG_GO) break;
      for (int i = threadIdx.x; i < D.n; i += kPgBlock) {
        const double* T = a.pose_cur + 12 * (D.node_off + i);
        double* C = a.pose_cand + 12 * (D.node_off + i);
        if (i == D.ref) {
          for (int k = 0; k < 12; ++k) C[k] = T[k];
        } else {
          double xi[6], Vm[12], t[12], c[12];
          for (int k = 0; k < 6; ++k) xi[k] = S.d[6 * pg_free(i, D.ref) + k];
          for (int k = 0; k < 12; ++k) t[k] = T[k];
          pg_V(xi, Vm);
          pg_mul(Vm, t, c);
          for (int k = 0; k < 12; ++k) C[k] = c[k];
        }
      }
      __syncthreads();
      const double Fn = pg_eval(a, D, a.pose_cand, mu, false, S);
      const double rho = (F - Fn) / den;
      accepted = rho > 0;  // false for a NaN
      pg_trace(a, D, n_trace, pass, S.ctl.lam, rho, Fn, accepted, 1);
      ++ntr;
      if (accepted) {
        status = pg_step(S, PG_EV_GAIN, F - Fn, F, 0.0, o);
        if (status != PG_GO) break;
        for (int i = threadIdx.x; i < 12 * D.n; i += kPgBlock)
          a.pose_cur[12 * D.node_off + i] = a.pose_cand[12 * D.node_off + i];
        __syncthreads();
        F = pg_eval(a, D, a.pose_cur, mu, true, S);  // the same sums as Fn, now with the linearisation stored
        pg_assemble(a, D, S, &maxdiag, &gmax);
        status = pg_step(S, PG_EV_ACCEPTED, gmax, F, rho, o);
      }
    } else {
      pg_trace(a, D, n_trace, pass, S.ctl.lam, 0.0, 0.0, 0, 0);
      ++ntr;
    }
    if (!accepted) status = pg_step(S, PG_EV_REJECTED, 0.0, 0.0, 0.0, o);
  }
  if (status == PG_GO) status = TEASER_HIP_PG_MAX_ITERATION_LM;  // not reachable: pg_trial_bound covers every sequence
  *Fout = F;
  *iterations = S.ctl.it;
  *trials = ntr;
  return status;
}

__global__ __launch_bounds__(kPgBlock) void posegraph_kernel(PgArgs a) {
  __shared__ PgShared S;
  const PgDesc& D = a.desc[blockIdx.x];
  teaser_posegraph_result_c res;
  res.F0 = res.F = 0.0;
  res.mu[0] = res.mu[1] = 0.0;
  res.iterations[0] = res.iterations[1] = res.trials[0] = res.trials[1] = 0;
  res.status = TEASER_HIP_PG_TRIVIAL;
  res.n_trace = 0;
  if (D.trivial) {
    for (int i = threadIdx.x; i < 16 * D.n; i += kPgBlock) a.poses_out[16 * D.node_off + i] = a.poses_in[16 * D.node_off + i];
    for (int k = threadIdx.x; k < D.m; k += kPgBlock) {
      a.conf[D.edge_off + k] = 1.0;
      a.pruned[D.edge_off + k] = 0;
    }
    if (threadIdx.x == 0) a.res[blockIdx.x] = res;
    return;
  }
  for (int i = threadIdx.x; i < D.n * 12; i += kPgBlock)
    a.pose_cur[12 * D.node_off + i] = a.poses_in[16 * D.node_off + (i / 12) * 16 + i % 12];
  for (int k = threadIdx.x; k < D.m; k += kPgBlock) a.pruned[D.edge_off + k] = 0;
  for (int64_t idx = threadIdx.x; idx < (int64_t)D.N * D.N; idx += kPgBlock) a.H[D.h_off + idx] = 0.0;
  __syncthreads();

  if (a.mode == PG_MODE_LINEARIZE) {
    const double mu = pg_mu(a, D, S);
    const double F = pg_eval(a, D, a.pose_cur, mu, true, S);
    double maxdiag, gmax;
    pg_assemble(a, D, S, &maxdiag, &gmax);
    for (int i = threadIdx.x; i < D.N; i += kPgBlock) a.g[D.g_off + i] = S.g[i];
    res.mu[0] = mu;
    res.F0 = res.F = F;
    res.status = PG_GO;
    if (threadIdx.x == 0) a.res[blockIdx.x] = res;
    return;
  }

  int n_trace = 0;
  int status = pg_pass(a, D, S, 0, &res.F0, &res.F, &res.mu[0], &res.iterations[0], &res.trials[0], &n_trace);
  // pruning: an uncertain edge whose l at pass one's final poses is below the threshold
  __syncthreads();
  if (threadIdx.x == 0) S.flag = 0;
  __syncthreads();
  for (int k = threadIdx.x; k < D.m; k += kPgBlock) {
    const int64_t K = D.edge_off + k;
    const double l = a.l[K];
    a.conf[K] = l;
    if (D.opt.edge_prune_threshold > 0 && a.unc[K] && l < D.opt.edge_prune_threshold) {
      a.pruned[K] = 1;
      S.flag = 1;  // every writer stores the same value
    }
  }
  __syncthreads();
  const int any = S.flag;
  __syncthreads();
  if (any) {
    double F0two;
    status = pg_pass(a, D, S, 1, &F0two, &res.F, &res.mu[1], &res.iterations[1], &res.trials[1], &n_trace);
    __syncthreads();
    for (int k = threadIdx.x; k < D.m; k += kPgBlock) {
      const int64_t K = D.edge_off + k;
      if (!a.pruned[K]) a.conf[K] = a.l[K];
    }
  }
  res.status = status;
  res.n_trace = n_trace;
  for (int i = threadIdx.x; i < 16 * D.n; i += kPgBlock) {
    const int node = i / 16, k = i % 16;
    a.poses_out[16 * D.node_off + i] =
        k < 12 ? a.pose_cur[12 * (D.node_off + node) + k] : a.poses_in[16 * D.node_off + i];
  }
  if (threadIdx.x == 0) a.res[blockIdx.x] = res;
}

}  // namespace

void launch_posegraph(hipStream_t s, int batch, const PgArgs& args) {
  if (batch > 0) hipLaunchKernelGGL(posegraph_kernel, dim3(batch), dim3(kPgBlock), 0, s, args);
}

}  // namespace thip
