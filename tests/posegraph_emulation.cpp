// The pose-graph kernel's arithmetic on the CPU, single-threaded, from the functions of csrc/posegraph_device.h that
// the kernel itself calls: the edge residual and system, the assembly in ascending edge index, a plain Cholesky (the
// blocked one subtracts the same products in the same ascending order, so the two agree bit for bit), the sums in the
// kernel's order (a partial per thread over its strided elements, then the tree over kPgBlock partials) and the shared
// controller pg_control.  tests/test_posegraph_emulation.py writes a graph file, runs this program under
// AddressSanitizer / UndefinedBehaviorSanitizer and compares the results with the numpy restatement.
//   posegraph_emulation <graph file> <result file>
// graph file (text): n m / 12 option fields / n x 16 poses / m x (s t uncertain, 16 X, 36 L)
// result file (text): status it0 it1 tr0 tr1 F0 F mu0 mu1 / n x 16 poses / m x (confidence pruned) / n_trace /
//                     rows (pass lam rho F_new accepted factorised)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "posegraph_device.h"

using namespace thip;

struct Graph {
  int n = 0, m = 0, ref = 0, N = 0;
  teaser_posegraph_option_c opt;
  std::vector<double> poses, X, L;  // 12 per node, 12 per edge, 36 per edge
  std::vector<int> s, t, unc, pruned;
};

struct Row {
  int pass;
  double lam, rho, Fn;
  int accepted, factorised;
};

static double block_sum(const std::vector<double>& v) {  // pg_block_sum over per-thread strided partials
  double red[kPgBlock];
  for (int t = 0; t < kPgBlock; ++t) {
    double p = 0.0;
    for (size_t k = (size_t)t; k < v.size(); k += kPgBlock) p += v[k];
    red[t] = p;
  }
  for (int o = kPgBlock / 2; o > 0; o >>= 1)
    for (int t = 0; t < o; ++t) red[t] += red[t + o];
  return red[0];
}

struct Lin {
  std::vector<double> e, r, l, A, b;
};

static double eval(const Graph& G, const std::vector<double>& poses, double mu, Lin* lin) {
  std::vector<double> f((size_t)G.m, 0.0);
  for (int k = 0; k < G.m; ++k) {
    if (G.pruned[(size_t)k]) continue;
    double B[12], e[6], r, l;
    const double* Ts = &poses[12 * (size_t)G.s[(size_t)k]];
    pg_edge_residual(Ts, &poses[12 * (size_t)G.t[(size_t)k]], &G.X[12 * (size_t)k], &G.L[36 * (size_t)k],
                     G.unc[(size_t)k], mu, B, e, &r, &l, &f[(size_t)k]);
    if (lin) {
      pg_edge_system(B, Ts, &G.L[36 * (size_t)k], e, l, &lin->A[36 * (size_t)k], &lin->b[6 * (size_t)k]);
      for (int i = 0; i < 6; ++i) lin->e[6 * (size_t)k + i] = e[i];
      lin->r[(size_t)k] = r;
      lin->l[(size_t)k] = l;
    }
  }
  // the kernel's partials skip pruned edges; their f is 0 here, and adding +0.0 changes no bit of a sum of these terms
  return block_sum(f);
}

static void assemble(const Graph& G, const Lin& lin, std::vector<double>& H, std::vector<double>& g) {
  const int N = G.N;
  H.assign((size_t)N * N, 0.0);
  g.assign((size_t)N, 0.0);
  for (int k = 0; k < G.m; ++k) {  // ascending edge index: every entry receives its edges in that order
    if (G.pruned[(size_t)k]) continue;
    const int s = G.s[(size_t)k], t = G.t[(size_t)k];
    const double* A = &lin.A[36 * (size_t)k];
    const double* b = &lin.b[6 * (size_t)k];
    const int fs = s == G.ref ? -1 : 6 * pg_free(s, G.ref), ft = t == G.ref ? -1 : 6 * pg_free(t, G.ref);
    for (int a = 0; a < 6; ++a) {
      for (int c = 0; c < 6; ++c) {
        if (fs >= 0) H[(size_t)(fs + a) * N + fs + c] += A[6 * a + c];
        if (ft >= 0) H[(size_t)(ft + a) * N + ft + c] += A[6 * a + c];
        if (fs >= 0 && ft >= 0) {
          H[(size_t)(fs + a) * N + ft + c] -= A[6 * a + c];
          H[(size_t)(ft + a) * N + fs + c] -= A[6 * c + a];
        }
      }
      if (fs >= 0) g[(size_t)fs + a] += b[a];
      if (ft >= 0) g[(size_t)ft + a] -= b[a];
    }
  }
}

static bool cholesky_solve(const std::vector<double>& H, double lam, const std::vector<double>& g, int N,
                           std::vector<double>& d) {
  std::vector<double> M((size_t)N * N, 0.0);
  for (int j = 0; j < N; ++j) {
    double dv = H[(size_t)j * N + j] + lam;
    for (int p = 0; p < j; ++p) dv -= M[(size_t)j * N + p] * M[(size_t)j * N + p];
    if (!std::isfinite(dv) || !(dv > 0)) return false;
    const double piv = sqrt(dv);
    M[(size_t)j * N + j] = piv;
    for (int i = j + 1; i < N; ++i) {
      double v = H[(size_t)i * N + j];
      for (int p = 0; p < j; ++p) v -= M[(size_t)i * N + p] * M[(size_t)j * N + p];
      M[(size_t)i * N + j] = v / piv;
    }
  }
  std::vector<double> y((size_t)N);
  for (int i = 0; i < N; ++i) {
    double v = -g[(size_t)i];
    for (int j = 0; j < i; ++j) v -= M[(size_t)i * N + j] * y[(size_t)j];
    y[(size_t)i] = v / M[(size_t)i * N + i];
  }
  d.assign((size_t)N, 0.0);
  for (int k = N - 1; k >= 0; --k) {
    double v = y[(size_t)k];
    for (int i = N - 1; i > k; --i) v -= M[(size_t)i * N + k] * d[(size_t)i];
    d[(size_t)k] = v / M[(size_t)k * N + k];
  }
  return true;
}

static double mu_of(const Graph& G) {
  double sum = 0.0;
  int cnt = 0;
  for (int k = 0; k < G.m; ++k)
    if (G.unc[(size_t)k] && !G.pruned[(size_t)k]) {
      sum += G.L[36 * (size_t)k + 35];
      ++cnt;
    }
  const double mcd = G.opt.max_correspondence_distance;
  return cnt ? G.opt.preference_loop_closure * mcd * mcd * (sum / (double)cnt) : 0.0;
}

static int run_pass(Graph& G, int pass, double* F0, double* Fout, double* mu_out, int* iterations, int* trials,
                    std::vector<Row>& trace, Lin& lin) {
  const teaser_posegraph_option_c& o = G.opt;
  const double mu = mu_of(G);
  *mu_out = mu;
  double F = eval(G, G.poses, mu, &lin);
  *F0 = F;
  std::vector<double> H, g, d;
  assemble(G, lin, H, g);
  auto maxdiag = [&] {
    double v = -INFINITY;
    for (int i = 0; i < G.N; ++i) v = (v != v || H[(size_t)i * G.N + i] != H[(size_t)i * G.N + i]) ? NAN : fmax(v, H[(size_t)i * G.N + i]);
    return v;
  };
  auto gmax = [&] {
    double v = 0.0;
    for (int i = 0; i < G.N; ++i) v = (v != v || g[(size_t)i] != g[(size_t)i]) ? NAN : fmax(v, fabs(g[(size_t)i]));
    return v;
  };
  PgCtl ctl;
  int status = pg_control(ctl, PG_EV_START, maxdiag(), gmax(), 0.0, o);
  int ntr = 0;
  for (int64_t left = pg_trial_bound(o); status == PG_GO && left > 0; --left) {
    const double lam = ctl.lam;
    bool accepted = false;
    if (cholesky_solve(H, lam, g, G.N, d)) {
      std::vector<double> dd((size_t)G.N), den((size_t)G.N);
      for (int i = 0; i < G.N; ++i) {
        dd[(size_t)i] = d[(size_t)i] * d[(size_t)i];
        den[(size_t)i] = d[(size_t)i] * (lam * d[(size_t)i] - g[(size_t)i]);
      }
      const double dnorm = sqrt(block_sum(dd)), denom = block_sum(den);
      double xs = 0.0;
      for (int i = 0; i < G.n; ++i) {
        if (i == G.ref) continue;
        double v[6], s = 0.0;
        pg_v6(&G.poses[12 * (size_t)i], v);
        for (int c = 0; c < 6; ++c) s += v[c] * v[c];
        xs += s;
      }
      status = pg_control(ctl, PG_EV_SOLVED, dnorm, sqrt(xs), 0.0, o);
      if (status != PG_GO) break;
      std::vector<double> cand(G.poses);
      for (int i = 0; i < G.n; ++i) {
        if (i == G.ref) continue;
        double Vm[12];
        pg_V(&d[6 * (size_t)pg_free(i, G.ref)], Vm);
        pg_mul(Vm, &G.poses[12 * (size_t)i], &cand[12 * (size_t)i]);
      }
      const double Fn = eval(G, cand, mu, nullptr);
      const double rho = (F - Fn) / denom;
      accepted = rho > 0;
      trace.push_back(Row{pass, lam, rho, Fn, accepted, 1});
      ++ntr;
      if (accepted) {
        status = pg_control(ctl, PG_EV_GAIN, F - Fn, F, 0.0, o);
        if (status != PG_GO) break;
        G.poses = cand;
        F = eval(G, G.poses, mu, &lin);
        assemble(G, lin, H, g);
        status = pg_control(ctl, PG_EV_ACCEPTED, gmax(), F, rho, o);
      }
    } else {
      trace.push_back(Row{pass, lam, 0.0, 0.0, 0, 0});
      ++ntr;
    }
    if (!accepted) status = pg_control(ctl, PG_EV_REJECTED, 0.0, 0.0, 0.0, o);
  }
  if (status == PG_GO) status = TEASER_HIP_PG_MAX_ITERATION_LM;
  *Fout = F;
  *iterations = ctl.it;
  *trials = ntr;
  return status;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 2;
  Graph G;
  teaser_posegraph_option_c& o = G.opt;
  int ok = fscanf(in, "%d %d", &G.n, &G.m) == 2;
  ok = ok && fscanf(in, "%d %d %lf %lf %lf %lf %lf %lf %lf %lf %lf %d", &o.max_iteration, &o.max_iteration_lm,
                    &o.min_relative_increment, &o.min_relative_residual_increment, &o.min_right_term, &o.min_residual,
                    &o.upper_scale_factor, &o.lower_scale_factor, &o.max_correspondence_distance,
                    &o.edge_prune_threshold, &o.preference_loop_closure, &o.reference_node) == 12;
  o.reserved = 0;
  if (!ok || G.n < 0 || G.m < 0 || G.n > TEASER_HIP_POSEGRAPH_MAX_NODES || G.m > TEASER_HIP_POSEGRAPH_MAX_EDGES) return 2;
  G.ref = o.reference_node < 0 ? 0 : o.reference_node;
  G.N = G.n > 1 ? 6 * (G.n - 1) : 0;
  std::vector<double> last((size_t)4 * G.n);
  G.poses.resize((size_t)12 * G.n);
  for (int i = 0; i < G.n; ++i)
    for (int k = 0; k < 16; ++k) ok = ok && fscanf(in, "%lf", k < 12 ? &G.poses[12 * (size_t)i + k] : &last[4 * (size_t)i + k - 12]) == 1;
  G.s.resize((size_t)G.m);
  G.t.resize((size_t)G.m);
  G.unc.resize((size_t)G.m);
  G.pruned.assign((size_t)G.m, 0);
  G.X.resize((size_t)12 * G.m);
  G.L.resize((size_t)36 * G.m);
  for (int k = 0; k < G.m; ++k) {
    ok = ok && fscanf(in, "%d %d %d", &G.s[(size_t)k], &G.t[(size_t)k], &G.unc[(size_t)k]) == 3;
    double skip;
    for (int q = 0; q < 16; ++q) ok = ok && fscanf(in, "%lf", q < 12 ? &G.X[12 * (size_t)k + q] : &skip) == 1;
    for (int q = 0; q < 36; ++q) ok = ok && fscanf(in, "%lf", &G.L[36 * (size_t)k + q]) == 1;
    ok = ok && G.s[(size_t)k] >= 0 && G.s[(size_t)k] < G.n && G.t[(size_t)k] >= 0 && G.t[(size_t)k] < G.n &&
         G.s[(size_t)k] != G.t[(size_t)k];
  }
  fclose(in);
  if (!ok || (G.n > 0 && G.ref >= G.n)) return 2;

  int status = TEASER_HIP_PG_TRIVIAL, it[2] = {0, 0}, tr[2] = {0, 0};
  double F0 = 0.0, F = 0.0, mu[2] = {0.0, 0.0};
  std::vector<double> conf((size_t)G.m, 1.0);
  std::vector<Row> trace;
  if (G.n > 1 && G.m > 0) {
    Lin lin;
    lin.e.resize((size_t)6 * G.m);
    lin.r.resize((size_t)G.m);
    lin.l.resize((size_t)G.m);
    lin.A.resize((size_t)36 * G.m);
    lin.b.resize((size_t)6 * G.m);
    status = run_pass(G, 0, &F0, &F, &mu[0], &it[0], &tr[0], trace, lin);
    bool any = false;
    for (int k = 0; k < G.m; ++k) {
      conf[(size_t)k] = lin.l[(size_t)k];
      if (o.edge_prune_threshold > 0 && G.unc[(size_t)k] && lin.l[(size_t)k] < o.edge_prune_threshold) {
        G.pruned[(size_t)k] = 1;
        any = true;
      }
    }
    if (any) {
      double F0two;
      status = run_pass(G, 1, &F0two, &F, &mu[1], &it[1], &tr[1], trace, lin);
      for (int k = 0; k < G.m; ++k)
        if (!G.pruned[(size_t)k]) conf[(size_t)k] = lin.l[(size_t)k];
    }
  }
  FILE* out = fopen(argv[2], "w");
  if (!out) return 2;
  fprintf(out, "%d %d %d %d %d %.17g %.17g %.17g %.17g\n", status, it[0], it[1], tr[0], tr[1], F0, F, mu[0], mu[1]);
  for (int i = 0; i < G.n; ++i) {
    for (int k = 0; k < 16; ++k) fprintf(out, "%.17g ", k < 12 ? G.poses[12 * (size_t)i + k] : last[4 * (size_t)i + k - 12]);
    fprintf(out, "\n");
  }
  for (int k = 0; k < G.m; ++k) fprintf(out, "%.17g %d\n", conf[(size_t)k], G.pruned[(size_t)k]);
  fprintf(out, "%zu\n", trace.size());
  for (const Row& r : trace) fprintf(out, "%d %.17g %.17g %.17g %d %d\n", r.pass, r.lam, r.rho, r.Fn, r.accepted, r.factorised);
  fclose(out);
  return 0;
}
