// Stand-alone host run of the sparse imaging solve's own vector code (csrc/tfm_sparse_ops.h with the
// sums of csrc/solve_ops.h), built with ASan and UBSan by tests/test_tfm_sparse_ref.py.  It replays
// alifmm_tfm_sparse pass by pass as host_tfm.cpp's tfm_sparse_run queues it: the start, the power
// estimate, the prox, the trial's five sums, the momentum pass, the gradient pass and the end, every
// sum as the two-stage sum of the device (lanes, wave tree, workgroup tree, partials), the scalars
// and the host's accept, restart and stop rules, so the index arithmetic is checked on a CPU before
// the kernels run on a GPU.  The two products are a dense matrix here (the kernels behind them have
// their own host models: tests/tfm_lsq_sim.cpp, tests/trace_fir_sim.cpp).  Test infrastructure only.
//   tfm_sparse_sim INPUT OUTPUT   INPUT: the file of tests/tfm_sparse_ref.py write_sim_input();
//   OUTPUT: float64 x [nimg], d - B x [ndata], info12, the L the first iteration began with.  Exit
//   status 0, or 2 on a malformed input.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#define AF_DEV inline
#include "tfm_sparse_ops.h"

using namespace af;

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// the 64 lanes of a wavefront in lock step (tests/solve_sim.cpp), K sums side by side
template <int K>
struct Lanes {
  double a[K][kSolveLanes];
};
// the workgroup's K sums over its 256 lanes lane0 .. lane0 + 255 of `width`
template <int K, class Term>
static void block_sums(long n, int lane0, int width, Term term, double* out) {
  double w[K][kSolveWaves];
  for (int v = 0; v < kSolveWaves; v++) {
    Lanes<K> s;
    for (int l = 0; l < kSolveLanes; l++) {
      double a[K];
      sparse_lane_sums<K>(n, lane0 + v * kSolveLanes + l, width, a, term);
      for (int k = 0; k < K; k++) s.a[k][l] = a[k];
    }
    for (int k = 0; k < K; k++) {
      struct Row {
        double a[kSolveLanes];
      } row;
      for (int l = 0; l < kSolveLanes; l++) row.a[l] = s.a[k][l];
      for (int o = kSolveLanes / 2; o > 0; o >>= 1) {  // solve_wave_tree: v = v + partner(v, o)
        Row nx;
        for (int l = 0; l < kSolveLanes; l++) nx.a[l] = row.a[l] + row.a[l ^ o];
        row = nx;
      }
      w[k][v] = row.a[0];
    }
  }
  for (int k = 0; k < K; k++) out[k] = solve_block_tree(w[k]);
}
// K two-stage sums of one pass (tfm_sparse.hip sparse_part, then sparse_total)
template <int K, class Term>
static void two_stage(long n, Term term, double* out) {
  const int parts = solve_parts(n);
  std::vector<double> part((size_t)K * parts);
  for (int b = 0; b < parts; b++) {
    double s[K];
    block_sums<K>(n, b * kSolveBlock, parts * kSolveBlock, term, s);
    for (int k = 0; k < K; k++) part[(size_t)k * parts + b] = s[k];
  }
  for (int k = 0; k < K; k++) {
    const double* p = part.data() + (size_t)k * parts;
    block_sums<1>(parts, 0, kSolveBlock, [&](long i, double* o) { o[0] = p[i]; }, out + k);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int64_t> h;
  std::vector<double> par, Bm, d;
  if (!rd(f, h, 8) || !rd(f, par, 5)) return 2;
  const int64_t niz = h[0], nix = h[1], nc = h[2], nd = h[3], power_iters = h[4], restart = h[5], max_iter = h[6];
  if (niz < 1 || nix < 1 || (nc != 1 && nc != 2) || nd < 1 || max_iter < 1 || niz * nix > (1 << 20)) return 2;
  const int64_t npix = niz * nix, ni = npix * nc;
  if (nd * ni > (1LL << 27)) return 2;
  if (!rd(f, Bm, (size_t)(nd * ni)) || !rd(f, d, (size_t)nd)) return 2;
  fclose(f);
  const double damp = par[0], smooth = par[1], lipschitz = par[3], tol = par[4];
  double lam = par[2];
  const double d2 = damp * damp, s2 = smooth * smooth;
  TfmLsqDims G;
  G.niz = (int)niz, G.nix = (int)nix, G.nc = (int)nc, G.nimg = ni, G.ndata = nd;

  // the products: out = B v, t = Bᵀ r
  auto forward = [&](const double* v, double* out) {
    for (int64_t i = 0; i < nd; i++) {
      double a = 0.0;
      for (int64_t e = 0; e < ni; e++) a += Bm[(size_t)(i * ni + e)] * v[e];
      out[i] = a;
    }
  };
  auto adjoint = [&](const double* r, double* t) {
    for (int64_t e = 0; e < ni; e++) t[e] = 0.0;
    for (int64_t i = 0; i < nd; i++)
      for (int64_t e = 0; e < ni; e++) t[e] += Bm[(size_t)(i * ni + e)] * r[i];
  };

  std::vector<double> xa((size_t)ni, 0.0), xb((size_t)ni, 0.0), y((size_t)ni, 0.0), g((size_t)ni), t((size_t)ni);
  std::vector<double> bxa((size_t)nd, 0.0), bxb((size_t)nd, 0.0), r((size_t)nd);
  double *x = xa.data(), *xn = xb.data(), *bx = bxa.data(), *bxn = bxb.data();
  double scal[kSpScalars] = {0};

  // the start
  double rhs2;
  two_stage<1>((long)nd, [&](long i, double* o) { o[0] = d[(size_t)i] * d[(size_t)i]; }, &rhs2);
  adjoint(d.data(), t.data());
  two_stage<1>((long)ni, [&](long e, double* o) { sparse_start_term(t.data(), g.data(), e, o); }, &scal[kSpG0]);
  for (int64_t q = 0; q < npix; q++) scal[kSpLamMax] = fmax(scal[kSpLamMax], sparse_modulus(t.data(), (int)nc, q));
  scal[kSpRr] = rhs2;
  scal[kSpFy] = sparse_fy(rhs2, 0.0);
  scal[kSpEst] = sqrt(scal[kSpG0]);
  const double g0 = sqrt(scal[kSpG0]), lam_max = scal[kSpLamMax];
  if (lam < 0) lam = -lam * lam_max;
  double L = lipschitz;
  bool go = g0 != 0.0;
  if (go && !(lipschitz > 0)) {
    if (power_iters < 1) return 2;
    for (int64_t k = 0; k < power_iters; k++) {
      for (int64_t e = 0; e < ni; e++) sparse_power_scale(t.data(), xn, scal[kSpEst], e);
      forward(xn, bxn);
      adjoint(bxn, t.data());
      double s;
      two_stage<1>((long)ni, [&](long e, double* o) { sparse_power_term(G, t.data(), xn, d2, s2, e, o); }, &s);
      scal[kSpEst] = sqrt(s);
    }
    L = scal[kSpEst];
    go = std::isfinite(L) && L > 0;
  }
  const double l0 = go ? L : 0.0;
  int iters = 0, reason = go ? 1 : 2, backtracks = 0, restarts = 0, doublings = 0;
  double theta = 1.0, gk = 0.0;
  for (int64_t k = 1; go && k <= max_iter; k++) {
    double* out4 = scal + kSpOut;
    for (;;) {
      const double step = 1.0 / L, tau = lam * step;
      for (int64_t q = 0; q < npix; q++) sparse_prox(y.data(), g.data(), xn, (int)nc, step, tau, q);
      forward(xn, bxn);
      double s[5];
      two_stage<5>((long)(ni + nd), [&](long i, double* o) {
        sparse_trial_term(G, xn, x, y.data(), g.data(), bxn, d.data(), d2, s2, i, o);
      }, s);
      sparse_trial_scalars(s, scal[kSpFy], L, out4);
      if (out4[0] <= out4[1]) break;
      if (++doublings > kSpMaxDoublings) {
        go = false;
        break;
      }
      L = 2 * L;
      backtracks++;
    }
    if (!go) {
      reason = 2;
      break;
    }
    gk = L * sqrt(out4[2]);
    iters = (int)k;
    std::swap(x, xn);
    std::swap(bx, bxn);
    if (restart && out4[3] > 0) theta = 1.0, restarts++;
    const double theta1 = (1.0 + sqrt(1.0 + 4.0 * theta * theta)) / 2.0, beta = (theta - 1.0) / theta1;
    theta = theta1;
    if (gk <= tol * g0) {
      reason = 0;
      break;
    }
    if (k == max_iter) break;
    double rr, yry;
    two_stage<1>((long)(ni + nd), [&](long i, double* o) {
      sparse_momentum_term(G, x, xn, y.data(), bx, bxn, d.data(), r.data(), beta, i, o);
    }, &rr);
    adjoint(r.data(), t.data());
    two_stage<1>((long)ni, [&](long e, double* o) { sparse_grad_term(G, t.data(), y.data(), g.data(), d2, s2, e, o); },
                 &yry);
    scal[kSpRr] = rr;
    scal[kSpFy] = sparse_fy(rr, yry);
  }
  double fin[2];
  two_stage<2>((long)(nd + npix), [&](long i, double* o) { sparse_final_term(G, x, bx, d.data(), r.data(), i, o); }, fin);
  const double info[13] = {(double)iters, g0, gk, sqrt(rhs2), sqrt(fin[0]), (double)reason, lam_max, lam, L,
                           (double)backtracks, (double)restarts, fin[1], l0};
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const bool ok = fwrite(x, 8, (size_t)ni, o) == (size_t)ni && fwrite(r.data(), 8, (size_t)nd, o) == (size_t)nd &&
                  fwrite(info, 8, 13, o) == 13;
  fclose(o);
  return ok ? 0 : 2;
}
