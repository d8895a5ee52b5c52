// Stand-alone host run of the least-squares imaging solve's own code (csrc/tfm_term.h in its float64
// instantiation, csrc/tfm_model_term.h, csrc/tfm_solve_ops.h with the sums of csrc/solve_ops.h),
// built with ASan and UBSan by tests/test_tfm_lsq_ref.py.  It replays alifmm_tfm_lsq kernel by
// kernel: the dense window's pixel list, Aᵀ with tfm_pixel<.., double>, A with the modelling term
// pixel after pixel, the fused vector kernels' element terms, every dot product as the two-stage
// sum of the device (lanes, wave tree, workgroup tree, partials), the scalars and the stop rule,
// so the index arithmetic is checked on a CPU before the kernels run on a GPU.  Test infrastructure
// only.
//   tfm_lsq_sim INPUT OUTPUT   INPUT: the file of tests/tfm_lsq_ref.py write_sim_input(); OUTPUT:
//   float64 Aᵀ d [nimg], the solve's x [nimg], the recurred r [ndata], info8.  Exit status 0, or 2 on
//   a malformed input.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define AF_DEV inline
#include "tfm_model_term.h"
#include "tfm_solve_ops.h"
#include "tfm_term.h"

using namespace af;

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// the 64 lanes of a wavefront in lock step (tests/solve_sim.cpp)
struct Lanes {
  double a[kSolveLanes];
};
static Lanes operator+(const Lanes& x, const Lanes& y) {
  Lanes r;
  for (int l = 0; l < kSolveLanes; l++) r.a[l] = x.a[l] + y.a[l];
  return r;
}
template <class Term>
static double wave_sum(long n, int lane0, int width, Term term) {
  Lanes v;
  for (int l = 0; l < kSolveLanes; l++) v.a[l] = solve_lane_sum(n, lane0 + l, width, term);
  v = solve_wave_tree(v, [](const Lanes& x, int o) {
    Lanes r;
    for (int l = 0; l < kSolveLanes; l++) r.a[l] = x.a[l ^ o];
    return r;
  });
  return v.a[0];
}
template <class Term>
static double block_sum(long n, int lane0, int width, Term term) {
  double w[kSolveWaves];
  for (int k = 0; k < kSolveWaves; k++) w[k] = wave_sum(n, lane0 + k * kSolveLanes, width, term);
  return solve_block_tree(w);
}
// the two-stage sum of solve_sums.h solve_part + sens_solve.hip solve_scalar_kernel
template <class Term>
static double two_stage(long n, Term term) {
  const int parts = solve_parts(n);
  std::vector<double> part((size_t)parts);
  for (int b = 0; b < parts; b++) part[b] = block_sum(n, b * kSolveBlock, parts * kSolveBlock, term);
  return block_sum(parts, 0, kSolveBlock, [&](long i) { return part[(size_t)i]; });
}

// t = Aᵀ r: tfm.hip's kernel, pixel after pixel
template <int NC>
static void adjoint(TfmParams P, const double* r, double* t) {
  P.fmc64 = r;
  for (int i = 0; i < P.niz; i++)
    for (int j = 0; j < P.nix; j++)
      tfm_pixel<NC, kTfmChunk, double>(P, tfm_pixel_offset(P, i, j), t + ((int64_t)i * P.nix + j) * NC);
}

// q = A p: tfm_model.hip's terms, one pair's trace after the other, the pixels in list order
template <int NC>
static void forward(TfmModelParams M, const double* p, double* q) {
  M.refl = p;
  const int64_t per = (int64_t)M.nt * NC;
  for (int64_t i = 0; i < (int64_t)M.ntx * M.nrx * per; i++) q[i] = 0.0;
  for (int a = 0; a < M.ntx; a++)
    for (int b = 0; b < M.nrx; b++)
      for (int64_t k = 0; k < M.npix; k++)
        tfm_model_pixel<NC, 1>(M, a, b, k, true, 0, 0, M.nt, [&](int, TfmModelSplit<NC> s) {
          tfm_model_add<NC>(s, 0, q + ((int64_t)a * M.nrx + b) * per, [](double* o, double v) { *o += v; });
        });
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int64_t> h;
  std::vector<double> par, fld, d;
  std::vector<int32_t> tx, rx;
  std::vector<float> w;
  if (!rd(f, h, 16) || !rd(f, par, 5)) return 2;
  const int64_t ntx = h[0], nrx = h[1], nt = h[2], nc = h[3], nfld = h[4], fnz = h[5], fnx = h[6], max_iter = h[13];
  if (ntx < 1 || nrx < 1 || nt < 2 || (nc != 1 && nc != 2) || nfld < 1 || fnz < 1 || fnx < 1 || max_iter < 1) return 2;
  if (ntx * nrx * nt * nc > (1LL << 26) || nfld * fnz * fnx > (1LL << 26)) return 2;
  const int64_t nd = ntx * nrx * nt * nc;
  if (!rd(f, tx, ntx) || !rd(f, rx, nrx) || !rd(f, fld, (size_t)(nfld * fnz * fnx)) || !rd(f, d, (size_t)nd) ||
      !rd(f, w, h[12] ? (size_t)(ntx * nrx) : 0))
    return 2;
  fclose(f);
  TfmParams P;
  P.iz0 = (int)h[7], P.ix0 = (int)h[8], P.niz = (int)h[9], P.nix = (int)h[10], P.step = (int)h[11];
  if (P.step < 1 || P.niz < 1 || P.nix < 1 || P.iz0 < 0 || P.ix0 < 0 || P.iz0 + (int64_t)P.step * (P.niz - 1) >= fnz ||
      P.ix0 + (int64_t)P.step * (P.nix - 1) >= fnx)
    return 2;
  std::vector<const double*> tab;
  for (int64_t k = 0; k < ntx + nrx; k++) {
    const int32_t s = k < ntx ? tx[k] : rx[k - ntx];
    if (s < 0 || s >= nfld) return 2;
    tab.push_back(fld.data() + (size_t)s * fnz * fnx);
  }
  const double t0 = par[0], fs = par[1], damp = par[2], smooth = par[3], tol = par[4];
  P.tx = tab.data();
  P.rx = tab.data() + ntx;
  P.fmc = nullptr;
  P.pair_w = h[12] ? w.data() : nullptr;
  P.image = nullptr;
  P.t0 = t0, P.fs = fs;
  P.ntx = (int)ntx, P.nrx = (int)nrx, P.nt = (int)nt, P.ncomp = (int)nc, P.fnx = (int)fnx;
  const int64_t npix = (int64_t)P.niz * P.nix, ni = npix * nc;
  // the pixel list of tfm_lsq_pix_kernel
  std::vector<int64_t> pix((size_t)npix);
  for (int64_t q = 0; q < npix; q++)
    pix[q] = tfm_model_pixel_offset(P.iz0, P.ix0, P.step, P.fnx, (int)(q / P.nix), (int)(q % P.nix));
  TfmModelParams M;
  M.tx = P.tx, M.rx = P.rx, M.pix = pix.data(), M.refl = nullptr, M.pair_w = P.pair_w, M.out = nullptr;
  M.t0 = t0, M.fs = fs, M.npix = npix;
  M.ntx = P.ntx, M.nrx = P.nrx, M.nt = P.nt, M.ncomp = P.ncomp, M.rg = 1, M.tile = P.nt, M.slabs = 1, M.combine = 0;
  TfmLsqDims G;
  G.niz = P.niz, G.nix = P.nix, G.nc = (int)nc, G.nimg = ni, G.ndata = nd;
  const double d2 = damp * damp, s2 = smooth * smooth;

  std::vector<double> x((size_t)ni, 0.0), p((size_t)ni, 0.0), s((size_t)ni), t((size_t)ni), atd, r = d, q((size_t)nd);
  auto At = [&](const double* rr, double* tt) { nc == 2 ? adjoint<2>(P, rr, tt) : adjoint<1>(P, rr, tt); };
  auto A = [&](const double* pp, double* qq) { nc == 2 ? forward<2>(M, pp, qq) : forward<1>(M, pp, qq); };
  auto grad = [&]() {  // tfm_lsq_s_kernel
    return two_stage((long)ni, [&](long e) { return tfm_lsq_s_term(G, t.data(), x.data(), s.data(), d2, s2, e); });
  };
  const double rhs2 = two_stage((long)nd, [&](long i) { return r[(size_t)i] * r[(size_t)i]; });
  At(r.data(), t.data());
  atd = t;
  double gamma0 = grad(), gamma = gamma0;
  for (int64_t e = 0; e < ni; e++) tfm_lsq_p(s.data(), p.data(), 0.0, e);
  int iters = 0, reason = 1;
  if (gamma0 == 0.0) reason = 2;
  else
    for (int it = 1; it <= max_iter; it++) {
      A(p.data(), q.data());
      const double qq = two_stage((long)(ni + nd), [&](long i) { return tfm_lsq_qq_term(G, p.data(), q.data(), d2, s2, i); });
      if (qq == 0.0) {
        reason = 2;
        break;
      }
      const double alpha = gamma / qq;
      for (int64_t i = 0; i < ni + nd; i++) tfm_lsq_update(G, x.data(), p.data(), r.data(), q.data(), alpha, i);
      At(r.data(), t.data());
      const double g1 = grad(), beta = g1 / gamma;
      for (int64_t e = 0; e < ni; e++) tfm_lsq_p(s.data(), p.data(), beta, e);
      gamma = g1;
      iters = it;
      if (gamma <= tol * tol * gamma0) {
        reason = 0;
        break;
      }
    }
  const double res2 = two_stage((long)nd, [&](long i) { return r[(size_t)i] * r[(size_t)i]; });
  const double info[8] = {(double)iters, sqrt(gamma0), sqrt(gamma), sqrt(rhs2), sqrt(res2), (double)reason, 0.0, 0.0};
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 2;
  bool ok = fwrite(atd.data(), 8, atd.size(), g) == atd.size() && fwrite(x.data(), 8, x.size(), g) == x.size() &&
            fwrite(r.data(), 8, r.size(), g) == r.size() && fwrite(info, 8, 8, g) == 8;
  fclose(g);
  return ok ? 0 : 2;
}
