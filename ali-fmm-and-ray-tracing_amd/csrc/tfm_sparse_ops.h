// tfm_sparse_ops.h — the per-element arithmetic of sparsity-regularised imaging (include/alifmm.h
// alifmm_tfm_sparse): FISTA with backtracking and gradient restart on
//   F(x) = ½ |B x - d|² + ½ x·R(x) + lam Σ_pixels |x_p|,   B = P A,  R(v) = damp² v + smooth² DᵀD v.
// This file holds the element terms of the fused vector passes between the two products, over
// image-space vectors ([niz][nix][ncomp]) and data-space vectors ([ntx][nrx][nt][ncomp]), and the
// scalars that follow from their sums.  The sums over them are solve_ops.h's two-stage sums, several
// of one pass side by side (sparse_lane_sums: the order of solve_lane_sum for each).  Shared verbatim
// by the kernels (tfm_sparse.hip) and by a stand-alone host program (tests/tfm_sparse_sim.cpp, built
// with ASan and UBSan) that replays them term by term.  Includes nothing from HIP; the includer
// defines AF_DEV (the function qualifier); build with -ffp-contract=off.  sqrt and the division are
// IEEE's, correctly rounded on the host and on the device alike.  Every index is 64-bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "tfm_solve_ops.h"

namespace af {

// the scalars of a solve on the device (scal[kSpScalars])
enum {
  kSpG0 = 0,   // |g0|²
  kSpLamMax,   // max_p |g0_p|
  kSpRr,       // |r|² of the last momentum pass (|d|² at the start)
  kSpFy,       // fy = ½ |r|² + ½ y·R(y)
  kSpEst,      // the power iteration's |w|
  kSpOut,      // 4 values, the one read of a trial: f⁺, Q + 2⁻⁴⁰ fy, |x⁺ - y|², (y - x⁺)·(x⁺ - x)
  kSpRes = kSpOut + 4,  // |d - B x|² of the returned x
  kSpNnz,      // its non-zero pixels
  kSpScalars = 16
};
// partial-sum arrays of kSolveMaxParts each: a pass's sums lie side by side from array 0 on; |r|² of
// the momentum pass has an array of its own (it is summed up by the next gradient pass's stage 2)
constexpr int kSpPartArrays = 6;
constexpr int kSpPartRr = 5;
// the accept test's slack, a constant of the contract: f⁺ <= Q + kSpSlack fy
constexpr double kSpSlack = 0x1p-40;
// doublings of L in one call before the solve gives up (breakdown)
constexpr int kSpMaxDoublings = 60;

// K sums of one pass over n elements by `width` lanes: lane l visits the elements l, l + width, ...
// in that order and adds term(e, t)'s K values to its K sums one by one, each starting from 0: for
// every sum the order of solve_ops.h solve_lane_sum
template <int K, class Term>
AF_DEV void sparse_lane_sums(long n, int lane, int width, double* a, Term term) {
  for (int k = 0; k < K; k++) a[k] = 0.0;
  for (long e = lane; e < n; e += width) {
    double t[K];
    term(e, t);
    for (int k = 0; k < K; k++) a[k] += t[k];
  }
}

// the modulus of pixel q over its components
AF_DEV double sparse_modulus(const double* v, int nc, int64_t q) {
  if (nc == 1) return fabs(v[q]);
  const double re = v[2 * q], im = v[2 * q + 1];
  return sqrt(re * re + im * im);
}

// the start, element e of nimg, from t = Bᵀ d: g = -t (the gradient at y = 0); t[0] = t², the
// element's share of |g0|²
AF_DEV void sparse_start_term(const double* t, double* g, int64_t e, double* out) {
  const double v = t[e];
  g[e] = -v;
  out[0] = v * v;
}

// the power iteration, element e of nimg: w = t + R(v) in place in t (t = Bᵀ B v); out[0] = w²
AF_DEV void sparse_power_term(const TfmLsqDims& G, double* t, const double* v, double damp2, double smooth2, int64_t e,
                              double* out) {
  const double w = t[e] + tfm_lsq_reg(v, G, e, damp2, smooth2);
  t[e] = w;
  out[0] = w * w;
}
// ... and its normalisation v = w / |w|
AF_DEV void sparse_power_scale(const double* w, double* v, double norm, int64_t e) { v[e] = w[e] / norm; }

// the gradient at y, element e of nimg: g = t + R(y) with t = Bᵀ r; out[0] = y R(y), the element's
// share of y·R(y)
AF_DEV void sparse_grad_term(const TfmLsqDims& G, const double* t, const double* y, double* g, double damp2,
                             double smooth2, int64_t e, double* out) {
  const double reg = tfm_lsq_reg(y, G, e, damp2, smooth2);
  g[e] = t[e] + reg;
  out[0] = y[e] * reg;
}
// fy from the two sums
AF_DEV double sparse_fy(double rr, double yry) { return 0.5 * rr + 0.5 * yry; }

// the prox of pixel q: z = y - step g; m = |z|; m > tau: x⁺ = z (m - tau) / m, else +0.0
AF_DEV void sparse_prox(const double* y, const double* g, double* xn, int nc, double step, double tau, int64_t q) {
  double z[2];
  for (int c = 0; c < nc; c++) z[c] = y[nc * q + c] - step * g[nc * q + c];
  const double m = sparse_modulus(z, nc, 0);
  const bool keep = m > tau;
  const double fac = keep ? (m - tau) / m : 0.0;
  for (int c = 0; c < nc; c++) xn[nc * q + c] = keep ? z[c] * fac : 0.0;
}

// the trial's sums, element i of nimg + ndata (the image's elements first, then the data's):
//   out[0] |B x⁺ - d|² (data)     out[1] x⁺·R(x⁺)     out[2] g·(x⁺ - y)     out[3] |x⁺ - y|²
//   out[4] (y - x⁺)·(x⁺ - x), the restart test
AF_DEV void sparse_trial_term(const TfmLsqDims& G, const double* xn, const double* x, const double* y, const double* g,
                              const double* bxn, const double* d, double damp2, double smooth2, int64_t i, double* out) {
  if (i < G.nimg) {
    const double v = xn[i], dy = v - y[i];
    out[0] = 0.0;
    out[1] = v * tfm_lsq_reg(xn, G, i, damp2, smooth2);
    out[2] = g[i] * dy;
    out[3] = dy * dy;
    out[4] = (y[i] - v) * (v - x[i]);
  } else {
    const double r = bxn[i - G.nimg] - d[i - G.nimg];
    out[0] = r * r;
    out[1] = out[2] = out[3] = out[4] = 0.0;
  }
}
// the four values the host reads after a trial, from the five sums and fy
AF_DEV void sparse_trial_scalars(const double* s, double fy, double L, double* out4) {
  out4[0] = 0.5 * s[0] + 0.5 * s[1];                          // f⁺
  out4[1] = ((fy + s[2]) + (0.5 * L) * s[3]) + kSpSlack * fy;  // Q and the slack
  out4[2] = s[3];
  out4[3] = s[4];
}

// the momentum step, element i of nimg + ndata: y = x⁺ + beta (x⁺ - x) (the image's elements);
// r = (B x⁺ + beta (B x⁺ - B x)) - d (the data's), out[0] = r²
AF_DEV void sparse_momentum_term(const TfmLsqDims& G, const double* xn, const double* x, double* y, const double* bxn,
                                 const double* bx, const double* d, double* r, double beta, int64_t i, double* out) {
  if (i < G.nimg) {
    y[i] = xn[i] + beta * (xn[i] - x[i]);
    out[0] = 0.0;
  } else {
    const int64_t k = i - G.nimg;
    const double v = (bxn[k] + beta * (bxn[k] - bx[k])) - d[k];
    r[k] = v;
    out[0] = v * v;
  }
}

// the end, element i of ndata + npix (the data's elements first, then the pixels): r = d - B x,
// out[0] = r²; out[1] = 1 for a pixel with a non-zero component
AF_DEV void sparse_final_term(const TfmLsqDims& G, const double* x, const double* bx, const double* d, double* r,
                              int64_t i, double* out) {
  if (i < G.ndata) {
    const double v = d[i] - bx[i];
    r[i] = v;
    out[0] = v * v;
    out[1] = 0.0;
  } else {
    const int64_t q = i - G.ndata;
    bool any = false;
    for (int c = 0; c < G.nc; c++) any |= x[G.nc * q + c] != 0.0;
    out[0] = 0.0;
    out[1] = any ? 1.0 : 0.0;
  }
}

}  // namespace af
