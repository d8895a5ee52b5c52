// tfm_solve_ops.h — the per-element arithmetic of the least-squares imaging solve (include/alifmm.h
// alifmm_tfm_lsq): the DᵀD stencil on the pixel window, and the element terms of the fused vector
// kernels of the CGLS iteration over image-space vectors ([niz][nix][ncomp]) and data-space vectors
// ([ntx][nrx][nt][ncomp]).  The sums over them are solve_ops.h's (strided lanes, a fixed tree, two
// stages whose partials depend on the length alone).  Shared verbatim by the kernels
// (tfm_solve.hip) and by a stand-alone host program (tests/tfm_lsq_sim.cpp, built with ASan and
// UBSan) that replays them term by term.  Includes nothing from HIP; the includer defines AF_DEV
// (the function qualifier); build with -ffp-contract=off.  Every index is 64-bit: a data-space
// vector passes 2^31 elements at the 64 x 64 x 4096 complex workload.
#pragma once
#include <stdint.h>

#include "solve_ops.h"

namespace af {

struct TfmLsqDims {
  int niz, nix, nc;  // the pixel window and the components per pixel (1 real, 2 complex)
  int64_t nimg;      // niz * nix * nc: elements of an image-space vector
  int64_t ndata;     // ntx * nrx * nt * nc: elements of a data-space vector
};

// (DᵀD v)[e] for element e = (pixel (z, x), component c) of an image-space vector, D the first
// difference between 4-neighbour pixels of the window per component: the differences to the upper,
// left, right and lower neighbour, added in that order (solve_ops.h solve_stencil on the window)
AF_DEV double tfm_lsq_stencil(const double* v, const TfmLsqDims& G, int64_t e) {
  const int64_t q = e / G.nc;
  const int z = (int)(q / G.nix), x = (int)(q % G.nix);
  const int64_t row = (int64_t)G.nix * G.nc;
  const double vc = v[e];
  double s = 0.0;
  if (z > 0) s += vc - v[e - row];
  if (x > 0) s += vc - v[e - G.nc];
  if (x + 1 < G.nix) s += vc - v[e + G.nc];
  if (z + 1 < G.niz) s += vc - v[e + row];
  return s;
}
// the regularisation's share of an element, R(v)[e] = damp² v + smooth² DᵀD v
AF_DEV double tfm_lsq_reg(const double* v, const TfmLsqDims& G, int64_t e, double damp2, double smooth2) {
  return damp2 * v[e] + smooth2 * tfm_lsq_stencil(v, G, e);
}

// |q|² + p·R(p): term i of nimg + ndata, the image's elements first, then the data's
AF_DEV double tfm_lsq_qq_term(const TfmLsqDims& G, const double* p, const double* q, double damp2, double smooth2,
                              int64_t i) {
  if (i < G.nimg) return p[i] * tfm_lsq_reg(p, G, i, damp2, smooth2);
  const double v = q[i - G.nimg];
  return v * v;
}

// x += alpha p (the image's elements); r -= alpha q (the data's): element i of nimg + ndata
AF_DEV void tfm_lsq_update(const TfmLsqDims& G, double* x, const double* p, double* r, const double* q, double alpha,
                           int64_t i) {
  if (i < G.nimg) x[i] = x[i] + alpha * p[i];
  else if (i < G.nimg + G.ndata) r[i - G.nimg] = r[i - G.nimg] - alpha * q[i - G.nimg];
}

// s = t - R(x) at element e, t = Aᵀ r; returns the element's share s² of gamma
AF_DEV double tfm_lsq_s_term(const TfmLsqDims& G, const double* t, const double* x, double* s, double damp2,
                             double smooth2, int64_t e) {
  const double v = t[e] - tfm_lsq_reg(x, G, e, damp2, smooth2);
  s[e] = v;
  return v * v;
}

// p = s + beta p at element e
AF_DEV void tfm_lsq_p(const double* s, double* p, double beta, int64_t e) { p[e] = s[e] + beta * p[e]; }

}  // namespace af
