// tfm_coh_term.h — the coherence-weighted TFM of include/alifmm.h alifmm_tfm_coh(): one term, the
// loop over all (transmitter, receiver) pairs of one pixel, and the factor.  The delay-and-sum is
// tfm_term.h's, statement for statement (so the image has alifmm_tfm's bits); next to it every
// counting term adds to the count n and to the sums of one KIND: 1 the coherence factor (q, the
// energy), 2 the sign coherence factor (b, the signs of the RF part), 3 the phase coherence factor
// (ph, the unit phasors).  Shared verbatim by the kernel (tfm_coh.hip) and by a stand-alone host
// program (tests/tfm_coh_sim.cpp, built with UBSan).  Includes nothing from HIP; build with
// -ffp-contract=off and without fast-math (the float64 sqrt and division are correctly rounded).
#pragma once
#include "tfm_term.h"

namespace af {

struct TfmCohParams {
  TfmParams T;     // alifmm_tfm's block (float32 data; T.image is the image)
  double* factor;  // [niz][nix]
  double* sums;    // [niz][nix][3] or nullptr
};

// the sums of one pixel: the image's, the count of the terms in range, and the kind's own
// (KIND 1: x[0] = q; 2: x[0] = b; 3: x[0], x[1] = ph; what is not used stays 0)
template <int NC>
struct TfmCohAcc {
  double s[NC];
  double n;
  double x[2];
};

// tfm_term with the sums of KIND.  As there, without branches: a term that does not count reads
// samples 0 and 1 and adds 0.0 to every accumulator, which leaves their bits as they are (none is
// ever -0.0: each starts at +0.0, and a sum is -0.0 only if both operands are).
template <int NC, int KIND, class S>
AF_TFM_HD inline void tfm_coh_term(double ta, double tb, double w, bool live, const S* s, int nt, double t0,
                                   double fs, TfmCohAcc<NC>& A) {
  const double u = ((ta + tb) - t0) * fs;
  const bool ok = live & (w != 0.0) & (u >= 0.0) & (u < (double)(nt - 1));
  const int k = (int)(ok ? u : 0.0);
  const double f = u - (double)k;
  const S* p = s + (int64_t)k * NC;
  double tc[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) {
    const double x0 = (double)p[c], x1 = (double)p[NC + c];
    const double t = w * (x0 + f * (x1 - x0));
    A.s[c] += ok ? t : 0.0;
    tc[c] = t;
  }
  A.n += ok ? 1.0 : 0.0;
  if (KIND == 2) {
    const double sg = (double)((int)(tc[0] > 0.0) - (int)(tc[0] < 0.0));
    A.x[0] += ok ? sg : 0.0;
  } else {
    double e = tc[0] * tc[0];
    if (NC == 2) e = e + tc[NC - 1] * tc[NC - 1];
    if (KIND == 1) {
      A.x[0] += ok ? e : 0.0;
    } else {
      const double g = __builtin_sqrt(e);
      const bool pos = ok & (g > 0.0);  // g 0 or NaN: the term counts in n and adds nothing to ph
      const double r = 1.0 / g;
#pragma unroll
      for (int c = 0; c < NC; c++) A.x[c] += pos ? tc[c] * r : 0.0;
    }
  }
}

// the sums of the pixel at field offset `off`, in tfm_pixel's order: receivers in chunks of RC,
// every transmitter per chunk, the chunk's receivers in order
template <int NC, int RC, int KIND>
AF_TFM_HD inline void tfm_coh_pixel(const TfmParams& P, int64_t off, TfmCohAcc<NC>& A) {
  static_assert(KIND >= 1 && KIND <= 3 && (KIND != 3 || NC == 2), "kind 1, 2, or 3 on complex data");
  const float* fmc = P.fmc;
#pragma unroll
  for (int c = 0; c < NC; c++) A.s[c] = 0.0;
  A.n = A.x[0] = A.x[1] = 0.0;
  const int64_t scan = (int64_t)P.nt * NC;  // samples per A-scan
  for (int b0 = 0; b0 < P.nrx; b0 += RC) {
    double tb[RC];
#pragma unroll
    for (int j = 0; j < RC; j++) tb[j] = b0 + j < P.nrx ? P.rx[b0 + j][off] : 0.0;
    for (int a = 0; a < P.ntx; a++) {
      const double ta = P.tx[a][off];
      const int64_t row = (int64_t)a * P.nrx + b0;
#pragma unroll
      for (int j = 0; j < RC; j++) {
        const bool live = b0 + j < P.nrx;  // past the last receiver: the chunk's first pair, not counted
        const int64_t pair = row + (live ? j : 0);
        const double w = P.pair_w ? (double)P.pair_w[pair] : 1.0;
        tfm_coh_term<NC, KIND>(ta, tb[j], w, live, fmc + pair * scan, P.nt, P.t0, P.fs, A);
      }
    }
  }
}

// the factor of the pixel's sums, operations in the contract's order
template <int NC, int KIND>
AF_TFM_HD inline double tfm_coh_factor(const TfmCohAcc<NC>& A) {
  if (KIND == 1) {
    double num = A.s[0] * A.s[0];
    if (NC == 2) num = num + A.s[NC - 1] * A.s[NC - 1];
    const double den = A.n * A.x[0];
    return den > 0.0 ? num / den : 0.0;
  }
  double y;
  if (KIND == 2) {
    const double m = A.x[0] / A.n;
    y = 1.0 - m * m;
  } else {
    const double num = A.x[0] * A.x[0] + A.x[1] * A.x[1];
    y = 1.0 - num / (A.n * A.n);
    if (y < 0.0) y = 0.0;
  }
  return A.n > 0.0 ? 1.0 - __builtin_sqrt(y) : 0.0;
}

}  // namespace af
