// tfm_term.h — the total-focusing-method (TFM) delay-and-sum of include/alifmm.h alifmm_tfm(): one
// term, and the loop over all (transmitter, receiver) pairs of one pixel.  Shared verbatim by the
// kernel (tfm.hip) and by a stand-alone host program (tests/tfm_sim.cpp, built with UBSan), so the
// range test and the integer conversion are checked on a CPU before the kernel runs.  Includes
// nothing from HIP; build with -ffp-contract=off (the contract fixes the operation order).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AF_TFM_HD __host__ __device__
#else
#define AF_TFM_HD
#endif

namespace af {

// receivers whose delays a pixel holds in registers while it walks the transmitters (the default;
// tfm.hip also instantiates 4, 16 and 32, option "tfm_chunk")
constexpr int kTfmChunk = 8;

struct TfmParams {
  const double* const* tx;  // [ntx] transmitter fields (fnz x fnx, row-major)
  const double* const* rx;  // [nrx] receiver fields, same shape
  const float* fmc;         // [ntx][nrx][nt][ncomp], S = float
  const float* pair_w;      // [ntx][nrx] or nullptr (all 1)
  double* image;            // [niz][nix][ncomp]
  double t0, fs;
  int ntx, nrx, nt, ncomp;
  int fnx;                  // field row pitch
  int iz0, ix0, niz, nix, step;
  const double* fmc64 = nullptr;  // the same, S = double (fmc is not read then)
};

// the data of sample type S
template <class S>
AF_TFM_HD inline const S* tfm_samples(const TfmParams& P);
template <>
AF_TFM_HD inline const float* tfm_samples<float>(const TfmParams& P) { return P.fmc; }
template <>
AF_TFM_HD inline const double* tfm_samples<double>(const TfmParams& P) { return P.fmc64; }

// field offset of pixel (i, j) of the window
AF_TFM_HD inline int64_t tfm_pixel_offset(const TfmParams& P, int i, int j) {
  return ((int64_t)P.iz0 + (int64_t)P.step * i) * P.fnx + ((int64_t)P.ix0 + (int64_t)P.step * j);
}

// acc[c] += w * lerp(s, u), u = ((ta + tb) - t0) * fs, for the A-scan s[nt][NC] of one pair; the
// term is 0 unless `live`, w != 0 and 0 <= u < nt - 1 (NaN, +-inf and huge delays fail the test,
// which comes before the conversion to an integer; then 0 <= k <= nt - 2 < 2^31, so the int
// conversion is exact).  Written without branches, so that the kernel's unrolled chunk issues all
// its gathers before it waits for the first: a term that does not count reads samples 0 and 1 and
// adds 0.0 instead of its value, which leaves the bits of acc as they are (acc is never -0.0: it
// starts at +0.0, and a sum is -0.0 only if both operands are).
template <int NC, class S>
AF_TFM_HD inline void tfm_term(double ta, double tb, double w, bool live, const S* s, int nt, double t0,
                               double fs, double* acc) {
  const double u = ((ta + tb) - t0) * fs;
  const bool ok = live & (w != 0.0) & (u >= 0.0) & (u < (double)(nt - 1));
  const int k = (int)(ok ? u : 0.0);
  const double f = u - (double)k;
  const S* p = s + (int64_t)k * NC;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    const double x0 = (double)p[c], x1 = (double)p[NC + c];
    const double t = w * (x0 + f * (x1 - x0));
    acc[c] += ok ? t : 0.0;
  }
}

// the image value of the pixel at field offset `off`: receivers in chunks of RC, every transmitter
// per chunk, the chunk's receivers in order.  The order depends on nothing but (ntx, nrx, RC).
template <int NC, int RC, class S = float>
AF_TFM_HD inline void tfm_pixel(const TfmParams& P, int64_t off, double* acc) {
  const S* fmc = tfm_samples<S>(P);
#pragma unroll
  for (int c = 0; c < NC; c++) acc[c] = 0.0;
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
        tfm_term<NC>(ta, tb[j], w, live, fmc + pair * scan, P.nt, P.t0, P.fs, acc);
      }
    }
  }
}

}  // namespace af
