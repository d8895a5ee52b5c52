// tfm_model_term.h — FMC modelling, the transpose of the TFM sum (include/alifmm.h
// alifmm_tfm_model()): one term spread over the two samples it touches, the time-tile membership
// of each of the two adds, and the pass of one workgroup's traces over the pixels.  Shared
// verbatim by the kernel (tfm_model.hip) and by a stand-alone host program
// (tests/tfm_model_sim.cpp, built with UBSan), so the range test, the integer conversion and the
// tiling are checked on a CPU before the kernel runs.  Includes nothing from HIP; build with
// -ffp-contract=off (the contract fixes the operation order).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AF_TFM_HD __host__ __device__
#else
#define AF_TFM_HD
#endif

namespace af {

// receivers of one transmitter whose traces a workgroup owns (their time tile in LDS): the default;
// tfm_model.hip also instantiates 1 and 4, option "tfm_model_rx"
constexpr int kTfmModelRx = 2;
// bytes of LDS the time tiles of one workgroup may take (of 160 KiB per CU): two complex traces of
// 4096 samples
constexpr int kTfmModelLds = 128 * 1024;

struct TfmModelParams {
  const double* const* tx;  // [ntx] transmitter fields (row-major, one shape)
  const double* const* rx;  // [nrx] receiver fields, same shape
  const int64_t* pix;       // [npix] field offsets of the pixels that are not all zero, window raster order
  const double* refl;       // [npix][ncomp] their reflectivities
  const float* pair_w;      // [ntx][nrx] or nullptr (all 1)
  double* out;              // [ntx][nrx][nt][ncomp]
  double t0, fs;
  int64_t npix;
  int ntx, nrx, nt, ncomp;
  int rg;                   // receivers per workgroup: 1, 2 or 4
  int tile;                 // samples of a trace a workgroup holds per pass, 1 <= tile
  int slabs;                // pixel slabs per trace group, 1 <= slabs; > 1: out is zeroed, the flush adds
  int combine;              // a wave of at most this many runs of lanes sharing a sample sums each run before it adds (0: never)
};

// field offset of pixel (i, j) of the window (tfm_term.h tfm_pixel_offset)
AF_TFM_HD inline int64_t tfm_model_pixel_offset(int iz0, int ix0, int step, int fnx, int i, int j) {
  return ((int64_t)iz0 + (int64_t)step * i) * fnx + ((int64_t)ix0 + (int64_t)step * j);
}

// the samples a workgroup holds per pass: `want` (0: as many as fit), at most nt and what fits the
// LDS budget beside the other traces of the group
AF_TFM_HD inline int tfm_model_tile(int want, int nt, int ncomp, int rg) {
  const int fit = kTfmModelLds / (rg * ncomp * (int)sizeof(double));
  int t = want > 0 ? want : fit;
  if (t > fit) t = fit;
  if (t > nt) t = nt;
  return t;
}

// pixels [p0, p1) of slab s of `slabs`
AF_TFM_HD inline void tfm_model_slab(int64_t npix, int slabs, int s, int64_t& p0, int64_t& p1) {
  const int64_t per = (npix + slabs - 1) / slabs;
  p0 = per * s < npix ? per * s : npix;
  p1 = p0 + per < npix ? p0 + per : npix;
}

// the add of a term into sample k belongs to the time tile [lo, lo + len) that holds k: a term
// whose k is a tile's last sample leaves c0 in that tile and c1 in the next
AF_TFM_HD inline bool tfm_model_in_tile(int k, int lo, int len) { return (k >= lo) & (k - lo < len); }

// One term (a, b) at one pixel, split over the two samples it touches, for the tile [lo, lo + len)
// of the pair's trace: u = ((ta + tb) - t0) * fs; no term unless `live`, w != 0 and 0 <= u < nt - 1
// (NaN, +-inf and huge delays fail the test, which comes before the conversion to an integer; then
// 0 <= k <= nt - 2 < 2^31 and the conversion is exact); g = w * x[c], c1 = f * g, c0 = g - c1; c0
// goes to sample k (in0: this tile holds it), c1 to sample k + 1 (in1).  Written without branches,
// so that the unrolled receiver group issues all its field reads before it waits for the first.
// A term that does not count has k = -1 and in0 = in1 = false.
template <int NC>
struct TfmModelSplit {
  int k;
  bool in0, in1;
  double c0[NC], c1[NC];
};

template <int NC>
AF_TFM_HD inline TfmModelSplit<NC> tfm_model_split(double ta, double tb, double w, bool live, const double* x, int nt,
                                                   double t0, double fs, int lo, int len) {
  TfmModelSplit<NC> s;
  const double u = ((ta + tb) - t0) * fs;
  const bool ok = live & (w != 0.0) & (u >= 0.0) & (u < (double)(nt - 1));
  const int k = (int)(ok ? u : 0.0);
  const double f = (ok ? u : 0.0) - (double)k;
  s.k = ok ? k : -1;
  s.in0 = ok & tfm_model_in_tile(k, lo, len);
  s.in1 = ok & tfm_model_in_tile(k + 1, lo, len);
#pragma unroll
  for (int c = 0; c < NC; c++) {
    const double g = w * x[c];
    s.c1[c] = f * g;
    s.c0[c] = g - s.c1[c];
  }
  return s;
}

// the two adds of a split term into tile[len][NC]; only the adds themselves are predicated (an add
// of 0.0 to a dummy sample would cost an LDS atomic, the resource the kernel is bound by).
// add(p, v): *p += v, atomically on the device.
template <int NC, class Add>
AF_TFM_HD inline void tfm_model_add(const TfmModelSplit<NC>& s, int lo, double* tile, Add add) {
  double* p = tile + (int64_t)(s.k - lo) * NC;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    if (s.in0) add(p + c, s.c0[c]);
    if (s.in1) add(p + NC + c, s.c1[c]);
  }
}

// Pixel q (of P.pix / P.refl; `valid`: q is a pixel of the slab, else nothing counts and pixel
// `safe` is read instead) for transmitter a and receivers b0 .. b0 + RG - 1: one T_a read, RG T_b
// reads, RG terms, each handed to sink(r, split) (tile + r * len * NC is receiver b0 + r's).
template <int NC, int RG, class Sink>
AF_TFM_HD inline void tfm_model_pixel(const TfmModelParams& P, int a, int b0, int64_t q, bool valid, int64_t safe, int lo,
                                      int len, Sink sink) {
  q = valid ? q : safe;
  const int64_t off = P.pix[q];
  double x[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) x[c] = P.refl[q * NC + c];
  const double ta = P.tx[a][off];
  double tb[RG], w[RG];
#pragma unroll
  for (int r = 0; r < RG; r++) {
    const bool live = b0 + r < P.nrx;  // past the last receiver: the group's first pair, not counted
    const int b = b0 + (live ? r : 0);
    tb[r] = P.rx[b][off];
    w[r] = P.pair_w ? (double)P.pair_w[(int64_t)a * P.nrx + b] : 1.0;
  }
#pragma unroll
  for (int r = 0; r < RG; r++)
    sink(r, tfm_model_split<NC>(ta, tb[r], w[r], valid & (b0 + r < P.nrx), x, P.nt, P.t0, P.fs, lo, len));
}

}  // namespace af
