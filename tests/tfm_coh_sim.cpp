// Stand-alone host run of the coherence-weighted TFM kernel's per-pixel code (csrc/tfm_coh_term.h:
// the term with its extra sums, the loop over pairs, the factor), built with UBSan by
// tests/test_tfm_coh_ref.py, so that code is checked on a CPU before the kernel (tfm_coh.hip, which
// calls the very same functions) runs on a GPU.  Test infrastructure only.
//   tfm_coh_sim INPUT OUTPUT KIND [CHUNK]   INPUT: the file of tests/tfm_ref.py write_sim_input();
//   KIND 1, 2 or 3; CHUNK 4, 8 (default), 16 or 32.  OUTPUT: raw float64, the image
//   [niz][nix][ncomp], then the factor [niz][nix], then the sums [niz][nix][3].
//   Exit status 0, or 2 on a malformed input.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tfm_coh_term.h"

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

struct Out {
  double *image, *factor, *sums;
};

template <int NC, int RC, int KIND>
static void run(const af::TfmParams& P, const Out& o) {
  for (int i = 0; i < P.niz; i++)
    for (int j = 0; j < P.nix; j++) {
      af::TfmCohAcc<NC> A;
      af::tfm_coh_pixel<NC, RC, KIND>(P, af::tfm_pixel_offset(P, i, j), A);
      const int64_t pix = (int64_t)i * P.nix + j;
      for (int c = 0; c < NC; c++) o.image[pix * NC + c] = A.s[c];
      o.factor[pix] = af::tfm_coh_factor<NC, KIND>(A);
      o.sums[pix * 3] = A.n, o.sums[pix * 3 + 1] = A.x[0], o.sums[pix * 3 + 2] = A.x[1];
    }
}

template <int NC, int KIND>
static void run_chunk(const af::TfmParams& P, const Out& o, int chunk) {
  if (chunk == 4) run<NC, 4, KIND>(P, o);
  else if (chunk == 16) run<NC, 16, KIND>(P, o);
  else if (chunk == 32) run<NC, 32, KIND>(P, o);
  else run<NC, af::kTfmChunk, KIND>(P, o);
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int kind = atoi(argv[3]), chunk = argc > 4 ? atoi(argv[4]) : af::kTfmChunk;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int64_t> h;
  std::vector<double> tf, fld;
  std::vector<int32_t> tx, rx;
  std::vector<float> fmc, w;
  if (!rd(f, h, 16) || !rd(f, tf, 2)) return 2;
  const int64_t ntx = h[0], nrx = h[1], nt = h[2], nc = h[3], nfld = h[4], fnz = h[5], fnx = h[6];
  if (ntx < 1 || nrx < 1 || nt < 2 || (nc != 1 && nc != 2) || nfld < 1 || fnz < 1 || fnx < 1) return 2;
  if (kind < 1 || kind > 3 || (kind == 3 && nc != 2)) return 2;
  if (!rd(f, tx, ntx) || !rd(f, rx, nrx) || !rd(f, fld, (size_t)(nfld * fnz * fnx)) ||
      !rd(f, fmc, (size_t)(ntx * nrx * nt * nc)) || !rd(f, w, h[12] ? (size_t)(ntx * nrx) : 0))
    return 2;
  fclose(f);
  af::TfmParams P;
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
  const size_t npix = (size_t)P.niz * P.nix;
  std::vector<double> out(npix * (nc + 4));
  const Out o = {out.data(), out.data() + npix * nc, out.data() + npix * (nc + 1)};
  P.tx = tab.data();
  P.rx = tab.data() + ntx;
  P.fmc = fmc.data();
  P.pair_w = h[12] ? w.data() : nullptr;
  P.image = o.image;
  P.t0 = tf[0], P.fs = tf[1];
  P.ntx = (int)ntx, P.nrx = (int)nrx, P.nt = (int)nt, P.ncomp = (int)nc, P.fnx = (int)fnx;
  if (nc == 2) {
    if (kind == 1) run_chunk<2, 1>(P, o, chunk);
    else if (kind == 2) run_chunk<2, 2>(P, o, chunk);
    else run_chunk<2, 3>(P, o, chunk);
  } else {
    if (kind == 1) run_chunk<1, 1>(P, o, chunk);
    else run_chunk<1, 2>(P, o, chunk);
  }
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) return 2;
  fclose(g);
  return 0;
}
