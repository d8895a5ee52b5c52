// Stand-alone host run of the TFM kernel's per-pixel code (csrc/tfm_term.h: the range test, the
// integer conversion, the 64-bit data offsets, the loop over pairs), built with UBSan by
// tests/test_tfm_ref.py, so that code is checked on a CPU before the kernel (tfm.hip, which calls
// the very same functions) runs on a GPU.  Test infrastructure only.
//   tfm_sim INPUT OUTPUT   INPUT: the file of tests/tfm_ref.py write_sim_input(); OUTPUT: the
//   image, raw float64 [niz][nix][ncomp].  Exit status 0, or 2 on a malformed input.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tfm_term.h"

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int64_t> h;
  std::vector<double> tf, fld;
  std::vector<int32_t> tx, rx;
  std::vector<float> fmc, w;
  if (!rd(f, h, 16) || !rd(f, tf, 2)) return 2;
  const int64_t ntx = h[0], nrx = h[1], nt = h[2], nc = h[3], nfld = h[4], fnz = h[5], fnx = h[6];
  if (ntx < 1 || nrx < 1 || nt < 2 || (nc != 1 && nc != 2) || nfld < 1 || fnz < 1 || fnx < 1) return 2;
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
  std::vector<double> img((size_t)P.niz * P.nix * nc);
  P.tx = tab.data();
  P.rx = tab.data() + ntx;
  P.fmc = fmc.data();
  P.pair_w = h[12] ? w.data() : nullptr;
  P.image = img.data();
  P.t0 = tf[0], P.fs = tf[1];
  P.ntx = (int)ntx, P.nrx = (int)nrx, P.nt = (int)nt, P.ncomp = (int)nc, P.fnx = (int)fnx;
  for (int i = 0; i < P.niz; i++)
    for (int j = 0; j < P.nix; j++) {
      double* o = P.image + ((int64_t)i * P.nix + j) * nc;
      if (nc == 2) af::tfm_pixel<2, af::kTfmChunk>(P, af::tfm_pixel_offset(P, i, j), o);
      else af::tfm_pixel<1, af::kTfmChunk>(P, af::tfm_pixel_offset(P, i, j), o);
    }
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(img.data(), sizeof(double), img.size(), g) != img.size()) return 2;
  fclose(g);
  return 0;
}
