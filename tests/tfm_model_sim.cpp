// Stand-alone host run of the FMC modelling kernel's code (csrc/tfm_model_term.h: the range test,
// the integer conversion, the time-tile membership of a term's two adds, the pass of a receiver
// group over the pixels), built with UBSan by tests/test_tfm_model_ref.py, so that code is checked
// on a CPU before the kernel (tfm_model.hip, which calls the very same functions) runs on a GPU.
// The loop over trace groups, time tiles and pixels and the flush are the kernel's, one "thread".
// Test infrastructure only.
//   tfm_model_sim INPUT OUTPUT   INPUT: the file of tests/tfm_model_ref.py write_sim_input();
//   OUTPUT: the data, raw float64 [ntx][nrx][nt][ncomp].  Exit status 0, or 2 on a malformed input.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tfm_model_term.h"

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <int NC>
static void run(const af::TfmModelParams& P) {
  constexpr int RG = af::kTfmModelRx;
  std::vector<double> tile((size_t)RG * P.tile * NC);
  auto add = [&](double* p, double v) {
    if (p < tile.data() || p >= tile.data() + tile.size()) __builtin_trap();  // an add outside the tile
    *p += v;
  };
  for (int a = 0; a < P.ntx; a++)
    for (int b0 = 0; b0 < P.nrx; b0 += RG)
      for (int lo = 0; lo < P.nt; lo += P.tile) {
        const int len = P.nt - lo < P.tile ? P.nt - lo : P.tile;
        const int per = len * NC, n = RG * per;
        for (int i = 0; i < n; i++) tile[i] = 0.0;
        for (int64_t q = 0; q < P.npix; q++)
          af::tfm_model_pixel<NC, RG>(P, a, b0, q, true, 0, lo, len, [&](int r, const af::TfmModelSplit<NC>& s) {
            af::tfm_model_add<NC>(s, lo, tile.data() + (int64_t)r * len * NC, add);
          });
        for (int i = 0; i < n; i++) {
          const int r = i / per, rem = i - r * per;
          if (b0 + r >= P.nrx) break;
          P.out[(((int64_t)a * P.nrx + (b0 + r)) * P.nt + lo) * NC + rem] = tile[i];
        }
      }
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int64_t> h;
  std::vector<double> tf, fld, refl;
  std::vector<int32_t> tx, rx;
  std::vector<float> w;
  if (!rd(f, h, 16) || !rd(f, tf, 2)) return 2;
  const int64_t ntx = h[0], nrx = h[1], nt = h[2], nc = h[3], nfld = h[4], fnz = h[5], fnx = h[6];
  const int64_t iz0 = h[7], ix0 = h[8], niz = h[9], nix = h[10], step = h[11];
  if (ntx < 1 || nrx < 1 || nt < 2 || nt > 0x7fffffff || (nc != 1 && nc != 2) || nfld < 1 || fnz < 1 || fnx < 1) return 2;
  if (step < 1 || niz < 1 || nix < 1 || iz0 < 0 || ix0 < 0 || iz0 + step * (niz - 1) >= fnz || ix0 + step * (nix - 1) >= fnx)
    return 2;
  if (h[13] < 0 || h[13] > 0x7fffffff) return 2;
  if (!rd(f, tx, ntx) || !rd(f, rx, nrx) || !rd(f, fld, (size_t)(nfld * fnz * fnx)) ||
      !rd(f, refl, (size_t)(niz * nix * nc)) || !rd(f, w, h[12] ? (size_t)(ntx * nrx) : 0))
    return 2;
  fclose(f);
  std::vector<const double*> tab;
  for (int64_t k = 0; k < ntx + nrx; k++) {
    const int32_t s = k < ntx ? tx[k] : rx[k - ntx];
    if (s < 0 || s >= nfld) return 2;
    tab.push_back(fld.data() + (size_t)s * fnz * fnx);
  }
  // the pixels that are not all zero, as alifmm_tfm_model() lists them
  std::vector<int64_t> pix;
  std::vector<double> val;
  for (int i = 0; i < niz; i++)
    for (int j = 0; j < nix; j++) {
      const double* x = refl.data() + ((int64_t)i * nix + j) * nc;
      bool any = false;
      for (int c = 0; c < nc; c++) any |= x[c] != 0.0;
      if (!any) continue;
      pix.push_back(af::tfm_model_pixel_offset((int)iz0, (int)ix0, (int)step, (int)fnx, i, j));
      for (int c = 0; c < nc; c++) val.push_back(x[c]);
    }
  std::vector<double> out((size_t)(ntx * nrx * nt * nc));
  af::TfmModelParams P;
  P.tx = tab.data();
  P.rx = tab.data() + ntx;
  P.pix = pix.data();
  P.refl = val.data();
  P.pair_w = h[12] ? w.data() : nullptr;
  P.out = out.data();
  P.t0 = tf[0], P.fs = tf[1];
  P.npix = (int64_t)pix.size();
  P.ntx = (int)ntx, P.nrx = (int)nrx, P.nt = (int)nt, P.ncomp = (int)nc;
  P.rg = af::kTfmModelRx;
  P.tile = af::tfm_model_tile((int)h[13], (int)nt, (int)nc, P.rg);
  P.slabs = 1;
  P.combine = 0;
  if (nc == 2) run<2>(P);
  else run<1>(P);
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) return 2;
  fclose(g);
  printf("tile %d\n", P.tile);
  return 0;
}
