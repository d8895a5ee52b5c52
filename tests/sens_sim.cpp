// Stand-alone host run of the sensitivity kernels' per-segment code (csrc/sens_walk.h: the guarded
// piece count, the walk, the entry arithmetic; csrc/tbp_walk.h: time_between_points()'s walk), built
// with ASan and UBSan by tests/test_sens_ref.py, so the guards (non-finite and huge coordinates,
// cells outside the grid, segments whose walk never ends) are checked on a CPU before the kernels
// (ray_sens.hip, which call the very same functions) run on a GPU.  The group velocity is
// device_common.h's arithmetic with the C library's trigonometry.  Test infrastructure only.
//   sens_sim INPUT OUTPUT   INPUT: the file of tests/sens_ref.py write_sim_input(); OUTPUT: int64
//   nrays, row_ptr int64 [nrays + 1], status int32 [nrays], col int32, len, time, dth float64
//   [row_ptr[nrays]].  Exit status 0, or 2 on a malformed input.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#define AF_DEV inline
#define AF_ATAN atan
#include "sens_walk.h"

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static bool wr(FILE* f, const std::vector<T>& v) {
  return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

// device_common.h table_vel / christoffel_group (the stiffness as exact doubles)
static double table_vel(const double* tab, int ncol, double eff, int col, double vm) {
  long a1 = (long)floor(eff);
  long a2 = (a1 + 1) % 180;
  double rem = eff - (double)a1;
  return vm * ((1 - rem) * tab[a1 * ncol + col] + rem * tab[a2 * ncol + col]);
}
static double christoffel_group(const double* s, double eff, double vm) {
  using af::pymod;
  double sigma = s[4];
  double e90 = pymod(eff, 90);
  if (e90 < 0.01 || e90 > 90 - 0.01) {
    double lam = (fabs(pymod(eff, 180) - 90) < 1) ? s[2] : s[0];
    return 1000 * vm * sqrt(lam / sigma);
  }
  double c22 = s[0], c23 = s[1], c33 = s[2], c44 = s[3];
  double tan_ang = tan(eff * af::kDeg2Rad);
  double A = c22 + c33 - 2 * c44;
  double B = (c23 + c44) * (tan_ang - 1 / tan_ang);
  double C = c22 - c33;
  double disc = B * B + A * A - C * C;
  double pa;
  if (eff < 90) pa = pymod(atan((-B - sqrt(disc)) / (C - A)), M_PI);
  else pa = pymod(atan((-B + sqrt(disc)) / (C - A)), M_PI);
  double lam = 0.5 * (cos(2 * pa) * (c22 - c44) + sin(2 * pa) * (c23 + c44) * tan_ang + c22 + c44);
  return 1000 * vm * sqrt(lam / sigma) / cos(eff * af::kDeg2Rad - pa);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int64_t> h, velpn, stif;
  std::vector<double> dn, veln, vm, gtab, xy;
  std::vector<int32_t> lens, flags;
  if (!rd(f, h, 8) || !rd(f, dn, 1)) return 2;
  const int64_t nz0 = h[0], nx0 = h[1], ncol = h[2], have_stif = h[3], sg = h[4], nrays = h[5], npts = h[6];
  if (nz0 < 1 || nx0 < 1 || nz0 * nx0 > (1 << 24) || ncol < 1 || ncol > 64 || sg < 1 || nrays < 0 || npts < 0) return 2;
  const size_t nc = (size_t)(nz0 * nx0);
  if (!rd(f, veln, nc) || !rd(f, velpn, nc) || !rd(f, vm, nc) || !rd(f, stif, have_stif ? 5 * nc : 0) ||
      !rd(f, gtab, (size_t)(361 * ncol)) || !rd(f, lens, (size_t)nrays) || !rd(f, flags, h[7] ? (size_t)nrays : 0) ||
      !rd(f, xy, (size_t)(2 * npts)))
    return 2;
  fclose(f);
  for (size_t c = 0; c < nc; c++)
    if (velpn[c] < 0 || velpn[c] >= ncol) return 2;
  int64_t sum = 0;
  for (int32_t l : lens) sum += l > 0 ? l : 0;
  if (sum != npts) return 2;
  const double dnx = dn[0];
  std::vector<int64_t> row_ptr((size_t)nrays + 1, 0);
  std::vector<int32_t> status((size_t)nrays, 0), col;
  std::vector<double> elen, etime, edth;
  int64_t off = 0;
  for (int64_t k = 0; k < nrays; k++) {
    const int n = lens[k] > 0 ? lens[k] : 0;
    const double* p = xy.data() + 2 * off;
    off += n;
    row_ptr[k + 1] = row_ptr[k];
    if (n < 2 || (h[7] && (flags[k] & 6))) continue;
    // the count pass: every segment of the ray
    std::vector<int> cnt((size_t)n - 1);
    bool bad = false;
    for (int s = 0; s < n - 1 && !bad; s++) {
      cnt[s] = af::sens_count(p[2 * s], p[2 * s + 2], p[2 * s + 1], p[2 * s + 3], (int)sg, (int)nz0, (int)nx0);
      bad = cnt[s] < 0;
    }
    if (bad) {
      status[k] = 1;
      continue;
    }
    // the fill pass
    for (int s = 0; s < n - 1; s++) {
      af::SensWalk W;
      W.start(p[2 * s], p[2 * s + 2], p[2 * s + 1], p[2 * s + 3], (int)sg);
      for (int j = 0; j < cnt[s] && W.more(); j++) {
        int y, x;
        double len;
        if (!W.next((int)nz0, (int)nx0, dnx, y, x, len)) return 3;  // sens_count() accepted the segment
        const size_t c = (size_t)y * nx0 + x;
        double srow[5];
        const bool christoffel = velpn[c] == 0 && have_stif;
        if (christoffel)
          for (int q = 0; q < 5; q++) srow[q] = (double)stif[5 * c + q];
        double sl, ds;
        af::sens_slowness(
            veln[c], W.angle, christoffel,
            [&](double eff) {
              return christoffel ? christoffel_group(srow, eff, vm[c])
                                 : table_vel(gtab.data(), (int)ncol, eff, (int)velpn[c], vm[c]);
            },
            sl, ds);
        col.push_back((int32_t)c);
        elen.push_back(len);
        etime.push_back(len * sl);
        edth.push_back(len * ds);
        row_ptr[k + 1]++;
      }
      if (W.more()) return 3;  // the walk ends with the counted pieces
    }
  }
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 2;
  std::vector<int64_t> head{nrays};
  if (!wr(g, head) || !wr(g, row_ptr) || !wr(g, status) || !wr(g, col) || !wr(g, elen) || !wr(g, etime) || !wr(g, edth))
    return 2;
  fclose(g);
  return 0;
}
