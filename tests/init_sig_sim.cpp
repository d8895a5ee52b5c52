// init_sig_sim.cpp — host run of the signature window of the source-init kernel (csrc/init_sig.h),
// built with ASan and UBSan by tests/test_init_sig.py: the window and cell arithmetic the kernel
// indexes the model and the signature with, checked on a CPU before a kernel runs.
//
//   init_sig_sim      exits 0 when every case holds, else prints the first failure and exits 1
//
// Each case marks the cells the window yields in an nz0 x nx0 array (so an index out of range is
// an ASan report, not only a failed comparison) and checks them against the clipped rectangle
// written out independently: every cell of [isz - W, isz + W] x [isx - W, isx + W] that lies on
// the grid, once, in row-major order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#define AF_DEV inline
#include "init_sig.h"

static int g_cases = 0;

static bool run_case(int nz0, int nx0, long isz, long isx, int exact_r) {
  g_cases++;
  const af::InitSigWin w = af::init_sig_window(isz, isx, exact_r, nz0, nx0);
  const int W = exact_r + 6 > 16 ? exact_r + 6 : 16;
  // the clipped rectangle, cell by cell
  std::vector<long> want;
  for (long z = isz - W; z <= isz + W; z++)
    for (long x = isx - W; x <= isx + W; x++)
      if (z >= 0 && z < nz0 && x >= 0 && x < nx0) want.push_back(z * nx0 + x);
  auto bad = [&](const char* what, long a, long b) {
    std::printf("FAIL %s: grid %d x %d source (%ld, %ld) exact_r %d: %ld vs %ld\n", what, nz0, nx0, isz, isx, exact_r,
                a, b);
    return false;
  };
  if (w.n != (int)want.size()) return bad("cell count", w.n, (long)want.size());
  if (w.n <= 0 || w.n > af::kInitSigMaxCells) return bad("count range", w.n, af::kInitSigMaxCells);
  if (w.z0 < 0 || w.x0 < 0 || w.z1 >= nz0 || w.x1 >= nx0 || w.z0 > w.z1 || w.x0 > w.x1)
    return bad("window bounds", w.z0, w.x0);
  if (!(w.z0 <= isz && isz <= w.z1 && w.x0 <= isx && isx <= w.x1)) return bad("source outside", isz, isx);
  std::vector<unsigned char> hit((size_t)nz0 * nx0, 0);
  std::vector<long> got((size_t)w.n);
  for (int k = 0; k < w.n; k++) {
    const long c = af::init_sig_cell(w, k, nx0);
    if (c < 0 || c >= (long)nz0 * nx0) return bad("index range", c, (long)nz0 * nx0);
    if (hit[(size_t)c]++) return bad("cell twice", c, k);
    got[(size_t)k] = c;
    if (c != want[(size_t)k]) return bad("order", c, want[(size_t)k]);
  }
  // deterministic: a second pass, last cell first, yields the same cell for the same k
  for (int k = w.n - 1; k >= 0; k--)
    if (af::init_sig_cell(af::init_sig_window(isz, isx, exact_r, nz0, nx0), k, nx0) != got[(size_t)k])
      return bad("second pass", k, got[(size_t)k]);
  return true;
}

int main() {
  const int grids[][2] = {{64, 160}, {7, 40}, {40, 7}, {20, 20}, {2, 2}, {109, 109}, {300, 130}};
  const int rs[] = {0, 20, 48};
  bool ok = true;
  for (const auto& g : grids) {
    const int nz = g[0], nx = g[1];
    const long zs[] = {0, 1, nz / 2, nz - 2 < 0 ? 0 : nz - 2, nz - 1};
    const long xs[] = {0, 1, nx / 2, nx - 2 < 0 ? 0 : nx - 2, nx - 1};
    for (int r : rs)
      for (long z : zs)      // the four corners, a source on each edge, the interior, and one node
        for (long x : xs)    // inside each edge
          ok = ok && run_case(nz, nx, z, x, r);
    // a source exactly the reach away from each edge: the window touches the edge without clipping
    for (int r : rs) {
      const int W = af::init_sig_reach(r);
      if (W < nz && W < nx) ok = ok && run_case(nz, nx, W, W, r) && run_case(nz, nx, nz - 1 - W, nx - 1 - W, r);
    }
  }
  // no window: a source off the grid, a reach past the signature's room
  const af::InitSigWin off[] = {af::init_sig_window(-1, 0, 20, 64, 160), af::init_sig_window(0, 160, 20, 64, 160),
                                af::init_sig_window(64, 0, 20, 64, 160), af::init_sig_window(3, 3, 49, 64, 160),
                                af::init_sig_window(3, 3, -1, 64, 160)};
  for (const auto& w : off)
    if (w.n != 0) {
      std::printf("FAIL no-window case has %d cells\n", w.n);
      ok = false;
    }
  if (!ok) return 1;
  std::printf("ok %d cases\n", g_cases);
  return 0;
}
