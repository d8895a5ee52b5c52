// init_sig.h — the material window of a source-init signature (fmm_shared.h InitSig): which cells
// of the model fmm_init_kernel's walk can read for a source, and the order they are recorded in.
// The three stage windows reach 2, 6 and 13 coarse cells from the source and the exact prefix
// window max(exact_r + 6, 16) (fmm_init.hip), each clipped at the grid's edges; update() and
// fouds18_A() read the material at their target cell only, so the prefix window's reach, taken
// for every exact_r (0 included), covers every cell the walk reads.  Shared verbatim by the
// kernel and by a stand-alone host program (tests/init_sig_sim.cpp, built with ASan and UBSan).
// Includes nothing from HIP; the includer defines AF_DEV.
#pragma once

namespace af {

// reach [cells] of the window around the source (fmm_init.hip: the prefix window's W)
AF_DEV int init_sig_reach(int exact_r) { return exact_r + 6 > 16 ? exact_r + 6 : 16; }

// largest reach a signature has room for: exact_r <= 48 (alifmm_set_option), a 109 x 109 window
constexpr int kInitSigMaxReach = 54;
constexpr int kInitSigMaxCells = (2 * kInitSigMaxReach + 1) * (2 * kInitSigMaxReach + 1);

// rows z0..z1, columns x0..x1 of the nz0 x nx0 grid (inclusive; never empty for a source on the
// grid), w columns per row, n cells
struct InitSigWin {
  int z0, x0, z1, x1, w, n;
};

// The window of source (isz, isx), 0 <= isz < nz0, 0 <= isx < nx0.  n == 0: no window (a source
// off the grid or a reach the signature has no room for); such a source is never reused.
AF_DEV InitSigWin init_sig_window(long isz, long isx, int exact_r, int nz0, int nx0) {
  InitSigWin w{0, 0, -1, -1, 0, 0};
  if (exact_r < 0 || nz0 < 1 || nx0 < 1 || isz < 0 || isz >= nz0 || isx < 0 || isx >= nx0) return w;
  const int r = init_sig_reach(exact_r);
  if (r > kInitSigMaxReach) return w;
  w.z0 = (int)(isz - r > 0 ? isz - r : 0);
  w.x0 = (int)(isx - r > 0 ? isx - r : 0);
  w.z1 = (int)(isz + r < (long)nz0 - 1 ? isz + r : (long)nz0 - 1);
  w.x1 = (int)(isx + r < (long)nx0 - 1 ? isx + r : (long)nx0 - 1);
  w.w = w.x1 - w.x0 + 1;
  w.n = (w.z1 - w.z0 + 1) * w.w;
  return w;
}

// cell k (0 <= k < n, row-major over the window) as a flat index of the nz0 x nx0 grid
AF_DEV long init_sig_cell(const InitSigWin& w, int k, int nx0) {
  return (long)(w.z0 + k / w.w) * nx0 + (w.x0 + k % w.w);
}

}  // namespace af
