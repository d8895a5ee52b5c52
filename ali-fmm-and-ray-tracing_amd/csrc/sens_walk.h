// sens_walk.h — travel-time sensitivities along a ray segment (include/alifmm.h alifmm_ray_sens):
// the guarded count of a segment's pieces, the walk that yields each piece's cell and length, and
// the arithmetic of an entry.  Shared verbatim by the kernels (ray_sens.hip) and by a stand-alone
// host program (tests/sens_sim.cpp, built with ASan and UBSan), so the guards are checked on a CPU
// before a kernel runs.  Includes nothing from HIP; the includer defines AF_DEV and AF_ATAN
// (tbp_walk.h); build with -ffp-contract=off.
#pragma once
#include <float.h>

#include "tbp_walk.h"

namespace af {

// the centred difference of the slowness in the orientation: h = 2^-10 degree, 1 / (2 h) = 512
constexpr double kSensH = 1.0 / 1024.0;
constexpr double kSensInv2H = 512.0;

// finite: NaN and +-inf fail
AF_DEV bool sens_finite(double v) { return fabs(v) <= DBL_MAX; }

// The coarse cell of the piece that ends at (nxv, nyv), as TbpWalk::cell (midpoint, rounded,
// negative indices wrapped once), with the range test made in double before any conversion to an
// integer (NaN, +-inf and huge values fail it).  False: the cell lies outside the grid.
AF_DEV bool sens_cell(const TbpWalk& w, double nxv, double nyv, int nz0, int nx0, int& y_pos, int& x_pos) {
  const double mx = rint((w.prev_x + nxv) / 2), my = rint((w.prev_y + nyv) / 2);
  if (!(mx >= -(double)nx0 && mx < (double)nx0 && my >= -(double)nz0 && my < (double)nz0)) return false;
  x_pos = (int)mx;
  y_pos = (int)my;
  if (x_pos < 0) x_pos += nx0;
  if (y_pos < 0) y_pos += nz0;
  return true;
}

// Pieces of the segment (x1, y1) -> (x2, y2) (fine-grid coordinates of subgrid sg) on an nz0 x nx0
// coarse grid, or -1 when the segment is invalid: a coordinate is not finite, a piece's cell lies
// outside the grid, or the walk is unfinished after B = floor|x2 - x1| + floor|y2 - y1| + 4 pieces
// (coordinates after the division by sg).  No finite walk needs more than B pieces; a horizontal
// segment at z = k + 0.5, k odd, never sets fin_y (a vertical one at x = k + 0.5 never fin_x) and
// would walk without end.  Ends on any input:
// every piece passes sens_cell, and a walk whose cells all lie in the grid crosses at most
// 2 (nz0 + nx0) cell edges, so B is also capped at 4 (nz0 + nx0) + 8 (which no valid walk reaches).
AF_DEV int sens_count(double x1, double x2, double y1, double y2, int sg, int nz0, int nx0) {
  if (!(sens_finite(x1) && sens_finite(x2) && sens_finite(y1) && sens_finite(y2))) return -1;
  TbpWalk w;
  double angle;
  w.setup(x1, x2, y1, y2, sg, angle);
  double bound = floor(fabs(w.end_x - w.start_x)) + floor(fabs(w.end_y - w.start_y)) + 4.0;
  const double cap = 4.0 * ((double)nz0 + (double)nx0) + 8.0;
  if (!(bound < cap)) bound = cap;
  w.begin();
  int n = 0;
  while (!w.done()) {
    if (!((double)n < bound)) return -1;
    double nxv, nyv;
    w.piece(nxv, nyv);
    int y_pos, x_pos;
    if (!sens_cell(w, nxv, nyv, nz0, nx0, y_pos, x_pos)) return -1;
    w.prev_x = nxv;
    w.prev_y = nyv;
    n++;
  }
  return n;
}

// The pieces of a segment sens_count() accepted, in walk order.
struct SensWalk {
  TbpWalk w;
  double angle;  // the segment's direction [deg] (TbpWalk::setup)
  AF_DEV void start(double x1, double x2, double y1, double y2, int sg) {
    w.setup(x1, x2, y1, y2, sg, angle);
    w.begin();
  }
  AF_DEV bool more() const { return !w.done(); }
  // the next piece: its cell and its length piece_dist [m]; false (nothing yielded) if its cell lies
  // outside the grid, which sens_count() has excluded
  AF_DEV bool next(int nz0, int nx0, double dnx, int& y_pos, int& x_pos, double& len) {
    double nxv, nyv;
    w.piece(nxv, nyv);
    if (!sens_cell(w, nxv, nyv, nz0, nx0, y_pos, x_pos)) return false;
    len = w.piece_dist(nxv, nyv, dnx);
    w.prev_x = nxv;
    w.prev_y = nyv;
    return true;
  }
};

// the reference's on-axis snap of the Christoffel group velocity (christoffel_group, :294-297)
AF_DEV bool sens_snap(double eff) {
  const double e90 = pymod(eff, 90);
  return e90 < 0.01 || e90 > 90 - 0.01;
}

// Slowness s and its derivative ds [s/m per degree of veln] of a cell of orientation veln along a
// segment at `angle`: vel(e) is the cell's group velocity at effective angle e (group_vel_cell),
// christoffel: the cell takes the closed form (velpn == 0 and a stiffness row).
//   eff = pymod(veln - angle, 180), s = 1 / vel(eff)
//   ds = (1 / vel(pymod(eff + h, 180)) - 1 / vel(pymod(eff - h, 180))) * 512, h = 2^-10 degree;
//   0 for a Christoffel cell inside the snap
template <class Vel>
AF_DEV void sens_slowness(double veln, double angle, bool christoffel, const Vel& vel, double& s, double& ds) {
  const double eff = pymod(veln - angle, 180);
  s = 1.0 / vel(eff);
  if (christoffel && sens_snap(eff)) {
    ds = 0.0;
    return;
  }
  const double sp = 1.0 / vel(pymod(eff + kSensH, 180));
  const double sm = 1.0 / vel(pymod(eff - kSensH, 180));
  ds = (sp - sm) * kSensInv2H;
}

}  // namespace af
