// tbp_walk.h — the plain arithmetic of time_between_points()'s walk (Anis_TTF_rays.py:2835-2989):
// Python's float '%' and round(), and the walk over a segment's pieces.  Includes nothing from HIP,
// so the kernels (through device_common.h) and stand-alone host programs (tests/sens_sim.cpp) compile
// the very same code.  The includer defines AF_DEV (the function qualifier) and AF_ATAN (the
// arctangent: cr_math.h's correctly rounded one on the device) first; build with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

namespace af {

constexpr double kDeg2Rad = M_PI / 180.0;
constexpr double kRad2Deg = 180.0 / M_PI;

// Python float '%' (CPython float_divmod; numba real_divmod_func_body).
// Fast paths for |a| < 2b (every call site: angles mod 180/90/pi) give the same bits as the
// generic fmod route: fmod(a, b) is exact, and a -/+ b is exact there by Sterbenz's lemma; the
// only rounding is the final '+ b' of negative remainders, which the reference performs too.
AF_DEV double pymod(double a, double b) {
  if (b > 0) {
    if (a >= 0 && a < b) return a == 0 ? 0.0 : a;  // -0.0 -> +0.0 as copysign(0, b)
    if (a >= b && a < 2 * b) return a - b;
    if (a < 0 && a >= -b) return a + b;            // a == -b: fmod gives -0.0 -> +0.0, as here
    if (a < -b && a > -2 * b) return (a + b) + b;
  }
  double m = fmod(a, b);
  if (m != 0.0) {
    if ((b < 0) != (m < 0)) m += b;
  } else {
    m = copysign(0.0, b);
  }
  return m;
}
// round(): half-even (numba lowers to llvm.rint).
AF_DEV long pyround(double x) { return (long)rint(x); }
// the same for values known to fit in int (grid coordinates): two instructions instead of the
// 64-bit conversion's sequence
AF_DEV int pyround_i(double x) { return (int)rint(x); }

// time_between_points :2835-2989 (coarse material, numba negative-index wrap)
// The walk over the segment's pieces (crossings of the half-integer cell edges): the geometry of
// piece k does not depend on the material, only the slowness does.
struct TbpWalk {
  double start_x, start_y, end_x, end_y, mm, cc;
  double next_x, next_y, prev_x, prev_y;
  int dir_x, dir_y;
  bool fin_x, fin_y;
  // the segment (x1, y1) -> (x2, y2) in subgrid-sg coordinates; *angle: its direction [deg]
  AF_DEV void setup(double x1, double x2, double y1, double y2, int sg, double& angle) {
    if (sg != 1) {  // (x / 1.0 is x)
      x1 = x1 / (double)sg;
      x2 = x2 / (double)sg;
      y1 = y1 / (double)sg;
      y2 = y2 / (double)sg;
    }
    start_x = x1;
    end_x = x2;
    start_y = y1;
    end_y = y2;
    angle = (x1 == x2) ? 0.0 : AF_ATAN((y2 - y1) / (x2 - x1)) * kRad2Deg;
    mm = 0;
    cc = 0;
    if (end_x != start_x) {
      mm = (end_y - start_y) / (end_x - start_x);
      cc = start_y - mm * start_x;
    }
    dir_x = (start_x < end_x) ? 1 : -1;
    dir_y = (start_y < end_y) ? 1 : -1;
  }
  AF_DEV void begin() {
    fin_x = fin_y = false;
    next_x = rint(start_x) + dir_x * 0.5;  // (double)pyround(x) is rint(x)
    next_y = rint(start_y) + dir_y * 0.5;
    prev_x = start_x;
    prev_y = start_y;
  }
  AF_DEV bool done() const { return fin_x && fin_y; }
  // the next piece's end point (nxv, nyv); the piece runs from (prev_x, prev_y)
  AF_DEV void piece(double& nxv, double& nyv) {
    if (((next_x > end_x && dir_x == 1) || (next_x < end_x && dir_x == -1)) && !fin_x) {
      fin_x = true;
      next_x = end_x;
    }
    if (((next_y > end_y && dir_y == 1) || (next_y < end_y && dir_y == -1)) && !fin_y) {
      fin_y = true;
      next_y = end_y;
    }
    if (end_x == start_x) {
      nxv = start_x;
      nyv = next_y;
      next_y += dir_y;
    } else {
      double next_x_yval = mm * next_x + cc;
      if (mm != 0) {
        double next_y_xval = (next_y - cc) / mm;
        double d1x = start_x - next_x, d1y = start_y - next_x_yval;
        double d2x = start_x - next_y_xval, d2y = start_y - next_y;
        if (d1x * d1x + d1y * d1y < d2x * d2x + d2y * d2y) {
          nxv = next_x;
          nyv = next_x_yval;
          next_x += dir_x;
        } else {
          nxv = next_y_xval;
          nyv = next_y;
          next_y += dir_y;
        }
      } else {
        nxv = next_x;
        nyv = next_x_yval;
        next_x += dir_x;
      }
    }
  }
  // the piece's coarse cell (midpoint, rounded; negative indices wrap like numba's); M: the model's
  // coarse shape (nz0, nx0)
  template <class Model>
  AF_DEV void cell(const Model& M, double nxv, double nyv, int& y_pos, int& x_pos) const {
    x_pos = pyround_i((prev_x + nxv) / 2);
    y_pos = pyround_i((prev_y + nyv) / 2);
    if (x_pos < 0) x_pos += M.nx0;
    if (y_pos < 0) y_pos += M.nz0;
  }
  // the piece's length [m] and its time at slowness slown (time_between_points' summand)
  AF_DEV double piece_dist(double nxv, double nyv, double dnx) const {
    double ddx = prev_x - nxv, ddy = prev_y - nyv;
    return dnx * sqrt(ddx * ddx + ddy * ddy);
  }
  AF_DEV double piece_time(double nxv, double nyv, double dnx, double slown) const {
    return piece_dist(nxv, nyv, dnx) * slown;
  }
};

}  // namespace af
