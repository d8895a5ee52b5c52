// solve_ops.h — the per-element arithmetic and the summation orders of the resident sensitivity
// operator (include/alifmm.h alifmm_sens_op_*): the term of an entry in both products, the term of
// the DᵀD stencil, which elements a lane, a wavefront and a workgroup add, and the pairing of the
// reduction tree.  Shared verbatim by the kernels (sens_solve.hip) and by a stand-alone host program
// (tests/solve_sim.cpp, built with ASan and UBSan) that replays the kernels' sums term by term.
// Includes nothing from HIP; the includer defines AF_DEV (the function qualifier); build with
// -ffp-contract=off.
#pragma once

namespace af {

constexpr int kSolveLanes = 64;                        // a wavefront
constexpr int kSolveWaves = 4;                         // wavefronts per workgroup
constexpr int kSolveBlock = kSolveLanes * kSolveWaves;  // 256 threads
// column product: a column of up to kSolveColThread entries is summed by one thread, of up to
// kSolveColWave by one wavefront, a longer one by one workgroup
constexpr int kSolveColThread = 4;
constexpr int kSolveColWave = 256;
// two-stage sums over a vector: at most this many workgroups leave one partial sum each
constexpr int kSolveMaxParts = 1024;

// A·x: the term of entry (col, val) of a row is val * (cs[col] * x[col]), cs null = 1.  The scaled
// vector xs = cs x is made once per product (one pass over the cells), so that an entry gathers one
// value, not two: the same bits
AF_DEV double solve_scaled(const double* cs, const double* x, long c) { return cs ? cs[c] * x[c] : x[c]; }
AF_DEV double solve_row_term(double val, const double* xs, int col) { return val * xs[col]; }
// Aᵀ·y: the term of entry (row, val) of a column; the column's sum is multiplied by cs[c] once
AF_DEV double solve_col_term(double val, const double* y, int row) { return val * y[row]; }
AF_DEV double solve_col_scale(double sum, const double* cs, long c) { return cs ? cs[c] * sum : sum; }

// (DᵀD v)[c], D the first difference over every 4-neighbour pair of cells that both have cs != 0:
// the differences to the upper, left, right and lower neighbour, added in that order; 0 in a
// frozen cell
AF_DEV bool solve_live(const double* cs, long c) { return !cs || cs[c] != 0.0; }
AF_DEV double solve_stencil(const double* v, const double* cs, int nz, int nx, long c) {
  if (!solve_live(cs, c)) return 0.0;
  const int z = (int)(c / nx), x = (int)(c % nx);
  const double vc = v[c];
  double s = 0.0;
  if (z > 0 && solve_live(cs, c - nx)) s += vc - v[c - nx];
  if (x > 0 && solve_live(cs, c - 1)) s += vc - v[c - 1];
  if (x + 1 < nx && solve_live(cs, c + 1)) s += vc - v[c + 1];
  if (z + 1 < nz && solve_live(cs, c + nx)) s += vc - v[c + nx];
  return s;
}
// the regularisation's share of an element: damp² v + smooth² DᵀD v
AF_DEV double solve_reg(const double* v, const double* cs, int nz, int nx, long c, double damp2, double smooth2) {
  return damp2 * v[c] + smooth2 * solve_stencil(v, cs, nz, nx, c);
}

// The sum of n terms by `width` lanes (64: a wavefront, 256: a workgroup): lane l adds the terms
// l, l + width, l + 2 width, ... in that order, starting from 0
template <class Term>
AF_DEV double solve_lane_sum(long n, int lane, int width, Term term) {
  double a = 0.0;
  long e = lane;
  // four terms at a time, so that their loads are in flight together; added one by one, in order
  for (; e + 3L * width < n; e += 4L * width) {
    const double t0 = term(e), t1 = term(e + width), t2 = term(e + 2L * width), t3 = term(e + 3L * width);
    a += t0;
    a += t1;
    a += t2;
    a += t3;
  }
  for (; e < n; e += width) a += term(e);
  return a;
}
// ... then the 64 lanes of a wavefront pair up over the lane distances 32, 16, 8, 4, 2, 1
// (partner(v, o): the value of lane ^ o; every lane ends with the same sum) ...
template <class V, class Partner>
AF_DEV V solve_wave_tree(V v, Partner partner) {
  for (int o = kSolveLanes / 2; o > 0; o >>= 1) v = v + partner(v, o);
  return v;
}
// ... and the wavefronts' sums of a workgroup pair up as (0 + 1) + (2 + 3)
AF_DEV double solve_block_tree(const double* w) { return (w[0] + w[1]) + (w[2] + w[3]); }

// Two-stage sum over n elements: thread t of workgroup b of solve_parts(n) is lane b 256 + t of
// parts x 256 lanes (solve_lane_sum), a workgroup's threads add up as above and leave one partial;
// one workgroup then adds the partials the same way.  The number of partials depends on n alone.
constexpr int solve_parts(long n) {  // (constexpr: the launchers call it on the host)
  const long b = (n + kSolveBlock - 1) / kSolveBlock;
  return b < 1 ? 1 : b > kSolveMaxParts ? kSolveMaxParts : (int)b;
}

}  // namespace af
