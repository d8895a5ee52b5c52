// Stand-alone host run of the resident sensitivity operator's arithmetic (csrc/solve_ops.h: the
// entry terms of both products, the DᵀD stencil, the lanes' shares of a sum and the pairing of the
// reduction trees), built with ASan and UBSan by tests/test_solve_ref.py.  It replays the kernels of
// csrc/sens_solve.hip sum by sum: the transposed copy (columns in ascending entry index), A x with a
// workgroup per row, Aᵀ y with a thread, a wavefront or a workgroup per column, and the CGLS of
// alifmm_sens_op_solve with its two-stage dot products and its stop rule, so the index arithmetic
// is checked on a CPU before the kernels run on a GPU.  Test infrastructure only.
//   solve_sim INPUT OUTPUT   INPUT: the file of tests/solve_ref.py write_sim_input(); OUTPUT: float64
//   A x [nrays], Aᵀ y [ncell], the solve's x [ncell], info8.  Exit status 0, or 2 on a malformed input.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define AF_DEV inline
#include "solve_ops.h"

using namespace af;

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// the 64 lanes of a wavefront in lock step
struct Lanes {
  double a[kSolveLanes];
};
static Lanes operator+(const Lanes& x, const Lanes& y) {
  Lanes r;
  for (int l = 0; l < kSolveLanes; l++) r.a[l] = x.a[l] + y.a[l];
  return r;
}
static bool g_tree_ok = true;  // every lane of a wavefront ends with the same sum
template <class Term>
static double wave_sum(long n, int lane0, int width, Term term) {
  Lanes v;
  for (int l = 0; l < kSolveLanes; l++) v.a[l] = solve_lane_sum(n, lane0 + l, width, term);
  v = solve_wave_tree(v, [](const Lanes& x, int o) {
    Lanes r;
    for (int l = 0; l < kSolveLanes; l++) r.a[l] = x.a[l ^ o];
    return r;
  });
  for (int l = 1; l < kSolveLanes; l++) g_tree_ok = g_tree_ok && memcmp(&v.a[l], &v.a[0], 8) == 0;
  return v.a[0];
}
// a workgroup whose thread t is lane lane0 + t of `width`
template <class Term>
static double block_sum(long n, int lane0, int width, Term term) {
  double w[kSolveWaves];
  for (int k = 0; k < kSolveWaves; k++) w[k] = wave_sum(n, lane0 + k * kSolveLanes, width, term);
  return solve_block_tree(w);
}
// the two-stage sum of sens_solve.hip solve_part + solve_scalar_kernel
template <class Term>
static double two_stage(long n, Term term) {
  const int parts = solve_parts(n);
  std::vector<double> part((size_t)parts);
  for (int b = 0; b < parts; b++) part[b] = block_sum(n, b * kSolveBlock, parts * kSolveBlock, term);
  return block_sum(parts, 0, kSolveBlock, [&](long i) { return part[(size_t)i]; });
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int64_t> h, row_ptr;
  std::vector<double> par, val, cs_v, xin, yin, rhs;
  std::vector<int32_t> col;
  if (!rd(f, h, 6) || !rd(f, par, 3)) return 2;
  const int64_t nrays = h[0], nz = h[1], nx = h[2], ne = h[3], have_cs = h[4], max_iter = h[5];
  if (nrays < 0 || nrays > (1 << 24) || nz < 1 || nx < 1 || nz * nx > (1 << 24) || ne < 0 || ne > (1LL << 28) || max_iter < 1)
    return 2;
  const long ncell = (long)(nz * nx);
  if (!rd(f, row_ptr, (size_t)nrays + 1) || !rd(f, col, (size_t)ne) || !rd(f, val, (size_t)ne) ||
      !rd(f, cs_v, have_cs ? (size_t)ncell : 0) || !rd(f, xin, (size_t)ncell) || !rd(f, yin, (size_t)nrays) ||
      !rd(f, rhs, (size_t)nrays))
    return 2;
  fclose(f);
  if (row_ptr[0] != 0 || row_ptr[(size_t)nrays] != ne) return 2;
  for (int64_t k = 0; k < nrays; k++)
    if (row_ptr[k + 1] < row_ptr[k]) return 2;
  for (int32_t c : col)
    if (c < 0 || c >= ncell) return 2;
  const double* cs = have_cs ? cs_v.data() : nullptr;
  const double damp2 = par[0] * par[0], smooth2 = par[1] * par[1], tol = par[2];

  // the transposed copy: a stable sort of the entries by column; an entry's row by bisection
  std::vector<int64_t> col_ptr((size_t)ncell + 1, 0);
  for (int32_t c : col) col_ptr[(size_t)c + 1]++;
  for (long c = 0; c < ncell; c++) col_ptr[c + 1] += col_ptr[c];
  std::vector<int32_t> crow((size_t)ne);
  std::vector<double> cval((size_t)ne);
  {
    std::vector<int64_t> at(col_ptr.begin(), col_ptr.end() - 1);
    for (int64_t e = 0; e < ne; e++) {
      int lo = 0, hi = (int)nrays;  // row_ptr[lo] <= e < row_ptr[hi]
      while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (row_ptr[mid] <= e) lo = mid;
        else hi = mid;
      }
      const int64_t j = at[col[e]]++;
      crow[j] = lo;
      cval[j] = val[e];
    }
  }

  std::vector<double> xs((size_t)ncell);
  auto rowprod = [&](const double* x, double* out) {
    for (long c = 0; c < ncell; c++) xs[c] = solve_scaled(cs, x, c);
    for (int64_t k = 0; k < nrays; k++) {
      const int32_t* c = col.data() + row_ptr[k];
      const double* v = val.data() + row_ptr[k];
      out[k] = block_sum(row_ptr[k + 1] - row_ptr[k], 0, kSolveBlock,
                         [&](long e) { return solve_row_term(v[e], xs.data(), c[e]); });
    }
  };
  auto colprod = [&](const double* y, double* out) {
    for (long c = 0; c < ncell; c++) {
      const long n = (long)(col_ptr[c + 1] - col_ptr[c]);
      const int32_t* r = crow.data() + col_ptr[c];
      const double* v = cval.data() + col_ptr[c];
      auto term = [&](long e) { return solve_col_term(v[e], y, r[e]); };
      if (n == 0) out[c] = 0.0;
      else if (n <= kSolveColThread) out[c] = solve_col_scale(solve_lane_sum(n, 0, 1, term), cs, c);
      else if (n <= kSolveColWave) out[c] = solve_col_scale(wave_sum(n, 0, kSolveLanes, term), cs, c);
      else out[c] = solve_col_scale(block_sum(n, 0, kSolveBlock, term), cs, c);
    }
  };

  std::vector<double> ax((size_t)nrays), aty((size_t)ncell);
  rowprod(xin.data(), ax.data());
  colprod(yin.data(), aty.data());

  // alifmm_sens_op_solve
  std::vector<double> x((size_t)ncell, 0.0), p((size_t)ncell, 0.0), s((size_t)ncell), t((size_t)ncell), r(rhs),
      q((size_t)nrays);
  auto grad = [&] {  // solve_s_kernel: s and |s|²
    return two_stage(ncell, [&](long c) {
      s[c] = t[c] - solve_reg(x.data(), cs, (int)nz, (int)nx, c, damp2, smooth2);
      return s[c] * s[c];
    });
  };
  const double rhs2 = two_stage((long)nrays, [&](long i) { return r[i] * r[i]; });
  colprod(r.data(), t.data());
  const double gamma0 = grad();
  double gamma = gamma0, beta = 0.0;
  for (long c = 0; c < ncell; c++) p[c] = s[c] + beta * p[c];
  int iters = 0, reason = 1;
  if (gamma0 == 0.0) reason = 2;
  else
    for (int it = 1; it <= max_iter; it++) {
      rowprod(p.data(), q.data());
      const double qq = two_stage(ncell + (long)nrays, [&](long i) {
        if (i < ncell) return p[i] * solve_reg(p.data(), cs, (int)nz, (int)nx, i, damp2, smooth2);
        return q[i - ncell] * q[i - ncell];
      });
      if (qq == 0.0) {
        reason = 2;
        break;
      }
      const double alpha = gamma / qq;
      for (long c = 0; c < ncell; c++) x[c] = x[c] + alpha * p[c];
      for (int64_t k = 0; k < nrays; k++) r[k] = r[k] - alpha * q[k];
      colprod(r.data(), t.data());
      const double now = grad();
      beta = now / gamma;
      gamma = now;
      for (long c = 0; c < ncell; c++) p[c] = s[c] + beta * p[c];
      iters = it;
      if (gamma <= tol * tol * gamma0) {
        reason = 0;
        break;
      }
    }
  const double res2 = two_stage((long)nrays, [&](long i) { return r[i] * r[i]; });
  if (!g_tree_ok) return 3;
  const double info[8] = {(double)iters, sqrt(gamma0), sqrt(gamma), sqrt(rhs2), sqrt(res2), (double)reason, (double)ne, 0.0};
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 2;
  bool ok = (ax.empty() || fwrite(ax.data(), 8, ax.size(), g) == ax.size()) && fwrite(aty.data(), 8, aty.size(), g) == aty.size() &&
            fwrite(x.data(), 8, x.size(), g) == x.size() && fwrite(info, 8, 8, g) == 8;
  fclose(g);
  return ok ? 0 : 2;
}
