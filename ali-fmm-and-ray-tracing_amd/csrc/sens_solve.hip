// sens_solve.hip — the resident sensitivity operator (include/alifmm.h alifmm_sens_op_*): products
// with one quantity of the tomography Jacobian in both directions and the CGLS iteration of the
// damped, smoothed least-squares step, all vectors and scalars on the device.
//
// The operator is the unmerged CSR that sens_fill_kernel (ray_sens.hip) writes, and a transposed
// copy of it (CSC) whose columns keep their entries in ascending entry index: a stable radix sort of
// the entry indices by column (rocPRIM; the one-off build step), the row of an entry by bisection
// of row_ptr, col_ptr by bisection of the sorted columns.  Both products are gathers bound by the
// 12 bytes per entry they stream.  A·x: one workgroup per row (rows are long, ~10^4 entries at the
// 4096² workload).  Aᵀ·y: the non-empty columns are listed by length class at build time (their
// lengths run from 1 to thousands) and summed by one thread, one wavefront or one workgroup each.
// Every sum has a fixed order (solve_ops.h: strided lanes, then a fixed tree), there is no float
// atomic, so every result is bit-reproducible.  The arithmetic is solve_ops.h's, shared with
// tests/solve_sim.cpp.
#include <rocprim/device/device_radix_sort.hpp>

#include "kernels.h"
#include "solve_ops.h"
#include "solve_sums.h"  // solve_block_sum, solve_part

namespace af {

// ---- build ----

__global__ __launch_bounds__(kSolveBlock) void solve_iota_kernel(const int* col, unsigned* key, unsigned* idx, long long n) {
  const long long e = (long long)blockIdx.x * kSolveBlock + threadIdx.x;
  if (e >= n) return;
  key[e] = (unsigned)col[e];
  idx[e] = (unsigned)e;
}

// CSC entry j is CSR entry idx[j]: its value, and its row = the last k with row_ptr[k] <= idx[j]
__global__ __launch_bounds__(kSolveBlock) void solve_gather_kernel(SensOp A, const unsigned* idx, int* row, double* cval) {
  const long long j = (long long)blockIdx.x * kSolveBlock + threadIdx.x;
  if (j >= A.entries) return;
  const long long e = idx[j];
  int lo = 0, hi = A.nrays;  // row_ptr[lo] <= e < row_ptr[hi]
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (A.row_ptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  row[j] = lo;
  cval[j] = A.val[e];
}

// col_ptr[c] = the first sorted entry whose column is >= c, c = 0 .. ncell
__global__ __launch_bounds__(kSolveBlock) void solve_colptr_kernel(const unsigned* key, long long n, long ncell, long long* col_ptr) {
  const long c = (long)blockIdx.x * kSolveBlock + threadIdx.x;
  if (c > ncell) return;
  long long lo = 0, hi = n;  // key[lo - 1] < c <= key[hi]
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if ((long)key[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  col_ptr[c] = lo;
}

AF_DEV int solve_col_class(long long n) { return n <= kSolveColThread ? 0 : n <= kSolveColWave ? 1 : 2; }

// cols null: count the non-empty columns of each class into cursor3; else list them, each class from
// its cursor on.  A wavefront claims the places of its columns of a class with one integer atomic and
// keeps them in ascending order, so neighbouring lanes of the column product read neighbouring
// entries; the order of the wavefronts in a list is the arrival's (every column's sum is its own, so
// the order changes no result)
__global__ __launch_bounds__(kSolveBlock) void solve_classify_kernel(const long long* col_ptr, long ncell, int* cols, int* cursor3) {
  const long c = (long)blockIdx.x * kSolveBlock + threadIdx.x;
  const long long n = c < ncell ? col_ptr[c + 1] - col_ptr[c] : 0;
  const int cls = n > 0 ? solve_col_class(n) : -1;
  const int lane = threadIdx.x & (kSolveLanes - 1);
  for (int k = 0; k < 3; k++) {
    const unsigned long long mine = __ballot(cls == k);
    if (mine == 0) continue;  // (uniform per wavefront)
    const int first = __ffsll((long long)mine) - 1;
    int base = 0;
    if (lane == first) base = atomicAdd(cursor3 + k, __popcll(mine));
    base = __shfl(base, first);
    if (cols && cls == k) cols[base + __popcll(mine & ((1ull << lane) - 1))] = (int)c;
  }
}

// ---- products ----

// xs = cs x (solve_ops.h solve_scaled)
__global__ __launch_bounds__(kSolveBlock) void solve_scale_kernel(const double* cs, const double* x, double* xs, long n) {
  const long c = (long)blockIdx.x * kSolveBlock + threadIdx.x;
  if (c < n) xs[c] = solve_scaled(cs, x, c);
}

__global__ __launch_bounds__(kSolveBlock) void solve_rowprod_kernel(SensOp A, const double* xs, double* out) {
  __shared__ double w[kSolveWaves];
  const long k = blockIdx.x;  // < nrays
  const long long e0 = A.row_ptr[k], n = A.row_ptr[k + 1] - e0;
  const int* col = A.col + e0;
  const double* val = A.val + e0;
  const double a = solve_block_sum(
      solve_lane_sum(n, threadIdx.x, kSolveBlock, [&](long e) { return solve_row_term(val[e], xs, col[e]); }), w);
  if (threadIdx.x == 0) out[k] = a;  // an empty row: 0
}

// CLS 0: a thread per column, 1: a wavefront, 2: a workgroup; list = A.cols[CLS]
template <int CLS>
__global__ __launch_bounds__(kSolveBlock) void solve_colprod_kernel(SensOp A, const double* y, double* out) {
  __shared__ double w[kSolveWaves];
  const int per = CLS == 0 ? kSolveBlock : CLS == 1 ? kSolveWaves : 1;  // columns per workgroup
  const int sub = CLS == 0 ? threadIdx.x : CLS == 1 ? threadIdx.x / kSolveLanes : 0;
  const long i = (long)blockIdx.x * per + sub;
  const bool live = i < A.ncols[CLS];  // (uniform per wavefront for CLS 1, per workgroup for CLS 2)
  long c = 0;
  long long n = 0;
  const int* row = nullptr;
  const double* val = nullptr;
  if (live) {
    c = A.cols[CLS][i];
    const long long e0 = A.col_ptr[c];
    n = A.col_ptr[c + 1] - e0;
    row = A.row + e0;
    val = A.cval + e0;
  }
  auto term = [&](long e) { return solve_col_term(val[e], y, row[e]); };
  if (CLS == 0) {
    if (live) out[c] = solve_col_scale(solve_lane_sum(n, 0, 1, term), A.cs, c);
  } else if (CLS == 1) {
    const double a = solve_wave_tree(solve_lane_sum(n, threadIdx.x & (kSolveLanes - 1), kSolveLanes, term),
                                     [](double v, int o) { return __shfl_xor(v, o); });
    if (live && (threadIdx.x & (kSolveLanes - 1)) == 0) out[c] = solve_col_scale(a, A.cs, c);
  } else {
    const double a = solve_block_sum(solve_lane_sum(n, threadIdx.x, kSolveBlock, term), w);
    if (live && threadIdx.x == 0) out[c] = solve_col_scale(a, A.cs, c);
  }
}

// ---- CGLS ----

// |q|² = |A p|² + pᵀ(damp² p + smooth² DᵀD p): the cells' terms, then the rays'
__global__ __launch_bounds__(kSolveBlock) void solve_qq_kernel(SensOp A, SolveVecs V) {
  __shared__ double w[kSolveWaves];
  solve_part(A.ncell + A.nrays, V.parts, w, [&](long i) {
    if (i < A.ncell) return V.p[i] * solve_reg(V.p, A.cs, A.nz, A.nx, i, V.damp2, V.smooth2);
    const double q = V.q[i - A.ncell];
    return q * q;
  });
}

// s = Aᵀ r - (damp² x + smooth² DᵀD x), and the partial sums of gamma = |s|²
__global__ __launch_bounds__(kSolveBlock) void solve_s_kernel(SensOp A, SolveVecs V) {
  __shared__ double w[kSolveWaves];
  solve_part(A.ncell, V.parts, w, [&](long c) {
    const double s = V.t[c] - solve_reg(V.x, A.cs, A.nz, A.nx, c, V.damp2, V.smooth2);
    V.s[c] = s;
    return s * s;
  });
}

__global__ __launch_bounds__(kSolveBlock) void solve_sumsq_kernel(const double* v, long n, double* parts) {
  __shared__ double w[kSolveWaves];
  solve_part(n, parts, w, [&](long i) { return v[i] * v[i]; });
}

// stage 2 (one workgroup) and the scalar that follows from the sum.  WHAT 0: scal[kSolNorm] = sum;
// 1: alpha = gamma / sum (sum = |q|²; 0: alpha = 0 and the breakdown flag); 2: the new gamma = sum,
// beta = sum / gamma, report = sum, or -1 after a breakdown; 3: the start: gamma = report = sum,
// beta = 0, no breakdown
template <int WHAT>
__global__ __launch_bounds__(kSolveBlock) void solve_scalar_kernel(const double* parts, int nparts, double* scal) {
  __shared__ double w[kSolveWaves];
  const double sum = solve_block_sum(solve_lane_sum(nparts, threadIdx.x, kSolveBlock, [&](long i) { return parts[i]; }), w);
  if (threadIdx.x != 0) return;
  if (WHAT == 0) scal[kSolNorm] = sum;
  if (WHAT == 1) {
    scal[kSolAlpha] = sum == 0.0 ? 0.0 : scal[kSolGamma] / sum;
    if (sum == 0.0) scal[kSolBreak] = 1.0;
  }
  if (WHAT == 2) {
    scal[kSolBeta] = sum / scal[kSolGamma];
    scal[kSolGamma] = sum;
    scal[kSolReport] = scal[kSolBreak] != 0.0 ? -1.0 : sum;
  }
  if (WHAT == 3) {
    scal[kSolGamma] = scal[kSolReport] = sum;
    scal[kSolBeta] = scal[kSolBreak] = 0.0;
  }
}

// x += alpha p (cells); r -= alpha q (rays)
__global__ __launch_bounds__(kSolveBlock) void solve_update_kernel(SensOp A, SolveVecs V) {
  const long i = (long)blockIdx.x * kSolveBlock + threadIdx.x;
  const double alpha = V.scal[kSolAlpha];
  if (i < A.ncell) V.x[i] = V.x[i] + alpha * V.p[i];
  else if (i < A.ncell + A.nrays) V.r[i - A.ncell] = V.r[i - A.ncell] - alpha * V.q[i - A.ncell];
}

// p = s + beta p
__global__ __launch_bounds__(kSolveBlock) void solve_p_kernel(SensOp A, SolveVecs V) {
  const long c = (long)blockIdx.x * kSolveBlock + threadIdx.x;
  if (c < A.ncell) V.p[c] = V.s[c] + V.scal[kSolBeta] * V.p[c];
}

}  // namespace af

using namespace af;

static dim3 solve_grid(long long n) { return dim3((unsigned)((n + kSolveBlock - 1) / kSolveBlock)); }

static int solve_key_bits(long ncell) {
  int b = 1;
  while (b < 32 && (1L << b) < ncell) b++;
  return b;
}

extern "C" size_t af_solve_sort_temp(long long entries, long ncell) {
  size_t bytes = 0;
  unsigned* k = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, k, k, k, k, (size_t)entries, 0, solve_key_bits(ncell));
  return bytes;
}

extern "C" hipError_t af_launch_solve_transpose(const SensOp* A, long long* col_ptr, int* row, double* cval, unsigned* key,
                                                unsigned* key2, unsigned* idx, unsigned* idx2, void* temp,
                                                size_t temp_bytes, hipStream_t stream) {
  const long long n = A->entries;
  if (n > 0) {
    hipLaunchKernelGGL(solve_iota_kernel, solve_grid(n), dim3(kSolveBlock), 0, stream, A->col, key, idx, n);
    hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, key, key2, idx, idx2, (size_t)n, 0,
                                             solve_key_bits(A->ncell), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(solve_gather_kernel, solve_grid(n), dim3(kSolveBlock), 0, stream, *A, idx2, row, cval);
    hipLaunchKernelGGL(solve_colptr_kernel, solve_grid(A->ncell + 1), dim3(kSolveBlock), 0, stream, key2, n, A->ncell, col_ptr);
  } else {
    hipError_t e = hipMemsetAsync(col_ptr, 0, (size_t)(A->ncell + 1) * sizeof(long long), stream);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

extern "C" hipError_t af_launch_solve_classify(const long long* col_ptr, long ncell, int* cols, int* cursor3, hipStream_t stream) {
  hipLaunchKernelGGL(solve_classify_kernel, solve_grid(ncell), dim3(kSolveBlock), 0, stream, col_ptr, ncell, cols, cursor3);
  return hipGetLastError();
}

// out = A x; xs [ncell] is scratch for cs x (untouched without a column scale)
extern "C" hipError_t af_launch_solve_rowprod(const SensOp* A, const double* x, double* xs, double* out, hipStream_t stream) {
  if (A->nrays <= 0) return hipSuccess;
  if (A->cs) hipLaunchKernelGGL(solve_scale_kernel, solve_grid(A->ncell), dim3(kSolveBlock), 0, stream, A->cs, x, xs, A->ncell);
  hipLaunchKernelGGL(solve_rowprod_kernel, dim3(A->nrays), dim3(kSolveBlock), 0, stream, *A, A->cs ? xs : x, out);
  return hipGetLastError();
}

extern "C" hipError_t af_launch_solve_colprod(const SensOp* A, const double* y, double* out, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(out, 0, (size_t)A->ncell * sizeof(double), stream);  // the untouched cells
  if (e != hipSuccess) return e;
  const dim3 b(kSolveBlock);
  if (A->ncols[0] > 0) hipLaunchKernelGGL(solve_colprod_kernel<0>, solve_grid(A->ncols[0]), b, 0, stream, *A, y, out);
  if (A->ncols[1] > 0)
    hipLaunchKernelGGL(solve_colprod_kernel<1>, dim3((A->ncols[1] + kSolveWaves - 1) / kSolveWaves), b, 0, stream, *A, y, out);
  if (A->ncols[2] > 0) hipLaunchKernelGGL(solve_colprod_kernel<2>, dim3(A->ncols[2]), b, 0, stream, *A, y, out);
  return hipGetLastError();
}

// gamma_0 = |s|², s = t - reg(x) with x = 0, and p = s (p = s + 0 p, p zeroed by the caller)
extern "C" hipError_t af_launch_solve_start(const SensOp* A, const SolveVecs* V, hipStream_t stream) {
  const int parts = solve_parts(A->ncell);
  hipLaunchKernelGGL(solve_s_kernel, dim3(parts), dim3(kSolveBlock), 0, stream, *A, *V);
  hipLaunchKernelGGL(solve_scalar_kernel<3>, dim3(1), dim3(kSolveBlock), 0, stream, V->parts, parts, V->scal);
  hipLaunchKernelGGL(solve_p_kernel, solve_grid(A->ncell), dim3(kSolveBlock), 0, stream, *A, *V);
  return hipGetLastError();
}

// q = A p; alpha = gamma / |q|²; x += alpha p, r -= alpha q; s and the new gamma; beta; p = s + beta p
extern "C" hipError_t af_launch_solve_iter(const SensOp* A, const SolveVecs* V, hipStream_t stream) {
  const dim3 b(kSolveBlock), one(1);
  const int pq = solve_parts(A->ncell + A->nrays), pc = solve_parts(A->ncell);
  hipError_t e = af_launch_solve_rowprod(A, V->p, V->xs, V->q, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(solve_qq_kernel, dim3(pq), b, 0, stream, *A, *V);
  hipLaunchKernelGGL(solve_scalar_kernel<1>, one, b, 0, stream, V->parts, pq, V->scal);
  hipLaunchKernelGGL(solve_update_kernel, solve_grid(A->ncell + A->nrays), b, 0, stream, *A, *V);
  e = af_launch_solve_colprod(A, V->r, V->t, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(solve_s_kernel, dim3(pc), b, 0, stream, *A, *V);
  hipLaunchKernelGGL(solve_scalar_kernel<2>, one, b, 0, stream, V->parts, pc, V->scal);
  hipLaunchKernelGGL(solve_p_kernel, solve_grid(A->ncell), b, 0, stream, *A, *V);
  return hipGetLastError();
}

// stage 2 of a two-stage sum and its scalar (solve_scalar_kernel), for the CGLS of tfm_solve.hip
extern "C" hipError_t af_launch_solve_scalar(int what, const double* parts, int nparts, double* scal, hipStream_t stream) {
  const dim3 one(1), b(kSolveBlock);
  if (what == 0) hipLaunchKernelGGL(solve_scalar_kernel<0>, one, b, 0, stream, parts, nparts, scal);
  else if (what == 1) hipLaunchKernelGGL(solve_scalar_kernel<1>, one, b, 0, stream, parts, nparts, scal);
  else if (what == 2) hipLaunchKernelGGL(solve_scalar_kernel<2>, one, b, 0, stream, parts, nparts, scal);
  else if (what == 3) hipLaunchKernelGGL(solve_scalar_kernel<3>, one, b, 0, stream, parts, nparts, scal);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

extern "C" hipError_t af_launch_solve_norm(const double* v, long n, const SolveVecs* V, hipStream_t stream) {
  const int parts = solve_parts(n);
  hipLaunchKernelGGL(solve_sumsq_kernel, dim3(parts), dim3(kSolveBlock), 0, stream, v, n, V->parts);
  hipLaunchKernelGGL(solve_scalar_kernel<0>, dim3(1), dim3(kSolveBlock), 0, stream, V->parts, parts, V->scal);
  return hipGetLastError();
}
