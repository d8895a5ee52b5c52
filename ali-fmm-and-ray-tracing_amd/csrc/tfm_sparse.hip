// tfm_sparse.hip — the vector side of sparsity-regularised imaging (include/alifmm.h
// alifmm_tfm_sparse): FISTA with backtracking and gradient restart on ½ |B x - d|² + ½ x·R(x) +
// lam Σ |x_p|, B = P A with A the FMC modelling kernel (tfm_model.hip, on the dense window through
// tfm_solve.hip's pixel list), Aᵀ the float64 TFM kernel (tfm.hip) and P the trace FIR
// (trace_fir.hip).  This file holds what lies between the products: the prox and the fused passes
// of an iteration.  Every vector stays on the device; the host reads 32 bytes per trial for the
// accept test, the stop rule and the restart.  All these kernels stream their vectors once and are
// bound by that traffic: an accepted iteration reads B x⁺ twice (the trial's sum, then the momentum
// pass that forms the next r) and writes it once (A or P), reads d twice and B x once, writes r once
// and reads it once (Aᵀ or Pᵀ).  The sums of one pass go into partial arrays side by side.  The
// arithmetic is tfm_sparse_ops.h's, the sums are solve_ops.h's (both shared with
// tests/tfm_sparse_sim.cpp); every index is 64-bit.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "solve_sums.h"

namespace af {

// stage 1 of K two-stage sums of one pass over n elements: parts[k * kSolveMaxParts + blockIdx.x]
template <int K, class Term>
AF_DEV void sparse_part(long n, double* parts, Term term) {
  __shared__ double w[K][kSolveWaves];
  double a[K];
  sparse_lane_sums<K>(n, (int)(blockIdx.x * kSolveBlock + threadIdx.x), (int)(gridDim.x * kSolveBlock), a, term);
  for (int k = 0; k < K; k++) {
    const double s = solve_block_sum(a[k], w[k]);
    if (threadIdx.x == 0) parts[(size_t)k * kSolveMaxParts + blockIdx.x] = s;
  }
}
// stage 2 by one workgroup: the sum of parts[0 .. nparts), valid in thread 0 (w: kSolveWaves values
// of this sum's own)
AF_DEV double sparse_total(const double* parts, int nparts, double* w) {
  return solve_block_sum(solve_lane_sum(nparts, threadIdx.x, kSolveBlock, [&](long i) { return parts[i]; }), w);
}

// the start from t = Bᵀ d: g = -t, |g0|² and lam_max = max_p |g0_p| (a maximum: any order gives the
// same value; here a lane's pixels, the wave, the workgroup, one partial per workgroup)
__global__ __launch_bounds__(kSolveBlock) void tfm_sparse_start_kernel(TfmLsqDims G, SparseVecs V) {
  __shared__ double wm[kSolveWaves];
  sparse_part<1>((long)G.nimg, V.parts, [&](long e, double* o) { sparse_start_term(V.t, V.g, e, o); });
  const int64_t npix = G.nimg / G.nc;
  double m = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * kSolveBlock + threadIdx.x; q < npix; q += (int64_t)gridDim.x * kSolveBlock)
    m = fmax(m, sparse_modulus(V.t, G.nc, q));
  for (int o = kSolveLanes / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  if ((threadIdx.x & (kSolveLanes - 1)) == 0) wm[threadIdx.x / kSolveLanes] = m;
  __syncthreads();
  if (threadIdx.x == 0) V.parts[(size_t)kSolveMaxParts + blockIdx.x] = fmax(fmax(wm[0], wm[1]), fmax(wm[2], wm[3]));
}
// rr: |d|² (af_launch_solve_norm's scalar)
__global__ __launch_bounds__(kSolveBlock) void tfm_sparse_start_scalar_kernel(SparseVecs V, int nparts, const double* rr) {
  __shared__ double w[kSolveWaves], wm[kSolveWaves];
  const double g0 = sparse_total(V.parts, nparts, w);
  double m = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kSolveBlock) m = fmax(m, V.parts[(size_t)kSolveMaxParts + i]);
  for (int o = kSolveLanes / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  if ((threadIdx.x & (kSolveLanes - 1)) == 0) wm[threadIdx.x / kSolveLanes] = m;
  __syncthreads();
  if (threadIdx.x != 0) return;
  V.scal[kSpG0] = g0;
  V.scal[kSpLamMax] = fmax(fmax(wm[0], wm[1]), fmax(wm[2], wm[3]));
  V.scal[kSpRr] = *rr;
  V.scal[kSpFy] = sparse_fy(*rr, 0.0);
  V.scal[kSpEst] = sqrt(g0);  // the power iteration's first divisor, |g0|
}

__global__ __launch_bounds__(kSolveBlock) void tfm_sparse_power_scale_kernel(TfmLsqDims G, SparseVecs V) {
  const int64_t e = (int64_t)blockIdx.x * kSolveBlock + threadIdx.x;
  if (e < G.nimg) sparse_power_scale(V.t, V.xn, V.scal[kSpEst], e);
}
__global__ __launch_bounds__(kSolveBlock) void tfm_sparse_power_kernel(TfmLsqDims G, SparseVecs V) {
  sparse_part<1>((long)G.nimg, V.parts,
                 [&](long e, double* o) { sparse_power_term(G, V.t, V.xn, V.damp2, V.smooth2, e, o); });
}
__global__ __launch_bounds__(kSolveBlock) void tfm_sparse_power_scalar_kernel(SparseVecs V, int nparts) {
  __shared__ double w[kSolveWaves];
  const double s = sparse_total(V.parts, nparts, w);
  if (threadIdx.x == 0) V.scal[kSpEst] = sqrt(s);
}

__global__ __launch_bounds__(kSolveBlock) void tfm_sparse_grad_kernel(TfmLsqDims G, SparseVecs V) {
  sparse_part<1>((long)G.nimg, V.parts,
                 [&](long e, double* o) { sparse_grad_term(G, V.t, V.y, V.g, V.damp2, V.smooth2, e, o); });
}
// fy from y·R(y) (nparts partials) and the momentum pass's |r|² (nparts_rr partials of their own array)
__global__ __launch_bounds__(kSolveBlock) void tfm_sparse_grad_scalar_kernel(SparseVecs V, int nparts, int nparts_rr) {
  __shared__ double w[2][kSolveWaves];
  const double yry = sparse_total(V.parts, nparts, w[0]);
  const double rr = sparse_total(V.parts + (size_t)kSpPartRr * kSolveMaxParts, nparts_rr, w[1]);
  if (threadIdx.x != 0) return;
  V.scal[kSpRr] = rr;
  V.scal[kSpFy] = sparse_fy(rr, yry);
}

__global__ __launch_bounds__(kSolveBlock) void tfm_sparse_prox_kernel(TfmLsqDims G, SparseVecs V, double step, double tau) {
  const int64_t q = (int64_t)blockIdx.x * kSolveBlock + threadIdx.x;
  if (q < G.nimg / G.nc) sparse_prox(V.y, V.g, V.xn, G.nc, step, tau, q);
}

__global__ __launch_bounds__(kSolveBlock) void tfm_sparse_trial_kernel(TfmLsqDims G, SparseVecs V) {
  sparse_part<5>((long)(G.nimg + G.ndata), V.parts, [&](long i, double* o) {
    sparse_trial_term(G, V.xn, V.x, V.y, V.g, V.bxn, V.d, V.damp2, V.smooth2, i, o);
  });
}
__global__ __launch_bounds__(kSolveBlock) void tfm_sparse_trial_scalar_kernel(SparseVecs V, int nparts, double L) {
  __shared__ double w[5][kSolveWaves];
  double s[5];
  for (int k = 0; k < 5; k++) s[k] = sparse_total(V.parts + (size_t)k * kSolveMaxParts, nparts, w[k]);
  if (threadIdx.x == 0) sparse_trial_scalars(s, V.scal[kSpFy], L, V.scal + kSpOut);
}

__global__ __launch_bounds__(kSolveBlock) void tfm_sparse_momentum_kernel(TfmLsqDims G, SparseVecs V, double beta) {
  sparse_part<1>((long)(G.nimg + G.ndata), V.parts + (size_t)kSpPartRr * kSolveMaxParts, [&](long i, double* o) {
    sparse_momentum_term(G, V.xn, V.x, V.y, V.bxn, V.bx, V.d, V.r, beta, i, o);
  });
}

__global__ __launch_bounds__(kSolveBlock) void tfm_sparse_final_kernel(TfmLsqDims G, SparseVecs V) {
  sparse_part<2>((long)(G.ndata + G.nimg / G.nc), V.parts,
                 [&](long i, double* o) { sparse_final_term(G, V.x, V.bx, V.d, V.r, i, o); });
}
__global__ __launch_bounds__(kSolveBlock) void tfm_sparse_final_scalar_kernel(SparseVecs V, int nparts) {
  __shared__ double w[2][kSolveWaves];
  const double res = sparse_total(V.parts, nparts, w[0]);
  const double nnz = sparse_total(V.parts + (size_t)kSolveMaxParts, nparts, w[1]);
  if (threadIdx.x != 0) return;
  V.scal[kSpRes] = res;
  V.scal[kSpNnz] = nnz;
}

}  // namespace af

using namespace af;

// one thread per element; false: more workgroups than a launch takes
static bool sparse_grid(int64_t n, dim3* g) {
  const int64_t b = (n + kSolveBlock - 1) / kSolveBlock;
  if (b < 1 || b > 0x7fffffffLL) return false;
  *g = dim3((unsigned)b);
  return true;
}
static const dim3 kOne(1), kBlock(kSolveBlock);

// after t = Bᵀ d: g = -t, |g0|², lam_max, fy = ½ |d|² (rr: |d|² on the device), the first divisor |g0|
extern "C" hipError_t af_launch_tfm_sparse_start(const TfmLsqDims* G, const SparseVecs* V, const double* rr,
                                                 hipStream_t stream) {
  const int parts = solve_parts((long)G->nimg);
  hipLaunchKernelGGL(tfm_sparse_start_kernel, dim3(parts), kBlock, 0, stream, *G, *V);
  hipLaunchKernelGGL(tfm_sparse_start_scalar_kernel, kOne, kBlock, 0, stream, *V, parts, rr);
  return hipGetLastError();
}

// the power iteration's v (in xn) = t / scal[kSpEst]
extern "C" hipError_t af_launch_tfm_sparse_power_scale(const TfmLsqDims* G, const SparseVecs* V, hipStream_t stream) {
  dim3 g;
  if (!sparse_grid(G->nimg, &g)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tfm_sparse_power_scale_kernel, g, kBlock, 0, stream, *G, *V);
  return hipGetLastError();
}
// after t = Bᵀ B v: w = t + R(v) in t, scal[kSpEst] = |w|
extern "C" hipError_t af_launch_tfm_sparse_power(const TfmLsqDims* G, const SparseVecs* V, hipStream_t stream) {
  const int parts = solve_parts((long)G->nimg);
  hipLaunchKernelGGL(tfm_sparse_power_kernel, dim3(parts), kBlock, 0, stream, *G, *V);
  hipLaunchKernelGGL(tfm_sparse_power_scalar_kernel, kOne, kBlock, 0, stream, *V, parts);
  return hipGetLastError();
}

// after t = Bᵀ r: g = t + R(y), fy = ½ |r|² + ½ y·R(y) (|r|²: the partials the momentum pass left)
extern "C" hipError_t af_launch_tfm_sparse_grad(const TfmLsqDims* G, const SparseVecs* V, hipStream_t stream) {
  const int parts = solve_parts((long)G->nimg);
  hipLaunchKernelGGL(tfm_sparse_grad_kernel, dim3(parts), kBlock, 0, stream, *G, *V);
  hipLaunchKernelGGL(tfm_sparse_grad_scalar_kernel, kOne, kBlock, 0, stream, *V, parts,
                     solve_parts((long)(G->nimg + G->ndata)));
  return hipGetLastError();
}

// x⁺ = prox(y - step g, tau) per pixel
extern "C" hipError_t af_launch_tfm_sparse_prox(const TfmLsqDims* G, const SparseVecs* V, double step, double tau,
                                                hipStream_t stream) {
  dim3 g;
  if (!sparse_grid(G->nimg / G->nc, &g)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tfm_sparse_prox_kernel, g, kBlock, 0, stream, *G, *V, step, tau);
  return hipGetLastError();
}

// after B x⁺: the trial's five sums in one pass and scal[kSpOut .. + 3]
extern "C" hipError_t af_launch_tfm_sparse_trial(const TfmLsqDims* G, const SparseVecs* V, double L, hipStream_t stream) {
  const int parts = solve_parts((long)(G->nimg + G->ndata));
  hipLaunchKernelGGL(tfm_sparse_trial_kernel, dim3(parts), kBlock, 0, stream, *G, *V);
  hipLaunchKernelGGL(tfm_sparse_trial_scalar_kernel, kOne, kBlock, 0, stream, *V, parts, L);
  return hipGetLastError();
}

// y = x⁺ + beta (x⁺ - x); r = (B x⁺ + beta (B x⁺ - B x)) - d and the partials of |r|²
extern "C" hipError_t af_launch_tfm_sparse_momentum(const TfmLsqDims* G, const SparseVecs* V, double beta,
                                                    hipStream_t stream) {
  const int parts = solve_parts((long)(G->nimg + G->ndata));
  hipLaunchKernelGGL(tfm_sparse_momentum_kernel, dim3(parts), kBlock, 0, stream, *G, *V, beta);
  return hipGetLastError();
}

// r = d - B x, scal[kSpRes] = |r|², scal[kSpNnz] = the non-zero pixels of x
extern "C" hipError_t af_launch_tfm_sparse_final(const TfmLsqDims* G, const SparseVecs* V, hipStream_t stream) {
  const int parts = solve_parts((long)(G->ndata + G->nimg / G->nc));
  hipLaunchKernelGGL(tfm_sparse_final_kernel, dim3(parts), kBlock, 0, stream, *G, *V);
  hipLaunchKernelGGL(tfm_sparse_final_scalar_kernel, kOne, kBlock, 0, stream, *V, parts);
  return hipGetLastError();
}
