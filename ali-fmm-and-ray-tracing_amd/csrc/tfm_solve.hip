// tfm_solve.hip — the vector side of the least-squares imaging solve (include/alifmm.h
// alifmm_tfm_lsq): CGLS on min |A x - d|² + damp² |x|² + smooth² |D x|² with A the FMC modelling
// kernel (tfm_model.hip, run on the dense window through the pixel list written here) and Aᵀ the
// float64 TFM kernel (tfm.hip).  This file holds what lies between the two products: the pixel list
// and the fused vector kernels of an iteration.  Every vector and every scalar stays on the device;
// the scalars (gamma, alpha, beta, the breakdown flag) are those of sens_solve.hip, made by its
// stage-2 kernel (af_launch_solve_scalar), and the iteration is that of alifmm_sens_op_solve line
// for line.  All these kernels stream their vectors once and are bound by that traffic.  The
// arithmetic is tfm_solve_ops.h's, the sums are solve_ops.h's (both shared with
// tests/tfm_lsq_sim.cpp); every index is 64-bit.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "solve_sums.h"

namespace af {

// pix[i * nix + j] = the field offset of pixel (i, j) of the window: the dense list, raster order
__global__ __launch_bounds__(kSolveBlock) void tfm_lsq_pix_kernel(int iz0, int ix0, int step, int fnx, int niz, int nix,
                                                                  int64_t* pix) {
  const int64_t q = (int64_t)blockIdx.x * kSolveBlock + threadIdx.x;
  if (q >= (int64_t)niz * nix) return;
  pix[q] = tfm_model_pixel_offset(iz0, ix0, step, fnx, (int)(q / nix), (int)(q % nix));
}

__global__ __launch_bounds__(kSolveBlock) void tfm_lsq_qq_kernel(TfmLsqDims G, SolveVecs V) {
  __shared__ double w[kSolveWaves];
  solve_part((long)(G.nimg + G.ndata), V.parts, w,
             [&](long i) { return tfm_lsq_qq_term(G, V.p, V.q, V.damp2, V.smooth2, i); });
}

__global__ __launch_bounds__(kSolveBlock) void tfm_lsq_update_kernel(TfmLsqDims G, SolveVecs V) {
  const int64_t i = (int64_t)blockIdx.x * kSolveBlock + threadIdx.x;
  tfm_lsq_update(G, V.x, V.p, V.r, V.q, V.scal[kSolAlpha], i);
}

__global__ __launch_bounds__(kSolveBlock) void tfm_lsq_s_kernel(TfmLsqDims G, SolveVecs V) {
  __shared__ double w[kSolveWaves];
  solve_part((long)G.nimg, V.parts, w, [&](long e) { return tfm_lsq_s_term(G, V.t, V.x, V.s, V.damp2, V.smooth2, e); });
}

__global__ __launch_bounds__(kSolveBlock) void tfm_lsq_p_kernel(TfmLsqDims G, SolveVecs V) {
  const int64_t e = (int64_t)blockIdx.x * kSolveBlock + threadIdx.x;
  if (e < G.nimg) tfm_lsq_p(V.s, V.p, V.scal[kSolBeta], e);
}

}  // namespace af

using namespace af;

// one thread per element; false: more workgroups than a launch takes
static bool lsq_grid(int64_t n, dim3* g) {
  const int64_t b = (n + kSolveBlock - 1) / kSolveBlock;
  if (b < 1 || b > 0x7fffffffLL) return false;
  *g = dim3((unsigned)b);
  return true;
}

extern "C" hipError_t af_launch_tfm_lsq_pix(int iz0, int ix0, int step, int fnx, int niz, int nix, int64_t* pix,
                                            hipStream_t stream) {
  dim3 g;
  if (niz < 1 || nix < 1 || !lsq_grid((int64_t)niz * nix, &g)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tfm_lsq_pix_kernel, g, dim3(kSolveBlock), 0, stream, iz0, ix0, step, fnx, niz, nix, pix);
  return hipGetLastError();
}

// after q = A p: alpha = gamma / (|q|² + p·R(p)) (0 and the breakdown flag when that is 0);
// x += alpha p, r -= alpha q
extern "C" hipError_t af_launch_tfm_lsq_step(const TfmLsqDims* G, const SolveVecs* V, hipStream_t stream) {
  dim3 g;
  if (!lsq_grid(G->nimg + G->ndata, &g)) return hipErrorInvalidValue;
  const int parts = solve_parts((long)(G->nimg + G->ndata));
  hipLaunchKernelGGL(tfm_lsq_qq_kernel, dim3(parts), dim3(kSolveBlock), 0, stream, *G, *V);
  hipError_t e = af_launch_solve_scalar(1, V->parts, parts, V->scal, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tfm_lsq_update_kernel, g, dim3(kSolveBlock), 0, stream, *G, *V);
  return hipGetLastError();
}

// after t = Aᵀ r: s = t - R(x) and gamma = |s|²; start: gamma_0 = gamma, beta = 0 (p zeroed by the
// caller), else beta = gamma' / gamma and the iteration's report; p = s + beta p
extern "C" hipError_t af_launch_tfm_lsq_grad(const TfmLsqDims* G, const SolveVecs* V, int start, hipStream_t stream) {
  dim3 g;
  if (!lsq_grid(G->nimg, &g)) return hipErrorInvalidValue;
  const int parts = solve_parts((long)G->nimg);
  hipLaunchKernelGGL(tfm_lsq_s_kernel, dim3(parts), dim3(kSolveBlock), 0, stream, *G, *V);
  hipError_t e = af_launch_solve_scalar(start ? 3 : 2, V->parts, parts, V->scal, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tfm_lsq_p_kernel, g, dim3(kSolveBlock), 0, stream, *G, *V);
  return hipGetLastError();
}
