// tfm_coh.hip — coherence-weighted TFM over resident travel-time fields (include/alifmm.h
// alifmm_tfm_coh).  tfm.hip's mapping: one thread per pixel; a wave covers 64 consecutive x of one
// image row, a workgroup kTfmCohRows rows; tail tiles, step > 1 and nrx not a multiple of RC go
// through the same code with predicates.  Next to the image's accumulators a pixel keeps the count
// of its terms and the sums of one kind (3 or 4 more float64 registers, against the 2 RC that hold
// the chunk's delays) across the chunks; the factor is computed from them in registers, and the
// image, the factor and, if asked for, the raw sums are stored once.  The per-pixel arithmetic and
// its order are tfm_coh_term.h's (shared with tests/tfm_coh_sim.cpp).
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace af {

constexpr int kTfmCohRows = 4;  // waves (image rows) per workgroup, tfm.hip's kTfmRows

template <int NC, int RC, int KIND>
__global__ __launch_bounds__(64 * kTfmCohRows) void tfm_coh_kernel(TfmCohParams Q) {
  const TfmParams& P = Q.T;
  const int j = blockIdx.x * 64 + threadIdx.x;
  const int i = blockIdx.y * kTfmCohRows + threadIdx.y;
  if (i >= P.niz || j >= P.nix) return;
  TfmCohAcc<NC> A;
  tfm_coh_pixel<NC, RC, KIND>(P, tfm_pixel_offset(P, i, j), A);
  const int64_t pix = (int64_t)i * P.nix + j;
  double* o = P.image + pix * NC;
#pragma unroll
  for (int c = 0; c < NC; c++) o[c] = A.s[c];
  Q.factor[pix] = tfm_coh_factor<NC, KIND>(A);
  if (Q.sums) {
    double* q = Q.sums + pix * 3;
    q[0] = A.n, q[1] = A.x[0], q[2] = A.x[1];
  }
}

template <int NC, int KIND>
static hipError_t launch_coh(const TfmCohParams& Q, int chunk, dim3 grid, dim3 block, hipStream_t stream) {
  if (chunk == 4) hipLaunchKernelGGL((tfm_coh_kernel<NC, 4, KIND>), grid, block, 0, stream, Q);
  else if (chunk == 16) hipLaunchKernelGGL((tfm_coh_kernel<NC, 16, KIND>), grid, block, 0, stream, Q);
  else if (chunk == 32) hipLaunchKernelGGL((tfm_coh_kernel<NC, 32, KIND>), grid, block, 0, stream, Q);
  else hipLaunchKernelGGL((tfm_coh_kernel<NC, kTfmChunk, KIND>), grid, block, 0, stream, Q);
  return hipGetLastError();
}

}  // namespace af

// kind: 1 CF, 2 SCF, 3 PCF (ncomp 2 only); chunk as in af_launch_tfm
extern "C" hipError_t af_launch_tfm_coh(const af::TfmCohParams* Q, int kind, int chunk, hipStream_t stream) {
  const af::TfmParams& P = Q->T;
  if (P.niz < 1 || P.nix < 1 || (P.ncomp != 1 && P.ncomp != 2) || !P.fmc || !P.image || !Q->factor || kind < 1 || kind > 3 ||
      (kind == 3 && P.ncomp != 2))
    return hipErrorInvalidValue;
  const dim3 block(64, af::kTfmCohRows), grid((P.nix + 63) / 64, (P.niz + af::kTfmCohRows - 1) / af::kTfmCohRows);
  if (P.ncomp == 2) {
    if (kind == 1) return af::launch_coh<2, 1>(*Q, chunk, grid, block, stream);
    if (kind == 2) return af::launch_coh<2, 2>(*Q, chunk, grid, block, stream);
    return af::launch_coh<2, 3>(*Q, chunk, grid, block, stream);
  }
  return kind == 1 ? af::launch_coh<1, 1>(*Q, chunk, grid, block, stream)
                   : af::launch_coh<1, 2>(*Q, chunk, grid, block, stream);
}
