// tfm.hip — TFM delay-and-sum over resident travel-time fields (include/alifmm.h alifmm_tfm).
// One thread per pixel; a wave covers 64 consecutive x of one image row (coalesced field reads at
// step 1), a workgroup kTfmRows rows.  Each thread keeps the delays of RC receivers in registers,
// walks every transmitter for that chunk (one T_a load per transmitter and chunk) and gathers the
// two neighbouring samples of each pair's A-scan through L1 / L2; neighbouring pixels have
// neighbouring delays, so a wave's gathers fall into a few cache lines of that A-scan.  The
// accumulators stay in registers across chunks; one image store at the end.  Tail tiles, step > 1
// and nrx not a multiple of RC go through the same code with predicates.  The per-pixel arithmetic
// and its order are tfm_term.h's (shared with tests/tfm_sim.cpp).  The float64 instantiation
// (alifmm_tfm_f64, and the Aᵀ of alifmm_tfm_lsq) is the same kernel with 8-byte samples: a complex
// pair of neighbouring samples is 32 bytes, two 16-byte loads per term.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace af {

constexpr int kTfmRows = 4;  // waves (image rows) per workgroup

template <int NC, int RC, class S>
__global__ __launch_bounds__(64 * kTfmRows) void tfm_kernel(TfmParams P) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  const int i = blockIdx.y * kTfmRows + threadIdx.y;
  if (i >= P.niz || j >= P.nix) return;
  double acc[NC];
  tfm_pixel<NC, RC, S>(P, tfm_pixel_offset(P, i, j), acc);
  double* o = P.image + ((int64_t)i * P.nix + j) * NC;
#pragma unroll
  for (int c = 0; c < NC; c++) o[c] = acc[c];
}

template <int NC, class S>
static hipError_t launch_nc(const TfmParams& P, int chunk, dim3 grid, dim3 block, hipStream_t stream) {
  if (chunk == 4) hipLaunchKernelGGL((tfm_kernel<NC, 4, S>), grid, block, 0, stream, P);
  else if (chunk == 16) hipLaunchKernelGGL((tfm_kernel<NC, 16, S>), grid, block, 0, stream, P);
  else if (chunk == 32) hipLaunchKernelGGL((tfm_kernel<NC, 32, S>), grid, block, 0, stream, P);
  else hipLaunchKernelGGL((tfm_kernel<NC, kTfmChunk, S>), grid, block, 0, stream, P);
  return hipGetLastError();
}

}  // namespace af

// chunk: receivers per register chunk, 4, 8, 16 or 32 (anything else: kTfmChunk)
template <class S>
static hipError_t launch_tfm(const af::TfmParams* P, int chunk, hipStream_t stream) {
  if (P->niz < 1 || P->nix < 1 || (P->ncomp != 1 && P->ncomp != 2) || !af::tfm_samples<S>(*P)) return hipErrorInvalidValue;
  const dim3 block(64, af::kTfmRows), grid((P->nix + 63) / 64, (P->niz + af::kTfmRows - 1) / af::kTfmRows);
  return P->ncomp == 2 ? af::launch_nc<2, S>(*P, chunk, grid, block, stream)
                       : af::launch_nc<1, S>(*P, chunk, grid, block, stream);
}

extern "C" hipError_t af_launch_tfm(const af::TfmParams* P, int chunk, hipStream_t stream) {
  return launch_tfm<float>(P, chunk, stream);
}

// the same over the float64 samples P->fmc64
extern "C" hipError_t af_launch_tfm_f64(const af::TfmParams* P, int chunk, hipStream_t stream) {
  return launch_tfm<double>(P, chunk, stream);
}
