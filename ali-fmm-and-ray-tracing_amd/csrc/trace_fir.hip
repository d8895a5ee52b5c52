// trace_fir.hip — the per-trace FIR P and its exact transpose Pᵀ on the device (include/alifmm.h
// alifmm_trace_fir; around the two kernels of the CGLS loop in alifmm_tfm_lsq_pulse).  The sum, its
// order and the tiled walk's index mappings are trace_fir_term.h's, shared with
// tests/trace_fir_sim.cpp.
//
// One workgroup per (trace, tile of kFirTile consecutive outputs); the flattened (trace, tile)
// space is walked with the grid's stride.  The tile's segment of kFirTile + ntap - 1 samples (zeros
// outside the trace) and the taps are staged in LDS; the forward sum stages the segment descending
// and stores its outputs descending, so both directions run the same loop.  A thread makes
// kFirOutPerThread consecutive outputs, one accumulator each, taps ascending, through a sliding
// window of as many samples in registers: a tap costs it one sample read and one (broadcast) tap
// read from LDS, and its outputs' dependent-add chains overlap.  The segment lies in LDS by
// trace_fir_slot (position i in row i mod 4), so the lanes of a wave read consecutive 8- or 16-byte
// samples: ds_read_b64 / ds_read_b128 without bank conflicts.  Every trace offset is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace af {

constexpr int kFirTile = 1024;  // outputs of a workgroup's tile ("trace_fir_tile")
constexpr int kFirBlock = kFirTile / kFirOutPerThread;
constexpr int kFirMaxBlocks = 4096;  // workgroups of a launch: 16 per CU, each walking its share of the tiles
// the largest staging buffer and the taps: a workgroup's dynamic LDS stays within the default limit
static_assert((4 * ((kFirTile + kFirMaxTaps - 1 + 3) / 4) * 2 + kFirMaxTaps * 2) * sizeof(double) <= 65536, "LDS");

template <int NC, int TC>
__global__ __launch_bounds__(kFirBlock) void trace_fir_kernel(TraceFirParams P) {
  extern __shared__ __align__(16) double fir_lds[];
  const int tid = threadIdx.x, ntap = P.ntap, nt = P.nt;
  const int seg = trace_fir_seg(kFirTile, ntap), quarter = trace_fir_quarter(seg);
  double* s = fir_lds;                               // [4 * quarter][NC], trace_fir_slot
  double* g = fir_lds + (size_t)4 * quarter * NC;    // [ntap][TC] staged taps
  for (int j = tid; j < ntap; j += kFirBlock) trace_fir_stage_tap<TC>(P.taps, j, P.transpose, g + (size_t)j * TC);
  const int64_t ntiles = ((int64_t)nt + kFirTile - 1) / kFirTile, total = P.ntrace * ntiles;
  for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const int64_t trace = w / ntiles, t0 = (w % ntiles) * kFirTile;
    const double* x = P.in + trace * (int64_t)nt * NC;
    double* y = P.out + trace * (int64_t)nt * NC;
    __syncthreads();  // the previous tile's reads are over
    for (int i = tid; i < seg; i += kFirBlock) trace_fir_stage<NC>(x, nt, P.transpose, t0, kFirTile, P.origin, i, quarter, s);
    __syncthreads();
    double acc[kFirOutPerThread][NC];
    trace_fir_thread<NC, TC>(s, quarter, g, ntap, tid, acc);
    for (int r = 0; r < kFirOutPerThread; r++)
      trace_fir_store<NC>(y, nt, P.transpose, t0, kFirTile, kFirOutPerThread * tid + r, acc[r]);
  }
}

}  // namespace af

using namespace af;

extern "C" int af_trace_fir_tile() { return kFirTile; }

extern "C" hipError_t af_launch_trace_fir(const TraceFirParams* P, int ncomp, int tap_comp, hipStream_t stream) {
  if (P->ntrace < 1 || P->nt < 1 || P->ntap < 1 || P->ntap > kFirMaxTaps || P->origin < 0 || P->origin >= P->ntap ||
      (P->transpose != 0 && P->transpose != 1) || !(ncomp == 1 || ncomp == 2) || !(tap_comp == 1 || tap_comp == 2) ||
      tap_comp > ncomp || P->in == P->out)
    return hipErrorInvalidValue;
  const int64_t total = P->ntrace * (((int64_t)P->nt + kFirTile - 1) / kFirTile);
  const dim3 grid((unsigned)std::min<int64_t>(total, kFirMaxBlocks));
  const size_t lds =
      ((size_t)4 * trace_fir_quarter(trace_fir_seg(kFirTile, P->ntap)) * ncomp + (size_t)P->ntap * tap_comp) * sizeof(double);
  if (ncomp == 1) hipLaunchKernelGGL((trace_fir_kernel<1, 1>), grid, dim3(kFirBlock), lds, stream, *P);
  else if (tap_comp == 1) hipLaunchKernelGGL((trace_fir_kernel<2, 1>), grid, dim3(kFirBlock), lds, stream, *P);
  else hipLaunchKernelGGL((trace_fir_kernel<2, 2>), grid, dim3(kFirBlock), lds, stream, *P);
  return hipGetLastError();
}
