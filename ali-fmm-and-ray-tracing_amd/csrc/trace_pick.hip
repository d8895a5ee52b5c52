// trace_pick.hip — the time-of-flight picker on the device (include/alifmm.h alifmm_trace_pick): per
// trace the peak of the energy inside a gate, its runner-up outside a guard, the onset and the
// refinement to a fractional sample.  The rules, the key order and a lane's two walks are
// trace_pick_term.h's, shared with tests/trace_pick_sim.cpp.
//
// One wavefront per trace, kPickWaves of them per workgroup; a wavefront walks the traces with the
// stride of all the launch's wavefronts and every sample offset is 64-bit.  Lane l reads samples
// lo + l, lo + l + 64, ... (consecutive lanes read consecutive samples: 4 to 16 bytes per lane) into
// its best key, and the 64 keys are combined over the lane distances 32 .. 1; the order is total, so
// every lane ends with the same key.  The runner-up and the onset need the peak, so they take a
// second walk over the gate, which the first one left in the cache.  Lane 0 refines and stores.
// No LDS, no barrier, no atomics.  A lane without a sample (a gate shorter than 64) carries the
// "none" key into the butterfly; a wavefront without a trace (a count that is no multiple of
// kPickWaves) leaves whole, so every shuffle sees all 64 lanes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace af {

constexpr int kPickWaves = 4;         // traces per workgroup
constexpr int kPickMaxBlocks = 2048;  // workgroups of a launch ("trace_pick_grid"): 8 per CU
static_assert(kPickLanes == 64, "one wavefront per trace");

__device__ inline PickKey pick_wave_max(PickKey k) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    PickKey o;
    o.e = __shfl_xor(k.e, d, 64);
    o.n = __shfl_xor(k.n, d, 64);
    k = pick_key_max(k, o);
  }
  return k;
}

template <typename T, int NC>
__global__ __launch_bounds__(64 * kPickWaves) void trace_pick_kernel(TracePickParams P) {
  const int lane = threadIdx.x & 63;
  const T* in = static_cast<const T*>(P.in);
  const int64_t stride = (int64_t)gridDim.x * kPickWaves;
  for (int64_t t = (int64_t)blockIdx.x * kPickWaves + (threadIdx.x >> 6); t < P.ntrace; t += stride) {
    const int lo = P.lo[t], hi = P.hi[t];
    PickOut o = pick_out_none(kPickNoGate);
    // (the host unit refuses a gate that leaves the trace; none is ever read through)
    if (lo < hi && lo >= 0 && hi <= P.nt) {
      const T* x = in + t * (int64_t)P.nt * NC;
      int bad = 0;
      PickKey best = pick_wave_max(pick_lane_peak<T, NC>(x, lo, hi, lane, &bad));
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) bad |= __shfl_xor(bad, d, 64);
      PickKey second = pick_key_none();
      int onset = -1;
      if (pick_has_peak(best)) {  // the same for all 64 lanes
        const double thr = pick_threshold(P.frac, best.e);
        second = pick_wave_max(pick_lane_second<T, NC>(x, lo, hi, lane, best.n, P.guard, P.mode, thr, &onset));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) onset = pick_idx_min(onset, __shfl_xor(onset, d, 64));
      }
      if (lane == 0) o = pick_refine<T, NC>(x, P.nt, lo, hi, P.mode, P.frac, best, bad, second, onset);
    }
    if (lane == 0) {
      P.pos[t] = o.pos;
      P.amp[t] = o.amp;
      P.idx[t] = o.idx;
      P.amp2[t] = o.amp2;
      P.idx2[t] = o.idx2;
      P.flags[t] = o.flags;
    }
  }
}

template <typename T, int NC>
static hipError_t launch(const TracePickParams& P, hipStream_t stream) {
  const int64_t nblock = (P.ntrace + kPickWaves - 1) / kPickWaves;
  const dim3 grid((unsigned)std::min<int64_t>(nblock, kPickMaxBlocks));
  hipLaunchKernelGGL((trace_pick_kernel<T, NC>), grid, dim3(64 * kPickWaves), 0, stream, P);
  return hipGetLastError();
}

}  // namespace af

using namespace af;

extern "C" int af_trace_pick_grid() { return kPickMaxBlocks; }

extern "C" hipError_t af_launch_trace_pick(const TracePickParams* P, int ncomp, int dtype, hipStream_t stream) {
  if (P->ntrace < 1 || P->nt < 1 || !(ncomp == 1 || ncomp == 2) || !(dtype == 0 || dtype == 1) ||
      !(P->mode == 0 || P->mode == 1) || (P->mode == 1 && !(P->frac > 0.0 && P->frac <= 1.0)) || P->guard < 0 || !P->in ||
      !P->lo || !P->hi || !P->pos || !P->amp || !P->idx || !P->amp2 || !P->idx2 || !P->flags)
    return hipErrorInvalidValue;
  if (dtype == 0) return ncomp == 1 ? launch<double, 1>(*P, stream) : launch<double, 2>(*P, stream);
  return ncomp == 1 ? launch<float, 1>(*P, stream) : launch<float, 2>(*P, stream);
}
