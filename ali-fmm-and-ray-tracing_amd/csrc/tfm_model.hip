// tfm_model.hip — FMC modelling over resident travel-time fields, the transpose of the TFM sum
// (include/alifmm.h alifmm_tfm_model).  Workgroups own traces: a workgroup takes one transmitter a
// and RG receivers (kTfmModelRx) and holds the current time tile of their traces in LDS as float64.
// It streams its slab of the non-zero pixels in list order (the host compacted the map, so a zero
// pixel costs nothing here; the list keeps the window's raster order, so a dense map reads the
// fields coalesced), reads T_a once and T_b per receiver, and adds c0 and c1 with LDS float64
// atomics.  Neighbouring pixels have neighbouring delays, so the lanes of a wave often hit the same
// sample, and same-address LDS atomics serialise (measured: 8 x from 64 distinct samples to one,
// DESIGN §3); a wave whose lanes fall into at most P.combine runs of neighbouring lanes that share a
// sample first sums each run with a segmented DPP scan, and the run's last lane alone adds.  Then
// the workgroup flushes the tile: plain stores with one slab, float64 atomic adds into the zeroed
// output with several (slabs give small ntx * nrx enough workgroups).  A trace longer than the tile
// is done in time tiles, the pixels streamed again per tile.  The term, the tile membership of its
// two adds and the pixel pass are tfm_model_term.h's (shared with tests/tfm_model_sim.cpp).
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace af {

constexpr int kTfmModelThreads = 1024;  // 16 waves: the field reads of a CU's one large tile need the occupancy

// v of the lane a DPP control names (row_shr:n = 0x110 + n within a row of 16 lanes; row_bcast:15 =
// 0x142, lane 15 of a row to the next row; row_bcast:31 = 0x143, lane 31 to rows 2 and 3), rows
// outside ROWS and lanes without a source get 0
template <int CTRL, int ROWS>
__device__ inline double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWS, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWS, 0xf, false);
  return __hiloint2double(hi, lo);
}

template <int NC, int CTRL, int ROWS>
__device__ inline void scan_step(TfmModelSplit<NC>& s, bool take) {
#pragma unroll
  for (int c = 0; c < NC; c++) {
    const double t0 = dpp_f64<CTRL, ROWS>(s.c0[c]), t1 = dpp_f64<CTRL, ROWS>(s.c1[c]);
    s.c0[c] = take ? s.c0[c] + t0 : s.c0[c];
    s.c1[c] = take ? s.c1[c] + t1 : s.c1[c];
  }
}

// Segmented inclusive scan over the wave: runs of neighbouring lanes with the same s.k (every lane
// of the wave active).  Afterwards the last lane of each run holds the run's sums; returns whether
// this lane is one.  A run of one lane keeps its values bit for bit.  A wave with more than
// max_runs runs adds as it is (true for every lane): the scan costs more than its few collisions.
template <int NC>
__device__ inline bool wave_combine(TfmModelSplit<NC>& s, int max_runs) {
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(s.k, 1);
  const unsigned long long heads = __ballot(lane == 0 || prev != s.k);
  if (__popcll(heads) > max_runs) return true;  // (uniform over the wave)
  const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));  // this lane's run begins here
  const int l16 = lane & 15;
  scan_step<NC, 0x111, 0xf>(s, l16 >= 1 && lane - 1 >= start);
  scan_step<NC, 0x112, 0xf>(s, l16 >= 2 && lane - 2 >= start);
  scan_step<NC, 0x114, 0xf>(s, l16 >= 4 && lane - 4 >= start);
  scan_step<NC, 0x118, 0xf>(s, l16 >= 8 && lane - 8 >= start);
  scan_step<NC, 0x142, 0xa>(s, (lane & 16) && start < (lane & 48));
  scan_step<NC, 0x143, 0xc>(s, lane >= 32 && start < 32);
  return lane == 63 || ((heads >> (lane + 1)) & 1);
}

template <int NC, int RG, bool COMBINE>
__global__ __launch_bounds__(kTfmModelThreads) void tfm_model_kernel(TfmModelParams P) {
  extern __shared__ double tile[];
  const int ngrp = (P.nrx + RG - 1) / RG;
  const int a = blockIdx.x / ngrp, b0 = (blockIdx.x % ngrp) * RG;
  const int tid = threadIdx.x;
  int64_t p0, p1;
  tfm_model_slab(P.npix, P.slabs, blockIdx.y, p0, p1);
  auto add = [](double* p, double v) { unsafeAtomicAdd(p, v); };
  for (int lo = 0; lo < P.nt; lo += P.tile) {
    const int len = P.nt - lo < P.tile ? P.nt - lo : P.tile;
    const int per = len * NC, n = RG * per;
    for (int i = tid; i < n; i += kTfmModelThreads) tile[i] = 0.0;
    __syncthreads();
    // every thread makes every trip (a wave combines with all its lanes); past the slab nothing counts
    for (int64_t q = p0; q < p1; q += kTfmModelThreads)
      tfm_model_pixel<NC, RG>(P, a, b0, q + tid, q + tid < p1, p0, lo, len, [&](int r, TfmModelSplit<NC> s) {
        if (COMBINE) {
          const bool last = wave_combine<NC>(s, P.combine);
          s.in0 &= last;
          s.in1 &= last;
        }
        tfm_model_add<NC>(s, lo, tile + (int64_t)r * per, add);
      });
    __syncthreads();
    for (int i = tid; i < n; i += kTfmModelThreads) {
      const int r = i / per, rem = i - r * per;
      if (b0 + r >= P.nrx) break;  // (r does not decrease with i)
      double* o = P.out + (((int64_t)a * P.nrx + (b0 + r)) * P.nt + lo) * NC + rem;
      const double v = tile[i];
      if (P.slabs == 1) *o = v;
      else if (v != 0.0) unsafeAtomicAdd(o, v);
    }
    __syncthreads();
  }
}

template <int NC, int RG, bool COMBINE>
static hipError_t launch(const TfmModelParams& P, hipStream_t stream) {
  const size_t lds = (size_t)RG * P.tile * NC * sizeof(double);
  hipError_t e = hipFuncSetAttribute((const void*)tfm_model_kernel<NC, RG, COMBINE>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)P.ntx * (unsigned)((P.nrx + RG - 1) / RG), P.slabs);
  hipLaunchKernelGGL((tfm_model_kernel<NC, RG, COMBINE>), grid, dim3(kTfmModelThreads), lds, stream, P);
  return hipGetLastError();
}

template <int NC, bool COMBINE>
static hipError_t launch_rg(const TfmModelParams& P, hipStream_t stream) {
  if (P.rg == 1) return launch<NC, 1, COMBINE>(P, stream);
  if (P.rg == 4) return launch<NC, 4, COMBINE>(P, stream);
  return launch<NC, 2, COMBINE>(P, stream);
}

}  // namespace af

// P->rg 1, 2 or 4; P->tile as tfm_model_tile() gives it; 1 <= P->slabs <= 64, > 1 needs P->out zeroed
extern "C" hipError_t af_launch_tfm_model(const af::TfmModelParams* P, hipStream_t stream) {
  if (P->npix < 1 || P->ntx < 1 || P->nrx < 1 || P->nt < 2 || (P->ncomp != 1 && P->ncomp != 2) || P->slabs < 1 ||
      P->slabs > 64 || (P->rg != 1 && P->rg != 2 && P->rg != 4) || P->tile < 1 ||
      P->tile != af::tfm_model_tile(P->tile, P->nt, P->ncomp, P->rg))
    return hipErrorInvalidValue;
  if ((int64_t)P->ntx * ((P->nrx + P->rg - 1) / P->rg) > 0x7fffffffLL) return hipErrorInvalidValue;
  if (P->combine)
    return P->ncomp == 2 ? af::launch_rg<2, true>(*P, stream) : af::launch_rg<1, true>(*P, stream);
  return P->ncomp == 2 ? af::launch_rg<2, false>(*P, stream) : af::launch_rg<1, false>(*P, stream);
}
